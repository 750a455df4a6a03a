"""GPU: the EMBEDDED BA window (N2b, include/nrs.h) sharded over a communicator (last bullet: "points sharded, node-side
contributions all-reduced").

As in tests/test_gpu_sharded.py the ranks are THREADS of this process, their contexts on the one GPU of the test box
(nrs_comm_init_local), and the RCCL back end is exercised with world = 1.  A rank holds the skinned observations of its own keyframe
range only: they reach node copies of their own keyframe, so the exchange steps are the plain window's (pose blocks, chi2, max
diagonal and PCG dot products all-reduced, boundary rows of the neighbour keyframes).  On a communicator the window solves by the
block-Jacobi PCG whatever nrs_options.embedded_solver says.  Held against the unsharded block-Jacobi PCG (embedded_solver = 2) at the
tolerances of the sharded plain window, against oracle/embedded_oracle.py and against the C2 x 500 golden."""
import os
import sys
import threading

import numpy as np
import pytest

import embedded_oracle as E
import nrs
import nrs_synth as S

pytestmark = pytest.mark.gpu


def _setup(n, k, m, seed, model=S.PINHOLE):
    p = S.make_dba_problem(n, k, seed, model)
    flag, nb = S.embedded_problem(p, m)
    p["nbr_nodes"] = nb
    e = nrs.dba_build_edges_embedded(p["kf_points"], flag, nb)
    w = S.embedded_window(p, e)
    cam = nrs.make_camera(p["model"], p["prm"])
    qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
    return p, e, w, cam, qt


def _oracle(p, e, w, iters=5, trace=None):
    return E.dba_solve_embedded(p["model"], p["prm"], p["poses_q"], p["poses_t"], w["lm_xyz"], w["lm_kf"], w["lm_uv"], e["sp_ij"], e["sp_d0"],
                                e["dm_idx"], e["dm_w"], w["sk_kf"], w["sk_uv"], w["sk_xyz"], e["sk_node"], e["sk_omega"], p["scale"], iters, trace)


def _unsharded(p, e, w, cam, qt, iters=5, exact=0):
    c = nrs.Context(embedded_solver=2, exact_trials=exact)
    c.dba_upload_embedded(cam, qt, w, e, p["scale"])
    tr = nrs.Trace()
    c.dba_optimize(iters, tr)
    pq, xyz = c.dba_download()
    sk = c.dba_download_skinned()
    st = c.dba_skin_stats()
    c.close()
    return tr.trials, pq, xyz, sk, st


def _run_sharded(world, p, e, w, cam, qt, iters=5, exact=0, solver=2, resets=0, one_shot=False):
    """every rank: upload (or the one-shot solve), optimize, download; returns per rank dict(trials, pq, xyz, sk, kft, skin, stats, runs)"""
    group = nrs.LocalGroup(world)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            c = nrs.Context(exact_trials=exact, embedded_solver=solver)
            c.comm_init_local(group, r)
            assert c.comm_rank() == (r, world)
            tr = nrs.Trace()
            runs = []
            if one_shot:
                pq, xyz, sk = c.dba_solve_embedded(cam, qt, w, e, p["scale"], iters, tr)
            else:
                c.dba_upload_embedded(cam, qt, w, e, p["scale"])
                c.dba_optimize(iters, tr)
                pq, xyz = c.dba_download()
                sk = c.dba_download_skinned()
                for _ in range(resets):
                    c.dba_reset()
                    t2 = nrs.Trace()
                    c.dba_optimize(iters, t2)
                    q2, x2 = c.dba_download()
                    runs.append((t2.trials, q2, x2, c.dba_download_skinned()))
            kft = None if one_shot else c.debug_kft_info()["on"]
            out[r] = dict(trials=tr.trials, iters=tr.iterations, pq=pq, xyz=xyz, sk=sk, kft=kft, skin=c.dba_skin_stats(),
                          stats=c.dba_stats(), runs=runs)
            c.close()
        except Exception as ex:                      # a failed rank would leave the others in the barrier
            errs.append((r, ex))
            raise

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    assert not errs, errs
    assert all(o is not None for o in out), "a rank did not finish"
    group.close()
    return out


def _same_trials(a, b, rtol=1e-6):
    """(the rules of tests/test_gpu_sharded.py: where an early-rejected trial stops depends on the batching of the inner solve)"""
    assert [t["accepted"] for t in a] == [t["accepted"] for t in b]
    for x, y in zip(a, b):
        assert abs(x["lam"] - y["lam"]) <= rtol * abs(y["lam"])
        assert abs(x["chi"] - y["chi"]) <= rtol * abs(y["chi"])
        assert not (x["early"] or y["early"]) or not (x["accepted"] or y["accepted"])
        if not y["early"] and not x["early"]:
            assert abs(x["chi_new"] - y["chi_new"]) <= rtol * abs(y["chi_new"])


def _key(trials):
    return [(t["accepted"], t["lam"], t["chi"], t["chi_new"], t["inner"], t["early"]) for t in trials]


def _close(o, ref):
    trials, pq, xyz, sk = ref[:4]
    _same_trials(o["trials"], trials)
    assert np.allclose(o["pq"][:, :4], pq[:, :4], atol=1e-6, rtol=0) and np.allclose(o["pq"][:, 4:], pq[:, 4:], atol=1e-5, rtol=0)
    assert np.allclose(o["xyz"], xyz, atol=1e-4, rtol=0)
    assert np.allclose(o["sk"], sk, atol=1e-4, rtol=0)


def _bit_identical(a, b):
    assert _key(a["trials"]) == _key(b["trials"])
    for f in ("pq", "xyz", "sk"):
        assert np.array_equal(a[f], b[f]), f


CASES = [(300, 4, 40, 53, S.PINHOLE), (600, 6, 80, 54, S.PINHOLE), (400, 5, 60, 55, S.KB8)]


@pytest.mark.parametrize("n,k,m,seed,model", CASES)
def test_sharded_matches_unsharded(n, k, m, seed, model):
    p, e, w, cam, qt = _setup(n, k, m, seed, model)
    ref = _unsharded(p, e, w, cam, qt)
    assert sum(t["inner"] for t in ref[0] if not t["early"]) > 20 * len(ref[0])
    for world in (2, 3, 4):
        out = _run_sharded(world, p, e, w, cam, qt)
        for r in range(world):
            _close(out[r], ref)
            assert out[r]["kft"] is False
        for r in range(1, world):                   # every rank holds the same complete result, bit for bit
            _bit_identical(out[r], out[0])


@pytest.mark.parametrize("exact", [0, 1])
def test_sharded_one_shot_matches_oracle(exact):
    """nrs_dba_solve_embedded on a communicator (collective: its download of the skinned points included)"""
    p, e, w, cam, qt = _setup(300, 4, 40, 53)
    out = _run_sharded(2, p, e, w, cam, qt, exact=exact, one_shot=True)
    otr = []
    oq, ot, opts, osk, nit = _oracle(p, e, w, 5, otr)
    _bit_identical(out[1], out[0])
    o = out[0]
    assert o["iters"] == nit
    assert [t["accepted"] for t in o["trials"]] == [t["accepted"] for t in otr]
    for a, b in zip(o["trials"], otr):
        assert (a["iter"], a["trial"]) == (b["iter"], b["trial"])
        assert abs(a["lam"] - b["lam"]) <= 1e-6 * b["lam"]
        assert abs(a["chi"] - b["chi"]) <= 1e-6 * b["chi"]
        if a["early"]:
            assert not exact and not a["accepted"] and not b["accepted"] and b["rho"] < -0.02
        else:
            assert abs(a["chi_new"] - b["chi_new"]) <= 1e-6 * b["chi_new"]
    assert np.allclose(o["pq"][:, :4], oq, atol=1e-6, rtol=0)
    assert np.allclose(o["pq"][:, 4:], ot, atol=1e-5, rtol=0)
    assert np.allclose(o["xyz"], opts, atol=1e-4, rtol=0)
    assert np.allclose(o["sk"], osk, atol=1e-4, rtol=0)


def test_a_communicator_means_block_jacobi_pcg():
    """embedded_solver 0 (cost model), 1 (always the factorisation) and 2 (PCG): the keyframe-block factorisation is not sharded, so all
    three run the block-Jacobi PCG on a communicator -- the same bits, PCG-sized inner iteration counts"""
    p, e, w, cam, qt = _setup(400, 5, 60, 55)
    outs = [_run_sharded(2, p, e, w, cam, qt, solver=s) for s in (0, 1, 2)]
    for out in outs:
        for o in out:
            assert o["kft"] is False
            assert sum(t["inner"] for t in o["trials"] if not t["early"]) > 20 * len(o["trials"])
        _bit_identical(out[0], outs[2][0])
        _bit_identical(out[1], outs[2][0])


@pytest.mark.parametrize("switch", ["NRS_SKIN_OP_OWN_LAUNCH", "NRS_SKIN_ROWS_OWN_LAUNCH", "NRS_SHARD_FULL_VECTORS"])
def test_launch_forms_give_the_same_bits(switch):
    """k_skin_op / the observations' row pass in launches of their own, and every row held on every rank: the same arithmetic"""
    p, e, w, cam, qt = _setup(600, 6, 80, 54)
    a = _run_sharded(3, p, e, w, cam, qt)
    nrs.debug_set(switch, "1")
    try:
        b = _run_sharded(3, p, e, w, cam, qt)
    finally:
        nrs.debug_set(switch, None)
    assert sum(t["inner"] for t in a[0]["trials"]) > 50
    for r in range(3):
        _bit_identical(a[r], b[r])


def test_reset_is_reproducible():
    """upload once, then reset + optimize three times: the same bits every time (the first lambda comes from the max diagonal, which
    must not see the previous solve's all-reduced pose blocks of poses another rank owns)"""
    p, e, w, cam, qt = _setup(500, 5, 70, 56)
    ref = _unsharded(p, e, w, cam, qt)
    out = _run_sharded(2, p, e, w, cam, qt, resets=3)
    for o in out:
        _close(o, ref)
        assert len(o["runs"]) == 3
        for trials, pq, xyz, sk in o["runs"]:
            assert _key(trials) == _key(o["trials"])
            assert np.array_equal(pq, o["pq"]) and np.array_equal(xyz, o["xyz"]) and np.array_equal(sk, o["sk"])
    _bit_identical(out[1], out[0])


def test_a_rank_holds_the_skinned_observations_of_its_own_keyframes():
    p, e, w, cam, qt = _setup(500, 8, 80, 62)
    world = 4
    kb = nrs.shard_plan(8, w["lm_kf"], world)
    assert kb.tolist() == [0, 2, 4, 6, 8]                            # an even share
    whole = _unsharded(p, e, w, cam, qt)[4]
    n_skin = len(w["sk_kf"])
    assert whole[0] == n_skin
    out = _run_sharded(world, p, e, w, cam, qt)
    assert sum(o["skin"][0] for o in out) == n_skin
    for r, o in enumerate(out):
        own = (w["sk_kf"] >= kb[r]) & (w["sk_kf"] < kb[r + 1])
        assert o["skin"][0] == own.sum()
        cnt = np.bincount(w["sk_kf"][own] - kb[r], minlength=kb[r + 1] - kb[r])
        assert o["skin"][1] == 256 * sum((c + 255) // 256 for c in cnt)
        assert o["skin"][2] <= 1.3 * whole[2] / world + 8 * o["stats"]["rows"] + 64 * 1024


@pytest.mark.parametrize("exact", [1, 0])
def test_full_size_c2_with_500_nodes_sharded_matches_the_oracle_golden(exact):
    """BASELINE configs[1] as written (C2: 5k points x 500 nodes x 20 keyframes) over 4 ranks, against
    tests/golden/dba_C2_embedded500_trace.npz with the checks of tests/test_gpu_embedded_ba.py"""
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    from make_embedded_ba_golden import skin_checksum
    g = np.load(os.path.join(here, "golden", "dba_C2_embedded500_trace.npz"))
    p = S.make_dba_problem("C2")
    flag, nb = S.embedded_problem(p, int(g["n_nodes"]))
    e = nrs.dba_build_edges_embedded(p["kf_points"], flag, nb)
    assert (int(g["n_lm"]), int(g["n_skin"]), int(g["n_sp"]), int(g["n_dm"])) == (len(e["lm_obs"]), len(e["sk_obs"]), len(e["sp_ij"]), len(e["dm_idx"]))
    assert int(g["edge_checksum"]) == S.edge_checksum(e) and int(g["skin_checksum"]) == skin_checksum(e)
    w = S.embedded_window(p, e)
    cam = nrs.make_camera(p["model"], p["prm"])
    qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
    out = _run_sharded(4, p, e, w, cam, qt, exact=exact)
    for o in out[1:]:
        _bit_identical(o, out[0])
    o = out[0]
    t = o["trials"]
    assert o["iters"] == int(g["out_iters"])
    assert [x["accepted"] for x in t] == g["out_accepted"].tolist()
    for x, chi, chi_new, lam in zip(t, g["out_chi"], g["out_chi_new"], g["out_lam"]):
        assert abs(x["lam"] - lam) <= 1e-6 * lam and abs(x["chi"] - chi) <= 1e-6 * chi
        if not x["early"]:
            assert abs(x["chi_new"] - chi_new) <= 1e-6 * chi_new
    pq, xyz, sk = o["pq"], o["xyz"], o["sk"]
    assert np.allclose(pq[:, :4], g["out_q"], atol=1e-6, rtol=0) and np.allclose(pq[:, 4:], g["out_t"], atol=1e-5, rtol=0)
    assert np.allclose(xyz[g["sel"]], g["out_pts_sel"], atol=1e-4, rtol=0) and np.allclose(sk[g["ssel"]], g["out_sk_sel"], atol=1e-4, rtol=0)
    assert np.allclose(xyz.sum(0), g["out_pts_sum"], atol=1e-4 * np.sqrt(len(xyz)), rtol=0)
    assert np.allclose(sk.sum(0), g["out_sk_sum"], atol=1e-4 * np.sqrt(len(sk)), rtol=0)


def test_rccl_backend_single_rank():
    """the embedded window on the sharded code path with every exchange step through librccl (world = 1)"""
    p, e, w, cam, qt = _setup(400, 5, 60, 55, S.KB8)
    ref = _unsharded(p, e, w, cam, qt)
    c = nrs.Context(embedded_solver=2)
    c.comm_init_rccl(1, 0, nrs.comm_unique_id())
    c.dba_upload_embedded(cam, qt, w, e, p["scale"])
    assert c.debug_kft_info()["on"] is False
    tr = nrs.Trace()
    c.dba_optimize(5, tr)
    pq, xyz = c.dba_download()
    o = dict(trials=tr.trials, pq=pq, xyz=xyz, sk=c.dba_download_skinned())
    assert c.dba_skin_stats()[0] == len(w["sk_kf"])
    c.close()
    _close(o, ref)


def test_errors_are_still_errors():
    # more ranks than keyframes
    p, e, w, cam, qt = _setup(200, 3, 30, 57)
    group = nrs.LocalGroup(4)
    c = nrs.Context()
    c.comm_init_local(group, 0)
    with pytest.raises(nrs.NrsError) as ei:
        c.dba_upload_embedded(cam, qt, w, e, p["scale"])
    assert ei.value.code == -1
    c.close()
    group.close()
    # a skinned observation reaching a node copy of another keyframe: rejected by the rank that holds it, and every rank fails
    bad = dict(e, sk_node=e["sk_node"].copy())
    other = np.where(w["lm_kf"] != w["sk_kf"][0])[0][0]
    bad["sk_node"][0, 0] = other
    group = nrs.LocalGroup(2)
    codes = [None, None]

    def rank_main(r):
        c = nrs.Context()
        c.comm_init_local(group, r)
        try:
            c.dba_upload_embedded(cam, qt, w, bad, p["scale"])
            codes[r] = 0
        except nrs.NrsError as ex:
            codes[r] = ex.code
        c.close()

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    group.close()
    owner = 0 if w["sk_kf"][0] < nrs.shard_plan(3, w["lm_kf"], 2)[1] else 1
    assert codes[owner] == -1 and codes[1 - owner] not in (None, 0)
