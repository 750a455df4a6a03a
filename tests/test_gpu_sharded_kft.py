"""GPU: the keyframe-block factorisation of an EMBEDDED BA window sharded over a communicator (nrs_options.sharded_kft = 1).

A rank holds and inverts the blocks of its own keyframes; the two elimination chains of the one-GPU schedule are handed from rank to
rank (csrc/nrs_engine_kft.hpp).  Ranks are threads of this process on the one GPU of the test box (nrs_comm_init_local), as in
tests/test_gpu_sharded_embedded.py, whose helpers and tolerances this file reuses; the RCCL back end is exercised with world = 1."""
import os
import sys
import threading

import numpy as np
import pytest

import nrs
import nrs_synth as S
import test_gpu_sharded_embedded as B

pytestmark = pytest.mark.gpu


def _unsharded_kft(p, e, w, cam, qt, iters=5, exact=0):
    c = nrs.Context(embedded_solver=1, exact_trials=exact)
    c.dba_upload_embedded(cam, qt, w, e, p["scale"])
    assert c.debug_kft_info()["on"] is True
    tr = nrs.Trace()
    c.dba_optimize(iters, tr)
    pq, xyz = c.dba_download()
    sk = c.dba_download_skinned()
    share = c.debug_kft_share()
    c.close()
    return tr.trials, pq, xyz, sk, share


def _ranks(world, fn):
    """fn(rank, group) on `world` thread ranks; returns the per-rank results"""
    group = nrs.LocalGroup(world)
    out, errs = [None] * world, []

    def main(r):
        try:
            out[r] = fn(r, group)
        except Exception as ex:
            errs.append((r, ex))
            raise

    th = [threading.Thread(target=main, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(600)
    assert not errs, errs
    assert all(o is not None for o in out), "a rank did not finish"
    group.close()
    return out


def _run(world, p, e, w, cam, qt, solver=1, sharded_kft=1, exact=0, iters=5, resets=0):
    def fn(r, group):
        c = nrs.Context(exact_trials=exact, embedded_solver=solver, sharded_kft=sharded_kft)
        c.comm_init_local(group, r)
        c.dba_upload_embedded(cam, qt, w, e, p["scale"])
        info = c.debug_kft_info()
        on = info["on"]
        share = dict(c.debug_kft_share(), mib=info["mib"]) if on else None
        tr = nrs.Trace()
        c.dba_optimize(iters, tr)
        pq, xyz = c.dba_download()
        sk = c.dba_download_skinned()
        runs = []
        for _ in range(resets):
            c.dba_reset()
            t2 = nrs.Trace()
            c.dba_optimize(iters, t2)
            q2, x2 = c.dba_download()
            runs.append((t2.trials, q2, x2, c.dba_download_skinned()))
        c.close()
        return dict(trials=tr.trials, iters=tr.iterations, pq=pq, xyz=xyz, sk=sk, kft=on, share=share, runs=runs)
    return _ranks(world, fn)


def _inner(trials):
    return sum(t["inner"] for t in trials)


# B.CASES, plus K = 6 over 4 ranks (two ranks hold a single keyframe) and K = 7 over 3 ranks (the middle keyframe 3 opens rank 1's range)
@pytest.mark.parametrize("n,k,m,seed,model,worlds", [c + ((2, 3, 4),) for c in B.CASES] + [(500, 7, 70, 58, S.PINHOLE, (3,))])
def test_sharded_factorisation_matches_unsharded(n, k, m, seed, model, worlds):
    p, e, w, cam, qt = B._setup(n, k, m, seed, model)
    ref = _unsharded_kft(p, e, w, cam, qt)
    for world in worlds:
        out = _run(world, p, e, w, cam, qt)
        for r, o in enumerate(out):
            assert o["kft"] is True
            assert _inner(o["trials"]) <= 3 * len(o["trials"])
            B._close(o, ref)
            sh = o["share"]
            assert sh["m"] == k // 2 and sh["handovers"] == world - 1
        kb = nrs.shard_plan(k, w["lm_kf"], world)
        assert [o["share"]["k0"] for o in out] == kb[:-1].tolist()
        assert [o["share"]["nk"] for o in out] == np.diff(kb).tolist()
        for o in out[1:]:
            B._bit_identical(o, out[0])


def test_middle_keyframe_first_of_its_rank_and_single_keyframe_ranks():
    p, e, w, cam, qt = B._setup(500, 8, 80, 62)
    ref = _unsharded_kft(p, e, w, cam, qt)
    kb = nrs.shard_plan(8, w["lm_kf"], 4)
    assert 4 in kb.tolist()                                             # m = 4 opens a rank's range
    out = _run(4, p, e, w, cam, qt)
    for o in out:
        assert o["kft"] is True and _inner(o["trials"]) <= 3 * len(o["trials"])
        B._close(o, ref)
    p, e, w, cam, qt = B._setup(600, 6, 80, 54)
    ref = _unsharded_kft(p, e, w, cam, qt)
    kb = nrs.shard_plan(6, w["lm_kf"], 4)
    assert 1 in np.diff(kb).tolist()                                    # a rank with a single keyframe
    out = _run(4, p, e, w, cam, qt)
    for o in out:
        assert o["kft"] is True
        B._close(o, ref)
    for o in out[1:]:
        B._bit_identical(o, out[0])


@pytest.mark.parametrize("world", [2, 3, 4])
def test_same_factor_bits(world):
    """M^-1 x and every own diagonal / coupling block: the one-GPU bits"""
    p, e, w, cam, qt = B._setup(600, 6, 80, 54)
    lam = 3.7e2
    c = nrs.Context(embedded_solver=1)
    c.dba_upload_embedded(cam, qt, w, e, p["scale"])
    K = 6
    x = np.random.default_rng(7).standard_normal(6 * K + 3 * len(w["lm_kf"]))
    ref_u = c.debug_kft_apply(lam, x)
    ref_a = [c.debug_kft_block(lam, k) for k in range(K)]
    ref_t = [c.debug_kft_block(lam, k, coupling=True) for k in range(K - 1)]
    c.close()

    def fn(r, group):
        c = nrs.Context(embedded_solver=1, sharded_kft=1)
        c.comm_init_local(group, r)
        c.dba_upload_embedded(cam, qt, w, e, p["scale"])
        u = c.debug_kft_apply(lam, x)
        share = c.debug_kft_share()
        blocks = {}
        for k in range(K):                                             # collective: every rank asks, the holder answers
            for cpl in (False, True):
                if cpl and k == K - 1:
                    continue
                try:
                    blocks[(k, cpl)] = c.debug_kft_block(lam, k, coupling=cpl)
                except nrs.NrsError as ex:
                    assert ex.code == -1
        c.close()
        return dict(u=u, share=share, blocks=blocks)
    out = _ranks(world, fn)
    for o in out:
        assert np.array_equal(o["u"], ref_u)
        own = range(o["share"]["k0"], o["share"]["k0"] + o["share"]["nk"])
        assert sorted(k for k, cpl in o["blocks"] if not cpl) == list(own)
        for (k, cpl), a in o["blocks"].items():
            assert np.array_equal(a, ref_t[k] if cpl else ref_a[k]), (k, cpl)


@pytest.mark.parametrize("exact", [0, 1])
def test_sharded_one_shot_matches_oracle(exact):
    p, e, w, cam, qt = B._setup(300, 4, 40, 53)

    def fn(r, group):
        c = nrs.Context(exact_trials=exact, embedded_solver=1, sharded_kft=1)
        c.comm_init_local(group, r)
        tr = nrs.Trace()
        pq, xyz, sk = c.dba_solve_embedded(cam, qt, w, e, p["scale"], 5, tr)
        c.close()
        return dict(trials=tr.trials, iters=tr.iterations, pq=pq, xyz=xyz, sk=sk)
    out = _ranks(2, fn)
    for o in out:                                                      # the factorisation ran (a PCG fallback needs > 20 a trial)
        assert _inner(o["trials"]) <= 3 * len(o["trials"])
    otr = []
    oq, ot, opts, osk, nit = B._oracle(p, e, w, 5, otr)
    B._bit_identical(out[1], out[0])
    o = out[0]
    assert o["iters"] == nit
    assert [t["accepted"] for t in o["trials"]] == [t["accepted"] for t in otr]
    for a, b in zip(o["trials"], otr):
        assert abs(a["lam"] - b["lam"]) <= 1e-6 * b["lam"] and abs(a["chi"] - b["chi"]) <= 1e-6 * b["chi"]
        if a["early"]:
            assert not exact and not a["accepted"] and not b["accepted"] and b["rho"] < -0.02
        else:
            assert abs(a["chi_new"] - b["chi_new"]) <= 1e-6 * b["chi_new"]
    assert np.allclose(o["pq"][:, :4], oq, atol=1e-6, rtol=0) and np.allclose(o["pq"][:, 4:], ot, atol=1e-5, rtol=0)
    assert np.allclose(o["xyz"], opts, atol=1e-4, rtol=0) and np.allclose(o["sk"], osk, atol=1e-4, rtol=0)


def test_full_size_c2_with_500_nodes_over_4_ranks():
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    g = np.load(os.path.join(here, "golden", "dba_C2_embedded500_trace.npz"))
    p = S.make_dba_problem("C2")
    flag, nb = S.embedded_problem(p, int(g["n_nodes"]))
    e = nrs.dba_build_edges_embedded(p["kf_points"], flag, nb)
    assert int(g["edge_checksum"]) == S.edge_checksum(e)
    w = S.embedded_window(p, e)
    cam = nrs.make_camera(p["model"], p["prm"])
    qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
    out = _run(4, p, e, w, cam, qt, exact=1)
    for o in out[1:]:
        B._bit_identical(o, out[0])
    o = out[0]
    t = o["trials"]
    assert o["kft"] is True and _inner(t) <= 3 * len(t)
    assert o["iters"] == int(g["out_iters"])
    assert [x["accepted"] for x in t] == g["out_accepted"].tolist()
    for x, chi, chi_new, lam in zip(t, g["out_chi"], g["out_chi_new"], g["out_lam"]):
        assert abs(x["lam"] - lam) <= 1e-6 * lam and abs(x["chi"] - chi) <= 1e-6 * chi
        if not x["early"]:
            assert abs(x["chi_new"] - chi_new) <= 1e-6 * chi_new
    pq, xyz, sk = o["pq"], o["xyz"], o["sk"]
    assert np.allclose(pq[:, :4], g["out_q"], atol=1e-6, rtol=0) and np.allclose(pq[:, 4:], g["out_t"], atol=1e-5, rtol=0)
    assert np.allclose(xyz[g["sel"]], g["out_pts_sel"], atol=1e-4, rtol=0) and np.allclose(sk[g["ssel"]], g["out_sk_sel"], atol=1e-4, rtol=0)
    # memory: a rank holds its own blocks and the two Schur-update operands (what was carved), and its whole buffer -- lists included --
    # scales with its share of the keyframes
    c = nrs.Context(embedded_solver=1)
    c.dba_upload_embedded(cam, qt, w, e, p["scale"])
    whole = dict(c.debug_kft_share(), mib=c.debug_kft_info()["mib"])
    c.close()
    K = whole["nk"]
    assert whole["mib"] * 1024 >= whole["kib"] >= 8 * K * 1408 * 1408 / 1024
    for o in out:
        nk = o["share"]["nk"]
        assert 8 * nk * 1408 * 1408 / 1024 <= o["share"]["kib"] <= (nk + 2) / (K + 2) * whole["kib"] + 1
        assert o["share"]["mib"] <= (nk + 2) / K * whole["mib"] + 16


def test_reset_is_reproducible_and_rccl_world_1():
    p, e, w, cam, qt = B._setup(500, 5, 70, 56)
    ref = _unsharded_kft(p, e, w, cam, qt)
    out = _run(2, p, e, w, cam, qt, resets=3)
    for o in out:
        B._close(o, ref)
        for trials, pq, xyz, sk in o["runs"]:
            assert B._key(trials) == B._key(o["trials"])
            assert np.array_equal(pq, o["pq"]) and np.array_equal(xyz, o["xyz"]) and np.array_equal(sk, o["sk"])
    c = nrs.Context(embedded_solver=1, sharded_kft=1)
    c.comm_init_rccl(1, 0, nrs.comm_unique_id())
    c.dba_upload_embedded(cam, qt, w, e, p["scale"])
    assert c.debug_kft_info()["on"] is True
    tr = nrs.Trace()
    c.dba_optimize(5, tr)
    pq, xyz = c.dba_download()
    o = dict(trials=tr.trials, pq=pq, xyz=xyz, sk=c.dba_download_skinned())
    c.close()
    assert _inner(o["trials"]) <= 3 * len(o["trials"])
    B._close(o, ref)


def test_pcg_choice_on_a_communicator_is_unchanged():
    p, e, w, cam, qt = B._setup(400, 5, 60, 55)
    a = _run(2, p, e, w, cam, qt, solver=2, sharded_kft=1)
    b = _run(2, p, e, w, cam, qt, solver=1, sharded_kft=0)
    for x, y in zip(a, b):
        assert x["kft"] is False and y["kft"] is False
        B._bit_identical(x, y)


def test_blocks_beyond_the_lds_fall_back_to_pcg():
    """forced mode, two keyframes of more than 1710 node copies (ld > 5120: the rows k_kft_tgt stages would not fit the LDS): block-Jacobi PCG"""
    p, e, w, cam, qt = B._setup(6000, 2, 2400, 59)
    assert np.bincount(w["lm_kf"]).min() > 1710
    res = {}
    for solver in (1, 2):
        c = nrs.Context(embedded_solver=solver)
        c.dba_upload_embedded(cam, qt, w, e, p["scale"])
        assert c.debug_kft_info()["on"] is False
        tr = nrs.Trace()
        c.dba_optimize(2, tr)
        pq, xyz = c.dba_download()
        res[solver] = dict(trials=tr.trials, pq=pq, xyz=xyz, sk=c.dba_download_skinned())
        c.close()
    B._bit_identical(res[1], res[2])
    out = _run(2, p, e, w, cam, qt, solver=1, iters=2)
    ref = _run(2, p, e, w, cam, qt, solver=2, iters=2)
    for o, r in zip(out, ref):
        assert o["kft"] is False
        B._bit_identical(o, r)


def _rank_codes(world, fn, timeout=180):
    """fn(rank, group) -> error code (0: success) on `world` thread ranks; a rank that does not finish in time is a hang"""
    group = nrs.LocalGroup(world)
    codes = [None] * world

    def main(r):
        codes[r] = fn(r, group)

    th = [threading.Thread(target=main, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout)
    assert all(not t.is_alive() for t in th), "a rank hangs"
    group.close()
    return codes


def test_a_rank_local_setup_failure_fails_every_rank():
    """a skinned observation reaching a node copy of another keyframe is rejected by the rank that holds it, before the factorisation's
    set-up: with sharded_kft = 1 every rank still returns an error, and none waits for a peer"""
    p, e, w, cam, qt = B._setup(300, 4, 40, 53)
    bad = dict(e, sk_node=e["sk_node"].copy())
    bad["sk_node"][0, 0] = np.where(w["lm_kf"] != w["sk_kf"][0])[0][0]

    def fn(r, group):
        c = nrs.Context(embedded_solver=1, sharded_kft=1)
        c.comm_init_local(group, r)
        try:
            c.dba_upload_embedded(cam, qt, w, bad, p["scale"])
            rc = 0
        except nrs.NrsError as ex:
            rc = ex.code
        c.close()
        return rc
    codes = _rank_codes(2, fn)
    owner = 0 if w["sk_kf"][0] < nrs.shard_plan(4, w["lm_kf"], 2)[1] else 1
    assert codes[owner] == -1 and codes[1 - owner] not in (None, 0)


def test_a_damper_across_two_keyframes_inside_one_rank_means_pcg_everywhere():
    """a damper joining keyframes k and k + 2 of one rank's range (6 keyframes over 2 ranks): on one GPU the factorisation does
    not apply (not block tridiagonal); sharded, every rank takes the same decision -- block-Jacobi PCG on both, no rank out of step"""
    p, e, w, cam, qt = B._setup(600, 6, 80, 54)
    kb = nrs.shard_plan(6, w["lm_kf"], 2)
    r = int(np.argmax(np.diff(kb)))
    assert kb[r + 1] - kb[r] >= 3
    k0 = int(kb[r])                                                    # keyframes k0 and k0 + 2 of one rank
    dm = e["dm_idx"].copy()
    q = int(np.where((dm[:, 0] >= 0) & (dm[:, 2] >= 0) & (dm[:, 3] >= 0) & (w["lm_kf"][np.maximum(dm[:, 0], 0)] == k0))[0][0])
    k2 = np.where(w["lm_kf"] == k0 + 2)[0]
    dm[q, 2], dm[q, 3] = k2[0], k2[1]
    e2 = dict(e, dm_idx=dm)
    c = nrs.Context(embedded_solver=1)
    c.dba_upload_embedded(cam, qt, w, e2, p["scale"])
    assert c.debug_kft_info()["on"] is False
    tr = nrs.Trace()
    c.dba_optimize(5, tr)
    pq, xyz = c.dba_download()
    ref = (tr.trials, pq, xyz, c.dba_download_skinned())
    c.close()
    out = _run(2, p, e2, w, cam, qt)
    for o in out:
        assert o["kft"] is False
        B._close(o, ref)
    B._bit_identical(out[1], out[0])
