"""GPU: the embedded BA window in ONE call (include/nrs.h nrs_dba_solve_window_embedded): the lists of nrs_dba_build_edges_embedded built
on the device (csrc/nrs_engine_embwin.hpp), then the set-up and the solve of nrs_dba_solve_embedded.

Held to the host builder index for index and bit for bit (the fp64 skinning weights included), to oracle/embedded_oracle.py
dba_build_embedded, to the three-step path (host build, gather, nrs_dba_solve_embedded) to the last bit of the solve, and with every
point a node to nrs_dba_solve_window.  The windows (tests/embedded_window_cases.py) come in two neighbour forms: the node-only lists,
and the full graph with the same flags and ~3 % BAD connections."""
import threading

import numpy as np
import pytest

import embedded_oracle as E
import embedded_window_cases as W
import nrs
import nrs_synth as S
from test_gpu_sharded_embedded import _close as sharded_close         # the tolerances of sharded against unsharded

pytestmark = pytest.mark.gpu

LISTS = ("lm_obs", "sp_ij", "sp_d0", "dm_idx", "dm_w", "sk_obs", "sk_node", "sk_omega")
_host = {}


def _setup(case, form):
    """window, node flags, neighbour lists, camera, poses and the HOST lists (computed once per window, shared, left unchanged)"""
    p, flag, nb = W.window(case, form)
    key = (case[:4], form)
    if key not in _host:
        _host[key] = nrs.dba_build_edges_embedded(p["kf_points"], flag, nb)
    cam = nrs.make_camera(p["model"], p["prm"])
    qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
    return p, flag, nb, cam, qt, _host[key]


def _key(trials):
    return [(t["accepted"], t["lam"], t["chi"], t["chi_new"]) for t in trials]


def _one_call(c, p, flag, nb, cam, qt, iters=5):
    tr = nrs.Trace()
    pq, xyz = c.dba_solve_window_embedded(cam, qt, p["kf_points"], p["lm_xyz"], p["lm_uv"], flag, nb, p["scale"], iters, tr)
    return pq, xyz, tr.trials


def _three_steps(c, p, flag, nb, cam, qt, iters=5):
    e = nrs.dba_build_edges_embedded(p["kf_points"], flag, nb)
    w = S.embedded_window(p, e)
    tr = nrs.Trace()
    pq, lm, sk = c.dba_solve_embedded(cam, qt, w, e, p["scale"], iters, tr)
    return pq, lm, sk, tr.trials, e


def _same_solve(p, one, three):
    """poses, trials and every row of obs_xyz: node copies, skinned observations, the rest unchanged"""
    pq, xyz, trials = one
    pq3, lm3, sk3, trials3, e = three
    assert len(trials) > 0 and _key(trials) == _key(trials3)
    assert np.array_equal(pq, pq3)
    assert np.array_equal(xyz[e["lm_obs"]], lm3) and np.array_equal(xyz[e["sk_obs"]], sk3)
    rest = np.ones(len(xyz), bool)
    rest[e["lm_obs"]] = False
    rest[e["sk_obs"]] = False
    assert np.array_equal(xyz[rest], p["lm_xyz"][rest])
    assert not np.array_equal(xyz[e["lm_obs"]], p["lm_xyz"][e["lm_obs"]])      # (the solve moved something)
    return rest.sum()


@pytest.mark.parametrize("form", W.FORMS)
@pytest.mark.parametrize("case", W.CASES, ids=lambda c: "%dx%dx%d" % c[:3])
def test_lists_index_for_index(ctx, case, form):
    p, flag, nb, cam, qt, host = _setup(case, form)
    W.check_not_vacuous(case, form, p, flag, nb, host)               # on the HOST lists, before the comparison
    _one_call(ctx, p, flag, nb, cam, qt, iters=1)
    dev = ctx.dba_window_edges_embedded()
    assert dev["on_device"] == 1
    for key in LISTS:
        assert dev[key].dtype == host[key].dtype and np.array_equal(dev[key], host[key]), key
    if case is W.CASES[0]:                                           # ... and the oracle's statement of the lists (tests/test_host_cpu.py)
        ora = E.dba_build_embedded(p["kf_points"], flag, nb["rowptr"], nb["col"], nb["w"], nb["d0"], nb["status"])
        for key in LISTS:
            assert np.array_equal(dev[key], ora[key]), key


@pytest.mark.parametrize("solver", [0, 2], ids=["factorisation", "pcg"])
@pytest.mark.parametrize("form", W.FORMS)
def test_same_solve_to_the_last_bit(solver, form):
    """the one call against host build + gather + nrs_dba_solve_embedded, each on a fresh context with the same options: the
    keyframe-block factorisation (the default of these sizes, as the fixture ctx) and the block-Jacobi PCG (as ctx_emb_pcg)"""
    p, flag, nb, cam, qt, host = _setup(W.CASES[1], form)
    a, b = nrs.Context(embedded_solver=solver), nrs.Context(embedded_solver=solver)
    try:
        one = _one_call(a, p, flag, nb, cam, qt)
        assert a.debug_kft_info()["on"] is (solver == 0)
        assert a.dba_window_edges_embedded()["on_device"] == 1
        three = _three_steps(b, p, flag, nb, cam, qt)
        unbound = _same_solve(p, one, three)
        assert (unbound > 0) == (form == "full")
    finally:
        a.close()
        b.close()


def test_every_point_a_node_is_the_plain_window(ctx):
    p, flag, nb, cam, qt, _ = _setup(W.CASES[0], "nodes")
    tr = nrs.Trace()
    pq0, xyz0 = ctx.dba_solve_window(cam, qt, p["kf_points"], p["lm_xyz"], p["lm_uv"], p["nbr"], p["scale"], 5, tr)
    pq, xyz, trials = _one_call(ctx, p, np.ones(p["n_points"], np.uint8), p["nbr"], cam, qt)
    e = ctx.dba_window_edges_embedded()
    assert e["on_device"] == 1 and len(e["sk_obs"]) == 0 and np.array_equal(e["lm_obs"], np.arange(len(p["lm_xyz"])))
    assert len(trials) > 0 and _key(trials) == _key(tr.trials)
    assert np.array_equal(pq, pq0) and np.array_equal(xyz, xyz0)


def test_host_pack_switch_takes_the_host_construction():
    p, flag, nb, cam, qt, host = _setup(W.CASES[1], "full")
    a, b = nrs.Context(), nrs.Context()
    try:
        nrs.debug_set("NRS_HOST_PACK", "1")
        one = _one_call(a, p, flag, nb, cam, qt)
        got = a.dba_window_edges_embedded()
        nrs.debug_set("NRS_HOST_PACK", None)
        assert got["on_device"] == 0
        for key in LISTS:
            assert np.array_equal(got[key], host[key]), key
        _same_solve(p, one, _three_steps(b, p, flag, nb, cam, qt))
    finally:
        nrs.debug_set("NRS_HOST_PACK", None)
        a.close()
        b.close()


def _is_state_error(c):
    with pytest.raises(nrs.NrsError) as ei:
        c.dba_window_edges_embedded()
    return ei.value.code == -5


def test_errors_leave_nothing_resident(ctx):
    p, flag, nb, cam, qt, host = _setup(W.CASES[0], "nodes")

    def refused(kf_points, flag_, nb_):
        _one_call(ctx, p, flag, nb, cam, qt, iters=1)                # a window is resident ...
        assert ctx.dba_window_edges_embedded()["on_device"] == 1
        with pytest.raises(nrs.NrsError) as ei:
            ctx.dba_solve_window_embedded(cam, qt, kf_points, p["lm_xyz"], p["lm_uv"], flag_, nb_, p["scale"], 1)
        assert ei.value.code == -1                                   # NRS_ERR_INVALID
        assert _is_state_error(ctx)                                  # ... and is gone after the refused call
        with pytest.raises(nrs.NrsError):
            ctx.dba_reset()

    # a map point (a node) listed twice in one keyframe: the same number of observations, the keyframe's second entry replaced
    kf = [np.array(x) for x in p["kf_points"]]
    node_here = kf[1][flag[kf[1]] != 0]
    assert len(node_here) >= 2
    kf[1][np.where(kf[1] == node_here[1])[0][0]] = node_here[0]
    refused(kf, flag, nb)
    refused(p["kf_points"], None, nb)                                # is_node null
    bad = dict(nb, col=nb["col"].copy())
    bad["col"][len(bad["col"]) // 2] = p["n_points"]                 # a neighbour index out of range
    refused(p["kf_points"], flag, bad)
    # a window made by nrs_dba_upload_embedded is not the one call's
    _one_call(ctx, p, flag, nb, cam, qt, iters=1)
    ctx.dba_upload_embedded(cam, qt, S.embedded_window(p, host), host, p["scale"])
    assert _is_state_error(ctx)


def test_a_communicator_takes_the_host_construction():
    """two thread ranks of a local group: the one call on every rank builds its lists on the host and returns the unsharded block-Jacobi
    PCG solve, to the tolerances of tests/test_gpu_sharded_embedded.py"""
    p, flag, nb, cam, qt, host = _setup(W.CASES[0], "nodes")
    ref_ctx = nrs.Context(embedded_solver=2)
    pq, lm, sk, trials, e = _three_steps(ref_ctx, p, flag, nb, cam, qt)
    ref_ctx.close()
    world = 2
    group = nrs.LocalGroup(world)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            c = nrs.Context()
            c.comm_init_local(group, r)
            q, xyz, tr = _one_call(c, p, flag, nb, cam, qt)
            got = c.dba_window_edges_embedded()
            out[r] = dict(trials=tr, pq=q, xyz=xyz[e["lm_obs"]], sk=xyz[e["sk_obs"]], on_device=got["on_device"],
                          same=all(np.array_equal(got[key], host[key]) for key in LISTS))
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
    for o in out:
        assert o["on_device"] == 0 and o["same"]
        sharded_close(o, (trials, pq, lm.astype(np.float64), sk.astype(np.float64)))
    assert _key(out[0]["trials"]) == _key(out[1]["trials"]) and np.array_equal(out[0]["pq"], out[1]["pq"]) and np.array_equal(out[0]["xyz"], out[1]["xyz"])


def test_the_window_stays_resident(ctx):
    p, flag, nb, cam, qt, host = _setup(W.CASES[2], "full")
    pq, xyz, trials = _one_call(ctx, p, flag, nb, cam, qt)
    sk = ctx.dba_download_skinned()
    assert sk.shape == (len(host["sk_obs"]), 3) and np.array_equal(sk.astype(np.float32), xyz[host["sk_obs"]])
    ctx.dba_reset()
    tr = nrs.Trace()
    ctx.dba_optimize(5, tr)
    assert len(trials) > 0 and _key(tr.trials) == _key(trials)
    pq2, lm2 = ctx.dba_download()
    assert np.array_equal(pq2, pq) and np.array_equal(lm2.astype(np.float32), xyz[host["lm_obs"]])
    assert np.array_equal(ctx.dba_download_skinned(), sk)
    assert ctx.debug_kft_info()["on"] is True
