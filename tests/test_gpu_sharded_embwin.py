"""GPU: nrs_dba_solve_window_embedded on a communicator under NRS_SHARD_EMBWIN_DEVICE=1 -- every rank builds its share of the embedded
window's lists on its own device (csrc/nrs_engine_embwin.hpp), hands a SLICED skinned list to the set-up and evaluates its skinned points
on the device.  (Without the switch a communicator keeps the host builder: tests/test_gpu_embedded_window.py.)

The ranks are threads of this process (nrs.LocalGroup), the windows those of tests/embedded_window_cases.py in a shape of their own:
300 points x 8 keyframes x 40 nodes over 2, 3 and 4 ranks, and 300 x 4 x 40 over 4 ranks, where a rank owns a single keyframe.  Held to
  lists    the host builder index for index and bit for bit: node copies, springs, dampers and sk_obs whole, sk_node / sk_omega as the
           rows [sk_base, sk_base + sk_held) of the host lists; the slices tile the window's list; [k0, k1) is nrs.shard_plan
  solve    every rank the same bits; the same bits as NRS_HOST_PACK=1 on the same group (trace included); the unsharded one call at
           the tolerances of tests/test_gpu_sharded_embedded.py test_sharded_matches_unsharded
  memory   the staging of a rank's skinned arrays: at most its own count's bytes plus the layout's padding (embwin_layout: every array
           rounded up to 256 bytes, then 256 more)
  edges    a rank without a skinned observation, observations bound to nothing, walks cut short by BAD, a node listed twice."""
import threading

import numpy as np
import pytest

import embedded_window_cases as W
import nrs
import nrs_synth as S
from test_gpu_sharded_embedded import _close as sharded_close         # the tolerances of sharded against unsharded
from test_gpu_sharded_embedded import _key as full_key

pytestmark = pytest.mark.gpu

CASE8 = (300, 8, 40, 61, S.PINHOLE, {})
CASE4 = (300, 4, 40, 53, S.PINHOLE, {})                              # over 4 ranks: one keyframe each
WHOLE = ("lm_obs", "sp_ij", "sp_d0", "dm_idx", "dm_w", "sk_obs")
PAD = 255 + 256                                                      # embwin_layout, per array
_host = {}


def _setup(case, form):
    p, flag, nb = W.window(case, form)
    key = (case[:4], form)
    if key not in _host:
        _host[key] = nrs.dba_build_edges_embedded(p["kf_points"], flag, nb)
    win = dict(kf_points=p["kf_points"], xyz=p["lm_xyz"], uv=p["lm_uv"], flag=flag, nb=nb, scale=p["scale"],
               cam=nrs.make_camera(p["model"], p["prm"]), qt=np.concatenate([p["poses_q"], p["poses_t"]], 1))
    return p, win, _host[key]


def _obs_kf(kf_points):
    return np.concatenate([np.full(len(x), k, np.int32) for k, x in enumerate(kf_points)])


def _solve(c, win, iters):
    tr = nrs.Trace()
    pq, xyz = c.dba_solve_window_embedded(win["cam"], win["qt"], win["kf_points"], win["xyz"], win["uv"], win["flag"], win["nb"], win["scale"], iters, tr)
    return pq, xyz, tr.trials


def _run_group(world, win, iters=5, host_ranks=()):
    """every rank: the one call, then the taps.  Returns per rank a dict, or dict(code, msg) when the call was refused; every
    context asks for the rank-local device builder (NRS_SHARD_EMBWIN_DEVICE), a rank of host_ranks builds on the host all the same
    (NRS_HOST_PACK on its own context)"""
    group = nrs.LocalGroup(world)
    out, errs = [None] * world, []

    def rank_main(r):
        c = None
        try:
            c = nrs.Context()
            c.comm_init_local(group, r)
            c.debug_set("NRS_SHARD_EMBWIN_DEVICE", "1")
            if r in host_ranks:
                c.debug_set("NRS_HOST_PACK", "1")
            try:
                pq, xyz, trials = _solve(c, win, iters)
            except nrs.NrsError as ex:
                out[r] = dict(code=ex.code, msg=str(ex))
                return
            out[r] = dict(pq=pq, xyz=xyz, trials=trials, lists=c.dba_window_edges_embedded(), slice=c.dba_window_slice_embedded(), skin=c.dba_skin_stats(),
                          sk64=c.dba_download_skinned())
        except Exception as ex:                      # a failed rank would leave the others in the barrier
            errs.append((r, ex))
            raise
        finally:
            if c is not None:
                c.close()

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert not any(t.is_alive() for t in th), "a rank did not end"
    assert not errs, errs
    group.close()
    return out


def _check_lists(out, host, kf_points, world):
    obs_kf = _obs_kf(kf_points)
    n_skin, n_lm, n_sp, n_dm = len(host["sk_obs"]), len(host["lm_obs"]), len(host["sp_ij"]), len(host["dm_idx"])
    kb = nrs.shard_plan(len(kf_points), obs_kf[host["lm_obs"]], world)
    sk_kf = obs_kf[host["sk_obs"]]
    at = 0
    for r, o in enumerate(out):
        got, sl = o["lists"], o["slice"]
        assert got["on_device"] == 1
        for key in WHOLE:
            assert got[key].dtype == host[key].dtype and np.array_equal(got[key], host[key]), key
        assert (sl["k0"], sl["k1"]) == (kb[r], kb[r + 1])
        base, held = sl["sk_base"], sl["sk_held"]
        assert base == at and held == ((sk_kf >= kb[r]) & (sk_kf < kb[r + 1])).sum()      # no gap, no overlap; the rank's keyframes
        at += held
        assert (got["sk_base"], got["sk_held"]) == (base, held)
        assert got["sk_node"].shape == (held, 11) and np.array_equal(got["sk_node"], host["sk_node"][base:base + held])
        assert got["sk_omega"].dtype == np.float64 and np.array_equal(got["sk_omega"], host["sk_omega"][base:base + held])
        assert o["skin"][0] == held
        # memory: 88 + 44 + 12 + 8 + 4 bytes per OWN skinned observation in five arrays; the whole blob adds sk_obs and the node side
        assert sl["sk_stage_bytes"] <= 156 * held + 5 * PAD
        assert sl["stage_bytes"] <= 156 * held + 4 * n_skin + 28 * n_lm + 12 * n_sp + 20 * n_dm + 14 * PAD
    assert at == n_skin


def _same_bits(a, b):
    assert len(a["trials"]) > 0 and full_key(a["trials"]) == full_key(b["trials"])
    assert np.array_equal(a["pq"], b["pq"]) and np.array_equal(a["xyz"], b["xyz"]) and np.array_equal(a["sk64"], b["sk64"])


@pytest.mark.parametrize("form", W.FORMS)
@pytest.mark.parametrize("world", [2, 3, 4])
def test_lists_rank_by_rank(world, form):
    p, win, host = _setup(CASE8, form)
    W.check_not_vacuous(CASE8, form, p, win["flag"], win["nb"], host)        # full: observations bound to nothing, walks cut short by BAD
    _check_lists(_run_group(world, win, iters=1), host, win["kf_points"], world)


def test_lists_one_keyframe_per_rank():
    p, win, host = _setup(CASE4, "full")
    out = _run_group(4, win, iters=1)
    assert [(o["slice"]["k0"], o["slice"]["k1"]) for o in out] == [(0, 1), (1, 2), (2, 3), (3, 4)]
    _check_lists(out, host, win["kf_points"], 4)


@pytest.mark.parametrize("case,world", [(CASE8, 2), (CASE8, 3), (CASE8, 4), (CASE4, 4)], ids=["8kf-2", "8kf-3", "8kf-4", "4kf-4"])
def test_solve(case, world):
    p, win, host = _setup(case, "full")
    dev = _run_group(world, win)
    for o in dev:
        assert o["lists"]["on_device"] == 1
        _same_bits(o, dev[0])                                        # every rank the same complete result
    nrs.debug_set("NRS_HOST_PACK", "1")
    try:
        hst = _run_group(world, win)
    finally:
        nrs.debug_set("NRS_HOST_PACK", None)
    for o in hst:
        assert o["lists"]["on_device"] == 0 and o["slice"]["sk_held"] == len(host["sk_obs"])
        _same_bits(o, dev[0])                                        # the LM trace equal trial by trial, poses and obs_xyz to the last bit
    ref = nrs.Context(embedded_solver=2)                             # a communicator: the block-Jacobi PCG
    try:
        pq, xyz, trials = _solve(ref, win, 5)
    finally:
        ref.close()
    lm, sk = host["lm_obs"], host["sk_obs"]
    for o in dev:
        sharded_close(dict(trials=o["trials"], pq=o["pq"], xyz=o["xyz"][lm], sk=o["xyz"][sk]), (trials, pq, xyz[lm].astype(np.float64), xyz[sk].astype(np.float64)))
        assert np.array_equal(o["sk64"].astype(np.float32), o["xyz"][sk])
        rest = np.ones(len(xyz), bool)
        rest[lm] = False
        rest[sk] = False
        assert rest.any() and np.array_equal(o["xyz"][rest], win["xyz"][rest])         # observations bound to nothing: unchanged


def test_a_rank_that_does_not_qualify_builds_on_the_host_alone():
    p, win, host = _setup(CASE8, "full")
    dev = _run_group(3, win)
    mix = _run_group(3, win, host_ranks=(1,))
    assert [o["lists"]["on_device"] for o in mix] == [1, 0, 1]
    assert mix[1]["slice"]["sk_held"] == len(host["sk_obs"]) and mix[0]["slice"]["sk_held"] == dev[0]["slice"]["sk_held"]
    for o in mix:
        _same_bits(o, dev[0])


def _without_skinned_in(win, host, k):
    """the window with the observations of keyframe k that are not node copies taken out"""
    obs_kf = _obs_kf(win["kf_points"])
    keep = (obs_kf != k) | (np.asarray(win["flag"])[np.concatenate(win["kf_points"])] != 0)
    kf = [np.asarray(x)[keep[obs_kf == i]] for i, x in enumerate(win["kf_points"])]
    return dict(win, kf_points=kf, xyz=win["xyz"][keep], uv=win["uv"][keep])


def test_a_rank_whose_keyframes_carry_no_skinned_observation():
    p, win, _ = _setup(CASE4, "full")
    win = _without_skinned_in(win, None, 2)
    host = nrs.dba_build_edges_embedded(win["kf_points"], win["flag"], win["nb"])
    assert not (_obs_kf(win["kf_points"])[host["sk_obs"]] == 2).any() and len(host["sk_obs"]) > 0
    dev = _run_group(4, win)
    _check_lists(dev, host, win["kf_points"], 4)
    assert dev[2]["slice"]["sk_held"] == 0 and (dev[2]["slice"]["k0"], dev[2]["slice"]["k1"]) == (2, 3)
    nrs.debug_set("NRS_HOST_PACK", "1")
    try:
        hst = _run_group(4, win)
    finally:
        nrs.debug_set("NRS_HOST_PACK", None)
    for o in dev + hst:
        _same_bits(o, dev[0])


def test_a_node_listed_twice_is_refused_on_every_rank():
    p, win, host = _setup(CASE8, "full")
    kf = [np.array(x) for x in win["kf_points"]]
    node_here = kf[5][np.asarray(win["flag"])[kf[5]] != 0]
    assert len(node_here) >= 2
    kf[5][np.where(kf[5] == node_here[1])[0][0]] = node_here[0]
    for host_ranks in ((), (0, 1, 2)):                               # the device's refusal and the host builder's: the same text
        out = _run_group(3, dict(win, kf_points=kf), iters=1, host_ranks=host_ranks)          # (_run_group asserts that every thread ended)
        for o in out:
            assert o["code"] == -1 and "a map point is listed twice in one keyframe" in o["msg"]
    _check_lists(_run_group(3, win, iters=1), host, win["kf_points"], 3)                      # the group is usable afterwards
