"""GPU: speculative LM trials of BA windows on the two-kernel PCG (nrs_engine_types.hpp SpecSet, nrs_engine.hip PcgSetView).

A run of rejected trials goes out as a batch on shadow sets; the host takes the results in order.  The same trials with the same
arithmetic: every trial record, the solution and the iteration count are held bit for bit to one trial at a time (NRS_SPEC_TRIALS=0).
"""
import numpy as np
import pytest

import nrs
import nrs_synth as S

pytestmark = pytest.mark.gpu

KEYS = ("accepted", "inner", "lam", "chi", "chi_new", "early")


def _window(n_points, n_kf, seed, model=S.PINHOLE):
    p = S.make_dba_problem(n_points, n_kf, seed, model)
    e = nrs.dba_build_edges(p["kf_points"], p["nbr"])
    cam = nrs.make_camera(p["model"], p["prm"])
    qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
    return p, e, cam, qt


def _solve(win, spec, steps=2, **opts):
    p, e, cam, qt = win
    ctx = nrs.Context(**opts)
    if spec is not None:
        ctx.debug_set("NRS_SPEC_TRIALS", str(spec))
    ctx.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"])
    runs = []
    for _ in range(steps):                                        # (dba_reset + optimize(5): the benchmark's step, twice -- the second batch is sized by the first run)
        ctx.dba_reset()
        tr = nrs.Trace()
        ctx.dba_optimize(5, tr)
        pq, xyz = ctx.dba_download()
        runs.append(([{k: t[k] for k in KEYS} for t in tr.trials], tr.iterations, pq.copy(), xyz.copy()))
    stats = ctx.dba_stats()
    ctx.close()
    return runs, stats


def _assert_same(a, b):
    assert len(a) == len(b)
    for (ta, ia, pa, xa), (tb, ib, pb, xb) in zip(a, b):
        assert ta == tb, "trial records differ"
        assert ia == ib
        assert np.array_equal(pa, pb), "poses differ"
        assert np.array_equal(xa, xb), "map points differ"


@pytest.mark.parametrize("exact", [0, 1])
def test_c2_bench_window_same_bits(exact):
    n, k, seed, model = S.CONFIGS["C2"]
    win = _window(n, k, seed, model)
    spec, st_spec = _solve(win, None, exact_trials=exact)
    one, st_one = _solve(win, 0, exact_trials=exact)
    _assert_same(spec, one)
    assert st_spec["device_bytes"] > st_one["device_bytes"], "the C2 window carves shadow sets"
    trials = spec[-1][0]
    assert not trials[0]["accepted"], "the benchmark window starts with a run of rejected trials (what the sets are for)"


@pytest.mark.parametrize("n_kf", [5, 10])
def test_small_plain_window_same_bits(n_kf):
    win = _window(5000, n_kf, 7)                                  # (5 keyframes: the single-launch PCG, which carves no sets; 10: the two-kernel PCG)
    spec, _ = _solve(win, None)
    one, _ = _solve(win, 0)
    _assert_same(spec, one)


@pytest.mark.parametrize("sets", [1, 3])
def test_other_set_counts_same_bits(sets):
    n, k, seed, model = S.CONFIGS["C2"]
    win = _window(n, k, seed, model)
    a, _ = _solve(win, sets, steps=1)
    b, _ = _solve(win, 0, steps=1)
    _assert_same(a, b)


@pytest.mark.parametrize("followers", [0, 1, 2])
def test_first_trial_followers_same_bits(followers):
    """NRS_SPEC_FIRST: the first trial of an iteration with followers (default: as many as there are sets).  A follower whose first
    PCG batch the host does not confirm is solved again -- the records stay the same either way"""
    n, k, seed, model = S.CONFIGS["C2"]
    win = _window(n, k, seed, model)
    p, e, cam, qt = win
    ctx = nrs.Context()
    ctx.debug_set("NRS_SPEC_FIRST", str(followers))
    ctx.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"])
    runs = []
    for _ in range(3):
        ctx.dba_reset()
        tr = nrs.Trace()
        ctx.dba_optimize(5, tr)
        pq, xyz = ctx.dba_download()
        runs.append(([{k: t[k] for k in KEYS} for t in tr.trials], tr.iterations, pq.copy(), xyz.copy()))
    ctx.close()
    one, _ = _solve(win, 0, steps=3)
    _assert_same(runs, one)


def test_c3_size_carves_no_sets():
    n, k, seed, model = S.CONFIGS["C3"]
    p, e, cam, qt = _window(n, k, seed, model)
    got = []
    for spec in (None, 0):
        ctx = nrs.Context()
        if spec is not None:
            ctx.debug_set("NRS_SPEC_TRIALS", str(spec))
        ctx.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"])
        got.append(ctx.dba_stats()["device_bytes"])
        ctx.close()
    assert got[0] == got[1]


def test_profiling_context_carves_no_sets():
    win = _window(5000, 10, 7)
    p, e, cam, qt = win
    got = []
    for spec in (None, 0):
        ctx = nrs.Context(profile=1)
        if spec is not None:
            ctx.debug_set("NRS_SPEC_TRIALS", str(spec))
        ctx.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"])
        got.append(ctx.dba_stats()["device_bytes"])
        ctx.close()
    assert got[0] == got[1]


def test_row_limit_carves_no_sets():
    win = _window(5000, 10, 7)
    a, st_a = _solve(win, None)
    p, e, cam, qt = win
    ctx = nrs.Context()
    ctx.debug_set("NRS_SPEC_MAX_ROWS", "1000")
    ctx.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"])
    st_b = ctx.dba_stats()
    ctx.close()
    _, st_one = _solve(win, 0, steps=1)
    assert st_b["device_bytes"] == st_one["device_bytes"] < st_a["device_bytes"]
