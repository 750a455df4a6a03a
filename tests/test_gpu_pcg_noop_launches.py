"""GPU: plain BA windows on the two-kernel PCG without the fills and launches that do no work (nrs_engine.hip pcg_begin, pcg_advance,
TrialBatch::join; nrs_engine_linearize.hpp k_finalize / publish_flags).

The evaluation that publishes a set's status words leaves them cleared for the next solve, one fill discards the speculative trials of
all shadow sets, and a solve that runs past the last one's iteration count goes on two iterations at a time.  None of it touches the
arithmetic: every trial record and the downloaded state are held bit for bit to one trial at a time, to a fill per trial
(NRS_NO_REARM) and to themselves over repeated runs on one context.

The window: 3400 points x 10 keyframes = 34 000 landmark rows before padding, the smallest round size above the 32 768-row floor
of the two-kernel path (below it d.fused: one launch per iteration, no shadow sets) and far below the NRS_SPEC_MAX_ROWS ceiling
(2^18).  That it carves shadow sets is asserted through the device bytes.
"""
import functools

import numpy as np
import pytest

import nrs
import nrs_synth as S

pytestmark = pytest.mark.gpu

KEYS = ("lam", "chi", "chi_new", "rho", "accepted", "early", "inner", "ok")
N_POINTS, N_KF, SEED = 3400, 10, 7


@functools.lru_cache(maxsize=None)
def _window():
    p = S.make_dba_problem(N_POINTS, N_KF, SEED)
    e = nrs.dba_build_edges(p["kf_points"], p["nbr"])
    cam = nrs.make_camera(p["model"], p["prm"])
    qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
    return p, e, cam, qt


def _upload(ctx, win=None, **repl):
    p, e, cam, qt = win or _window()
    a = dict(qt=qt, xyz=p["lm_xyz"], uv=p["lm_uv"])
    a.update(repl)
    ctx.dba_upload(cam, a["qt"], a["xyz"], p["lm_kf"], a["uv"], e, p["scale"])


def _step(ctx):
    ctx.dba_reset()
    tr = nrs.Trace()
    ctx.dba_optimize(5, tr)
    pq, xyz = ctx.dba_download()
    return [{k: t[k] for k in KEYS} for t in tr.trials], tr.iterations, pq.copy(), xyz.copy()


def _run(steps=1, **switches):
    ctx = nrs.Context()
    for k, v in switches.items():
        ctx.debug_set(k, str(v))
    _upload(ctx)
    out = [_step(ctx) for _ in range(steps)]
    stats = ctx.dba_stats()
    ctx.close()
    return out, stats


@functools.lru_cache(maxsize=None)
def _default3():
    """reset + optimize(5) three times on a fresh context, default path: the reference every test below compares with (read-only)"""
    return _run(3)


def _same(a, b):
    ta, ia, pa, xa = a
    tb, ib, pb, xb = b
    assert ta == tb, "trial records differ"
    assert ia == ib
    assert np.array_equal(pa, pb), "poses differ"
    assert np.array_equal(xa, xb), "map points differ"


def test_window_takes_the_two_kernel_path_with_shadow_sets():
    (_, st) = _default3()
    (_, st0) = _run(1, NRS_SPEC_TRIALS=0)
    assert st["device_bytes"] > st0["device_bytes"], "the window carves shadow sets (two-kernel PCG)"


@pytest.mark.parametrize("switches", [dict(NRS_SPEC_TRIALS=0), dict(NRS_SPEC_FIRST=0), dict(NRS_NO_REARM=1), dict(NRS_SPEC_TRIALS=0, NRS_NO_REARM=1)],
                         ids=["one_trial_at_a_time", "no_first_followers", "fill_per_trial", "one_at_a_time_fill_per_trial"])
def test_same_trace(switches):
    """every trial of optimize(5) -- lambda, chi2, chi2_new, rho, accepted, early_rejected, inner_iters -- and the downloaded state,
    bit for bit: default path against one trial at a time (no followers, no aborts) and against a fill in front of every trial"""
    ref, _ = _default3()
    got, _ = _run(3, **switches)
    for a, b in zip(got, ref):
        _same(a, b)
    assert len(ref[0][0]) >= 5 and all(t["ok"] for t in ref[0][0])


def test_no_stale_flags_over_repeated_runs():
    """reset + optimize(5) three times on one context: the second and third run give the first run's trace and bits (a status word
    that survived the re-arm -- a peek level, a milestone count, the done word -- would change the looks the host takes or end a
    solve early)"""
    ref, _ = _default3()
    _same(ref[1], ref[0])
    _same(ref[2], ref[0])


def test_failed_solve_does_not_leak_into_the_next():
    """A window with a non-finite observation (the input tests/test_gpu_edge_cases.py uses) fails with NRS_ERR_NUMERIC; the window
    uploaded next on the same context, and a reset + optimize after it, are solved as on a fresh context.  (No input of the existing
    tests raises a trial's flags[2] on a BA window short of this: the non-finite chi2 ends the call before the first trial.)"""
    ref, _ = _default3()
    p = _window()[0]
    uv = p["lm_uv"].copy()
    uv[5, 0] = np.nan
    ctx = nrs.Context()
    _upload(ctx)
    _same(_step(ctx), ref[0])                                      # (status words in use)
    _upload(ctx, uv=uv)
    with pytest.raises(nrs.NrsError, match="NRS_ERR_NUMERIC"):
        ctx.dba_optimize(5, nrs.Trace())
    _upload(ctx)
    _same(_step(ctx), ref[0])
    _same(_step(ctx), ref[0])
    ctx.close()


def test_reset_and_taps_in_between():
    """dba_reset, an optimize of another length and the gradient tap (a linearisation outside optimize, which publishes and clears
    the words) between solves: the next solve starts from cleared words.  (A plain window refuses mask / fixed-flag updates, so no
    such call can come in between on the windows that re-arm.)"""
    ref, _ = _default3()
    ctx = nrs.Context()
    _upload(ctx)
    ctx.dba_optimize(2, nrs.Trace())                               # (ends mid-way: whatever its last trial left)
    _same(_step(ctx), ref[0])
    ctx.dba_reset()
    ctx.dba_gradient()
    ctx.dba_optimize(1, nrs.Trace())
    ctx.dba_gradient()
    _same(_step(ctx), ref[0])
    ctx.dba_reset()
    ctx.dba_reset()
    _same(_step(ctx), ref[0])
    ctx.close()
