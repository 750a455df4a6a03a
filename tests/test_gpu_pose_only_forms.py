"""GPU parity: a1 CameraPoseOptimization (nrs_pose_only_solve) in all THREE kernel forms of csrc/nrs_pose_only.hip against the oracle,
on the cases tests/test_pose_only_cases_cpu.py vets on the CPU (tests/pose_only_cases.py):

  A  one workgroup, points cached in LDS       the default up to 7168 points
  B  one workgroup, points in global memory    the default from 7169 to 32767 points; NRS_PO_NO_CACHE=1 at any size
  C  many workgroups (k_po_pass / k_po_step)   the default from 32768 points; NRS_PO_MULTI_MIN=1 at any size, NRS_PO_MULTI_GROUPS=<g>
                                               caps its grid, so that a few hundred points take several grid-stride trips per thread
                                               and sum several partial-sum slots

Every device-versus-oracle check: q within 1e-6 and t within 1e-5 (pose_only_cases.tolerance), the inlier mask identical outside the
gate band (the CPU test found the band empty on every case, so: identical), conftest.compare_lm_traces over all three rounds, and
trace.iterations and the trial count equal to the oracle's where the traces are compared to their end."""
import contextlib
import struct
import time

import numpy as np
import pytest

import nrs
import pose_only_cases as PC

pytestmark = pytest.mark.gpu

SWITCHES = ("NRS_PO_NO_CACHE", "NRS_PO_MULTI_MIN", "NRS_PO_MULTI_GROUPS")
FORMS = {"default": {}, "no_cache": {"NRS_PO_NO_CACHE": "1"}, "multi_g2": {"NRS_PO_MULTI_MIN": "1", "NRS_PO_MULTI_GROUPS": "2"}}


@contextlib.contextmanager
def form(**switches):
    try:
        for k, v in switches.items():
            nrs.debug_set(k, v)
        yield
    finally:
        for k in SWITCHES:
            nrs.debug_set(k, None)


def multi(g):
    return form(NRS_PO_MULTI_MIN="1", NRS_PO_MULTI_GROUPS=str(g))


def solve(ctx, name, cap=1024, n=None):
    """one call on case `name` (its first n points): pose, mask, the stored trials, count and iterations; cap None: no trace"""
    c = PC.case(name)
    cam = nrs.make_camera(c["model"], c["prm"])
    tr = nrs.Trace(cap) if cap is not None else None
    q, t, inl = ctx.pose_only_solve(cam, c["uv"][:n], c["X"][:n], c["pose_q"], c["pose_t"], tr)
    r = dict(q=q, t=t, inl=inl)
    if tr is not None:
        r.update(trials=tr.trials, count=tr.c.count, iterations=tr.iterations)
        assert len(r["trials"]) == min(r["count"], cap)
    return r


def trial_bytes(x):
    """round, iter, trial, lam, chi, chi_new, rho, accepted, ok of one trial, the doubles by their bits"""
    return struct.pack("<3i4d2i", x["round"], x["iter"], x["trial"], x["lam"], x["chi"], x["chi_new"], x["rho"], int(x["accepted"]), int(x["ok"]))


def same_bytes(a, b, trace=True):
    assert a["q"].tobytes() == b["q"].tobytes() and a["t"].tobytes() == b["t"].tobytes()
    assert np.array_equal(a["inl"], b["inl"])
    if trace:
        assert a["count"] == b["count"] and a["iterations"] == b["iterations"]
        assert [trial_bytes(x) for x in a["trials"]] == [trial_bytes(x) for x in b["trials"]]


def against_oracle(r, name):
    o = PC.oracle(name)
    tq, tt = PC.tolerance(name)
    dq, dt = np.abs(r["q"] - o["q"]).max(), np.abs(r["t"] - o["t"]).max()
    diff = r["inl"] != o["inl"]
    print("%s: |dq| %.2e (bar %.0e), |dt| %.2e (bar %.0e), mask differs at %d, %d trials in %d iterations (oracle %d in %d)" % (
        name, dq, tq, dt, tt, diff.sum(), r["count"], r["iterations"], len(o["trace"]), o["iterations"]))
    assert dq <= tq and dt <= tt
    assert not (diff & ~o["band"]).any() and diff.sum() <= min(PC.GATE_BAND_MAX, o["n_band"])
    assert PC.compare_traces(r["trials"], name) >= o["compared"]
    if o["to_the_end"]:
        assert r["count"] == len(o["trace"]) and r["iterations"] == o["iterations"]


def forms_agree(a, b, name):
    """two forms of one solve differ in the order of their fp64 sums only (the 100k-point bound of tests/test_gpu_pose_only.py)"""
    assert np.abs(a["q"] - b["q"]).max() <= PC.TOL_Q_FORMS and np.abs(a["t"] - b["t"]).max() <= PC.TOL_T_FORMS
    diff = a["inl"] != b["inl"]
    assert not (diff & ~PC.oracle(name)["band"]).any() and diff.sum() <= PC.GATE_BAND_MAX


@pytest.mark.parametrize("name", PC.LADDER)
def test_ladder_default_form_matches_oracle(ctx, name):
    """every size of the ladder on the path it takes by default: form A up to 7168 points (with and without the dynamic-LDS attribute),
    form B at 7169 and 12000"""
    against_oracle(solve(ctx, name), name)


@pytest.mark.parametrize("name", [n for n in PC.LADDER if int(n.split("_")[1]) <= 7168])
def test_form_b_equals_form_a_bit_for_bit(ctx, name):
    """where the points are read from changes neither the arithmetic nor the order of the sums: NRS_PO_NO_CACHE=1 returns the default
    run's pose bytes, inlier bytes and trace.  (Form B is thereby held to the oracle through form A at every size.)"""
    a = solve(ctx, name)
    with form(NRS_PO_NO_CACHE="1"):
        b = solve(ctx, name)
    same_bytes(a, b)


@pytest.mark.parametrize("name", PC.NARROW)
def test_form_c_on_a_narrow_grid(ctx, name):
    """form C on 1, 2 and 3 workgroups: up to ceil(7169 / 256) = 29 grid-stride trips per thread, 1-3 slots of partial sums, some of
    them empty or partly filled.  Each against the oracle, bit-reproducible between calls, and the three agreeing up to summation order."""
    runs = []
    for g in (1, 2, 3):
        with multi(g):
            r = solve(ctx, name)
            again = solve(ctx, name)
        against_oracle(r, name)
        same_bytes(r, again)
        runs.append(r)
    forms_agree(runs[0], runs[1], name)
    forms_agree(runs[0], runs[2], name)


@pytest.fixture(scope="module")
def handover_oracles():
    """the oracle on 32768 points, and on 32767 when the two runs together stay under 10 s on this host"""
    t0 = time.perf_counter()
    PC.oracle("pin_%d" % PC.HANDOVER[1])
    dt = time.perf_counter() - t0
    both = 2 * dt <= 10.0
    if both:
        PC.oracle("pin_%d" % PC.HANDOVER[0])
    print("oracle on %d points: %.1f s; %d against the oracle: %s" % (PC.HANDOVER[1], dt, PC.HANDOVER[0], both))
    return both


def test_default_handover(ctx, handover_oracles):
    """no switch set: 32767 points run form B, 32768 form C.  Both against the oracle (on a slow host 32767 against form C on the
    same points instead, at the bound between forms)."""
    lo, hi = ("pin_%d" % n for n in PC.HANDOVER)
    r_hi = solve(ctx, hi)
    against_oracle(r_hi, hi)
    r_lo = solve(ctx, lo)
    if handover_oracles:
        against_oracle(r_lo, lo)
    with form(NRS_PO_MULTI_MIN="1"):
        c_lo = solve(ctx, hi, n=PC.HANDOVER[0])
    assert np.abs(r_lo["q"] - c_lo["q"]).max() <= PC.TOL_Q_FORMS and np.abs(r_lo["t"] - c_lo["t"]).max() <= PC.TOL_T_FORMS
    assert (r_lo["inl"] != c_lo["inl"]).sum() <= PC.GATE_BAND_MAX


@pytest.mark.parametrize("which", sorted(FORMS))
@pytest.mark.parametrize("name", PC.CONTROL)
def test_control_flow(ctx, name, which):
    """runs of rejected trials within one iteration (far_seed), rounds that start with no active edge (all_outliers_after_round0:
    optimize() returns at once, the round's classification still runs) and points behind the camera, in all three forms"""
    with form(**FORMS[which]):
        r = solve(ctx, name)
    against_oracle(r, name)
    if name == "all_outliers_after_round0":
        assert not r["inl"].any() and {x["round"] for x in r["trials"]} == {0}


@pytest.mark.parametrize("which", ["default", "multi_g2"])
def test_short_trace_buffer(ctx, which):
    """a trace buffer shorter than the number of trials, and none at all: the solve is the same solve, the count goes on counting,
    and what is stored is the first trials"""
    with form(**FORMS[which]):
        full = solve(ctx, "far_seed")
        short = solve(ctx, "far_seed", cap=4)
        none = solve(ctx, "far_seed", cap=None)
        full_again = solve(ctx, "far_seed")
    assert full["count"] > 4 and len(full["trials"]) == full["count"]
    assert short["count"] == full["count"] and short["iterations"] == full["iterations"]
    assert len(short["trials"]) == 4 and [trial_bytes(x) for x in short["trials"]] == [trial_bytes(x) for x in full["trials"][:4]]
    same_bytes(short, full, trace=False)
    same_bytes(none, full, trace=False)
    same_bytes(full_again, full)                                                    # (and the long buffer after the short one)


def test_buffers_are_reused_cleanly():
    """po_level, po_err and po_multi live on the context: a small frame behind a large one, a large one behind a small one and the
    many-workgroup form behind both give, byte for byte, what the same call gives on a fresh context"""
    steps = [("pin_12000", {}), ("pin_5", {}), ("pin_7168", {}), ("pin_257", dict(NRS_PO_MULTI_MIN="1"))]
    shared = nrs.Context()
    try:
        for name, sw in steps:
            with form(**sw):
                r = solve(shared, name)
                fresh = nrs.Context()
                try:
                    f = solve(fresh, name)
                finally:
                    fresh.close()
            same_bytes(r, f)
            against_oracle(r, name)
    finally:
        shared.close()
