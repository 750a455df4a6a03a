"""GPU: nrs_init_essential (include/nrs.h f6) against tests/init_oracle.py, stage by stage: each stage of the oracle is fed the DEVICE's bits
of the stage before, so a difference is charged where it arises.

Tolerances (tests/init_cases.py; measured by tests/test_init_oracle_cpu.py, which also asserts the caps on what may be excused):
  hyp_E    2.1e-6 = 10 x the largest disagreement of the oracle's two fp64 methods (2.1e-7 measured) -- above 4 fp32 ulp of 1 (4.8e-7)
  scores   pairs whose fp64 error lies within 2e-6 rad of the threshold may flip (<= 1 % of the pairs)
  pose     4 fp32 ulp of 1 per rotation entry and per component of t
  code     identical except within a relative 1e-5 of a gate (<= 1 % of the points); counters and verdict exact
  xyz      4.8e-6 relative = 4 x the oracle's fp32 mid-point against the same in fp64 (1.2e-6 measured)"""
import numpy as np
import pytest

import init_cases as IC
import init_oracle as IO
import nrs

pytestmark = pytest.mark.gpu
F32 = np.float32
THR = F32(0.005)


def _call(ctx, p, **kw):
    return ctx.init_essential(nrs.make_camera(p["model"], p["prm"]), p["ref_xy"], p["cur_xy"], p["status"], kw.pop("n_matches", p["n_matches"]),
                              radians_per_pixel=float(p["rpp"]), **kw)


def _quat_R(q):
    x, y, z, w = np.asarray(q, np.float64)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _check_downstream(p, r, compact_indexing=0, expect_best=False):
    """stages 4-6 of the oracle on the device's bits: scores and masks under the excusal rule, best hypothesis, pose, codes, xyz, counters, verdict"""
    cmap, rr, cr = IO.compact_unproject(p["model"], p["prm"], p["ref_xy"], p["cur_xy"], p["status"])
    nm = p["n_matches"]
    assert r["n_compact"] == len(cmap)
    o_score, excusable = [], []
    for E in r["hyp_E"]:
        m, err = IO.score(E, rr, cr, nm, THR)
        o_score.append(int(m.sum()))
        excusable.append(int(np.sum(np.abs(err - float(THR)) < IC.SCORE_BAND)))
    o_score, excusable = np.array(o_score), np.array(excusable)
    diff = np.abs(o_score - r["hyp_score"])
    print("scores: %d hypotheses differ, %d pairs excusable of %d" % (int((diff > 0).sum()), int(excusable.sum()), nm * len(o_score)))
    assert np.all(diff <= excusable)
    assert excusable.sum() <= IC.SCORE_CAP * nm * len(o_score)
    order = np.sort(o_score)[::-1]
    margin = int(order[0] - order[1]) if len(order) > 1 else 1 << 30
    if margin > 2 * int(excusable.max()):
        assert r["best_hypothesis"] == int(np.argmax(o_score))
    else:
        assert not expect_best, "winning margin %d within the excused count on a case that must compare best_hypothesis" % margin
    b = r["best_hypothesis"]
    assert r["score"] == r["hyp_score"][b] and np.array_equal(r["E"], r["hyp_E"][b])
    assert r["hyp_score"][b] == r["hyp_score"].max() and b == int(np.argmax(r["hyp_score"]))     # highest score, lowest h
    m, err = IO.score(r["E"], rr, cr, nm, THR)
    flips = m != r["inlier"]
    assert np.all(np.abs(err[flips] - float(THR)) < IC.SCORE_BAND) and r["inlier"].sum() == r["score"]
    # cameras and points from the device's E and flags
    kp_of = IO.kp_table(cmap, nm, compact_indexing)
    q, t = IO.cameras(r["E"], p["model"], p["prm"], p["ref_xy"], p["cur_xy"], r["inlier"], kp_of)
    dR, dt = np.max(np.abs(_quat_R(q) - _quat_R(r["pose_q"]))), np.max(np.abs(t.astype(np.float64) - r["pose_t"]))
    print("pose: rotation entries differ by %.3g, t by %.3g (tolerance %.3g)" % (dR, dt, IC.POSE_TOL))
    assert r["pose_q"][3] >= 0 and dR <= IC.POSE_TOL and dt <= IC.POSE_TOL
    xyz, code, counters, verdict, margins = IO.points(p["model"], p["prm"], p["ref_xy"], p["cur_xy"], r["pose_q"], r["pose_t"], r["inlier"], kp_of,
                                                      len(p["status"]), p["rpp"])
    visited = np.isfinite(margins)
    close = visited & (margins < IC.GATE_BAND)
    assert close.sum() <= IC.GATE_CAP * max(int(visited.sum()), 1)
    assert np.array_equal(code[~close], r["code"][~close])
    both = (code == 0) & (r["code"] == 0)
    if both.any():
        rel = np.linalg.norm(xyz[both].astype(np.float64) - r["xyz"][both], axis=1) / np.linalg.norm(xyz[both].astype(np.float64), axis=1)
        print("xyz: largest relative difference %.3g over %d points (tolerance %.3g)" % (rel.max(), int(both.sum()), IC.XYZ_RTOL))
        assert rel.max() <= IC.XYZ_RTOL
    assert np.all(r["xyz"][r["code"] != 0] == 0)
    assert [r["counters"][k] for k in nrs.INIT_COUNTERS] == list(counters) and r["verdict"] == verdict
    return verdict


@pytest.mark.parametrize("n_compact", IC.SAMPLER_COMPACT)
@pytest.mark.parametrize("n_hyp", [16, 256])
def test_sampler_matches_the_restatement(ctx, n_compact, n_hyp):
    p = IC.sampler_case(n_compact)
    r = _call(ctx, p, n_hypotheses=n_hyp, seed=4)
    labels, centres, samples = IO.sampler(p["ref_xy"][p["status"] == 1], n_hyp, 4)
    assert r["n_compact"] == n_compact
    assert np.array_equal(r["labels"], labels) and np.array_equal(r["samples"], samples)
    assert np.array_equal(r["centres"].view(np.uint32), centres.view(np.uint32))
    if n_compact == 8:
        assert sorted(r["labels"]) == list(range(8))
    r2 = _call(ctx, p, n_hypotheses=n_hyp, seed=5)                   # another seed: other picks from the same clusters
    assert np.array_equal(r2["labels"], labels) and (n_compact == 8 or not np.array_equal(r2["samples"], samples))


@pytest.mark.parametrize("name", IC.HYP_CASES)
def test_hypotheses_match_the_fp64_restatement(ctx, name):
    p = IC.case(name)
    _, rr, cr = IC.rays(name)
    samples = IC.samples(name, 256)[2]
    r = _call(ctx, p, n_hypotheses=256, samples=samples)
    assert np.array_equal(r["samples"], samples)
    worst = 0.0
    for s, E in zip(samples, r["hyp_E"]):
        ref = IO.compute_E(rr[s], cr[s])
        worst = max(worst, float(np.max(np.abs(IO.align_sign(E, ref).astype(np.float64) - ref))))
    print("%s: hyp_E differs from the restatement by at most %.3g (tolerance %.3g)" % (name, worst, IC.HYP_E_TOL))
    assert worst <= IC.HYP_E_TOL
    _check_downstream(p, r)


@pytest.mark.parametrize("name,n_hyp,ok", [("pinhole300", 16, True), ("kb8_300", 16, True), ("outlier30", 16, False), ("outlier30", 1024, True)])
def test_cases_end_to_end(ctx, name, n_hyp, ok):
    p = IC.case(name)
    r = _call(ctx, p, n_hypotheses=0 if n_hyp == 16 else n_hyp)
    assert r["n_hypotheses"] == n_hyp
    o = IC.oracle(name, n_hyp)
    assert np.array_equal(r["labels"], o["labels"]) and np.array_equal(r["samples"], o["samples"])
    verdict = _check_downstream(p, r, expect_best=n_hyp == 16 and name != "outlier30")      # (margins asserted by tests/test_init_oracle_cpu.py)
    assert (verdict == 0) == ok and (o["verdict"] == 0) == ok


def test_fewer_than_eight_matches_is_verdict_1(ctx):
    p = dict(IC.case("pinhole300"))
    p["status"] = np.where(np.arange(300) < 7, 1, 3).astype(np.int32)
    r = _call(ctx, p, n_matches=7)
    assert r["verdict"] == nrs.INIT_FEW_MATCHES and np.all(r["code"] == 1) and np.all(r["xyz"] == 0)


def test_pure_rotation_fails_as_the_oracle_says(ctx):
    p = IC.case("rotation")
    r = _call(ctx, p)
    verdict = _check_downstream(p, r)
    assert verdict in (2, 3) and verdict == IC.oracle("rotation", 16)["verdict"]


def test_compact_indexing_against_the_reference_indexing(ctx):
    p = IC.case("untracked")
    r0, r1 = _call(ctx, p, compact_indexing=0), _call(ctx, p, compact_indexing=1)
    assert np.array_equal(r0["hyp_E"], r1["hyp_E"]) and np.array_equal(r0["inlier"], r1["inlier"])      # the quirk starts behind the flags
    assert not np.array_equal(r0["code"], r1["code"]) and r0["counters"] != r1["counters"]
    _check_downstream(p, r0, 0)
    _check_downstream(p, r1, 1)
    assert np.all(r1["code"][p["status"] != 1] == 1)                 # through the compact map no untracked keypoint is ever read


def test_bad_arguments_are_refused(ctx):
    p = IC.case("pinhole300")
    with pytest.raises(nrs.NrsError) as e:
        _call(ctx, p, struct_size=36)
    assert e.value.code == -1
    bad = np.array(IC.samples("pinhole300", 16)[2])
    bad[3, 5] = 300
    with pytest.raises(nrs.NrsError) as e:
        _call(ctx, p, n_hypotheses=16, samples=bad)
    assert e.value.code == -1
    bad[3, 5] = -1
    with pytest.raises(nrs.NrsError) as e:
        _call(ctx, p, n_hypotheses=16, samples=bad)
    assert e.value.code == -1
    with pytest.raises(nrs.NrsError) as e:
        _call(ctx, p, n_hypotheses=4097)
    assert e.value.code == -1


@pytest.mark.parametrize("name", ["pinhole300", "whole4000"])
def test_whole_call_with_1024_hypotheses(ctx, name):
    p = IC.case(name)
    r = _call(ctx, p, n_hypotheses=1024)
    cmap = np.where(p["status"] == 1)[0]
    labels, centres, samples = IO.sampler(p["ref_xy"][cmap], 1024, 4)
    assert np.array_equal(r["labels"], labels) and np.array_equal(r["samples"], samples)
    assert np.array_equal(r["centres"].view(np.uint32), centres.view(np.uint32))
    assert _check_downstream(p, r) == 0
