"""nrs_stereo_match_pattern (include/nrs.h "f7: evaluation") against tests/eval_oracle.py: status, match position, fp64 score and point
all exactly equal, for the matrix-core form and for the plain form (NRS_STEREO_NO_MFMA=1), which must give the same bits."""
import numpy as np
import pytest

import eval_oracle as E
import nrs
import nrs_synth as S
import stereo_cases as SC

pytestmark = pytest.mark.gpu

PRM = np.array([383.19, 383.05, 155.97, 124.34], np.float32)
BF = 2000.0
# 96 x 64, 24 keypoints: one tile of the matrix-core form in x and two short ones in y, N below one fragment
# 203 x 131, 70 keypoints: odd sizes (M and N end inside a tile), h odd (the (h-1)/2.f - 2 truncation), rows with a stride above the width
CASES = {"96x64": ((96, 64), (7, 0), 24, 0), "203x131": ((203, 131), (9, 0, 4), 70, 5)}


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def case(request):
    wh, disp, n, pad = CASES[request.param]
    p = S.make_stereo_pair(wh, 3, disp, n, row_pad=pad)
    p["oracle"] = E.stereo_match_pattern(PRM, BF, p["left"], p["right"], p["xy"])
    return p


def _run(ctx, p, right=None):
    cam = nrs.make_camera(0, PRM)
    if "left_rows" in p and right is None:
        return ctx.stereo_match_pattern(cam, BF, p["left_rows"], p["right_rows"], p["xy"], width=p["wh"][0])
    return ctx.stereo_match_pattern(cam, BF, p["left"], p["right"] if right is None else right, p["xy"])


def _same(dev, ora):
    xyz, status, score, match = dev
    o_xyz, o_status, o_score, o_match = ora
    assert np.array_equal(status, o_status)
    assert np.array_equal(match, o_match)
    assert np.array_equal(score.view(np.uint64)[~np.isnan(o_score)], o_score.view(np.uint64)[~np.isnan(o_score)])
    assert np.array_equal(np.isnan(score), np.isnan(o_score))
    assert np.array_equal(np.isnan(xyz), np.isnan(o_xyz))
    ok = o_status == E.OK
    assert np.array_equal(xyz[ok].view(np.uint32), o_xyz[ok].view(np.uint32))


def test_pattern_matcher_matches_the_oracle_exactly(ctx, case):
    dev = _run(ctx, case)
    _same(dev, case["oracle"])
    status, match = dev[1], dev[3]
    assert np.array_equal(status, case["expect_status"])          # the planted boundary, saturated and zero-disparity keypoints
    t = case["kind"].index("tie")
    assert tuple(match[t]) == (0, 0)                              # the repeated patch: the first row-major position wins


def test_plain_form_gives_identical_bits(ctx, case):
    a = _run(ctx, case)
    nrs.debug_set("NRS_STEREO_NO_MFMA", "1")
    b = _run(ctx, case)
    nrs.debug_set("NRS_STEREO_NO_MFMA", None)
    _same(b, case["oracle"])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert a[2].tobytes() == b[2].tobytes() and a[0].tobytes() == b[0].tobytes()


def _run_scene(ctx, sc, plain):
    if plain:
        nrs.debug_set("NRS_STEREO_NO_MFMA", "1")
    return ctx.stereo_match_pattern(nrs.make_camera(0, SC.PRM), SC.BF_PATTERN, sc["left"], sc["right"], sc["xy"])


@pytest.mark.parametrize("plain", [False, True], ids=["mfma", "plain"])
@pytest.mark.parametrize("second_workgroup", [False, True], ids=["first_position", "second_workgroup"])
def test_exact_ties_at_every_reduction_level(ctx, second_workgroup, plain):
    """a lattice of positions that all score exactly 1.0: ties between a lane's registers and rows, lane groups, waves, workgroups (and
    the plain form's tiles) in x and y; the first row-major position must win -- in the first workgroup, and in the second one in x and
    y (tests/stereo_cases.py lattice_scene; the conditions are asserted in tests/test_stereo_cases_cpu.py)"""
    sc = SC.lattice_scene(second_workgroup)
    SC.lattice_holds(sc)
    dev = _run_scene(ctx, sc, plain)
    print(dev[3].tolist())
    _same(dev, sc["oracle"])


@pytest.mark.parametrize("plain", [False, True], ids=["mfma", "plain"])
@pytest.mark.parametrize("name", list(SC.NEAR_TIES))
def test_near_ties_are_decided_in_fp64(ctx, name, plain):
    """two windows that differ in one grey level of one pixel: scores about 1e-7 apart (relative), which fp32 cannot order -- the later
    and better one must replace the earlier one (in one workgroup's rows, and across two workgroups), the later and worse one must not"""
    sc = SC.near_tie_scene(name)
    print(name, "relative gap %.3e" % SC.near_tie_holds(sc))
    _same(_run_scene(ctx, sc, plain), sc["oracle"])


@pytest.mark.parametrize("plain", [False, True], ids=["mfma", "plain"])
def test_all_black_right_image_scores_zero(ctx, case, plain):
    if plain:
        nrs.debug_set("NRS_STEREO_NO_MFMA", "1")
    xyz, status, score, match = _run(ctx, case, right=np.zeros_like(case["right"]))
    searched = ~np.isin(case["expect_status"], (E.OUT_OF_BOUNDS, E.SATURATED))
    assert searched.sum() > 10
    assert (score[searched] == 0).all() and (status[searched] == E.LOW_CORRELATION).all() and (match[searched] == 0).all()
    assert np.array_equal(status[~searched], case["expect_status"][~searched]) and np.isnan(xyz).all()
