"""The evaluation oracle (tests/eval_oracle.py) on the generators' planted cases, and nrs_stereo_from_tracks (host code, no device)
against it bit for bit."""
import numpy as np
import pytest

import eval_oracle as E
import nrs_synth as S

F32 = np.float32
PRM = np.array([383.19, 383.05, 155.97, 124.34], F32)


@pytest.fixture(scope="module", params=[((96, 64), (7, 0), 24), ((203, 131), (9, 0, 4), 70)], ids=["96x64", "203x131"])
def pair(request):
    wh, disp, n = request.param
    p = S.make_stereo_pair(wh, 3, disp, n)
    p["oracle"] = E.stereo_match_pattern(PRM, 2000.0, p["left"], p["right"], p["xy"])
    return p


def test_generator_plants_every_special_keypoint(pair):
    kinds = pair["kind"]
    assert kinds.count("saturated") == 1 and kinds.count("zero") == 1 and kinds.count("tie") == 1 and kinds.count("boundary") == 5
    assert len(kinds) == len(pair["xy"]) and kinds.count("ok") >= 10


def test_oracle_matcher_finds_every_planted_disparity(pair):
    xyz, status, score, match = pair["oracle"]
    for i, k in enumerate(pair["kind"]):
        if k in ("ok", "zero"):
            assert tuple(match[i]) == tuple(pair["match"][i]) and score[i] == 1.0, (i, k)
            assert match[i][0] == int(pair["xy"][i, 0] - 7) - pair["disparity"][i]
            if status[i] == E.OK:
                disp = abs(F32(match[i][0] + 7) - pair["xy"][i, 0])
                assert xyz[i, 2] == F32(2000.0) / disp


def test_oracle_returns_the_intended_status_of_each_special_keypoint(pair):
    xyz, status, score, match = pair["oracle"]
    assert np.array_equal(status, pair["expect_status"])
    t = pair["kind"].index("tie")
    assert tuple(match[t]) == (0, 0) and score[t] == 1.0          # the copy in the corner comes first in row-major order
    rejected = status != E.OK
    assert np.isnan(xyz[rejected]).all() and np.isfinite(xyz[~rejected]).all()
    oob = status == E.OUT_OF_BOUNDS
    assert np.isnan(score[oob]).all() and (match[oob] == -1).all()


def test_one_correlation_per_cell_gives_the_bytes_of_one_per_keypoint(pair):
    """stereo_match_pattern remembers the first maximum per template cell; the statement it replaced (kept as
    stereo_match_pattern_per_keypoint) correlates once per keypoint.  The same bytes, also when cells repeat and on strided-row scenes'
    images and on the scene of the resident pair"""
    import stereo_cases as SC
    sc = SC.pattern_scene()
    twice = np.concatenate([pair["xy"][:16], pair["xy"][:16][::-1] + F32(0.125)])       # cells that repeat, with other fractions
    for left, right, xy, bf in ((pair["left"], pair["right"], pair["xy"], 2000.0), (pair["left"], pair["right"], twice, 400.0),
                                (sc["left"], sc["right"], sc["xy"], SC.BF_PATTERN), (pair["left"], pair["right"], pair["xy"][:0], 2000.0)):
        a = E.stereo_match_pattern(PRM, bf, left, right, xy)
        b = E.stereo_match_pattern_per_keypoint(PRM, bf, left, right, xy)
        for x, y, name in zip(a, b, ("xyz", "status", "score", "match")):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name
    assert np.array_equal(E.ScoreMaps(pair["left"], pair["right"]).map(30, 8).shape, E.search_dims(*pair["wh"])[::-1])


@pytest.mark.parametrize("wh, disp, n", [((96, 64), (0, 8), 40), ((203, 131), (8, 16, 4, 10, 6), 90)], ids=["96x64", "203x131"])
def test_one_correlation_per_cell_on_the_scenes_of_the_stereo_start(wh, disp, n):
    p = S.make_stereo_pair(wh, 3, disp, n)
    a = E.stereo_match_pattern(PRM, 400.0, p["left"], p["right"], p["xy"])
    b = E.stereo_match_pattern_per_keypoint(PRM, 400.0, p["left"], p["right"], p["xy"])
    for x, y, name in zip(a, b, ("xyz", "status", "score", "match")):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name


def test_stereo_from_tracks_matches_the_oracle_bit_for_bit(lib_built):
    nrs = lib_built
    rng = np.random.default_rng(4)
    n = 64
    l = np.stack([rng.uniform(30, 600, n), rng.uniform(20, 440, n)], 1).astype(F32)
    r = l.copy()
    r[:, 0] -= rng.uniform(2, 40, n).astype(F32)
    r[:, 1] += rng.uniform(-1, 1, n).astype(F32)
    st = np.full(n, 1, np.int32)
    r[0, 1] = l[0, 1] + F32(2.0)                                  # |dy| = 2.0 passes, 2.0001 does not
    l[1, 1] = F32(100.0)
    r[1, 1] = F32(102.0001)
    r[2, 0] = l[2, 0]                                             # zero disparity
    st[3], st[4] = 3, 0                                           # BAD, TRACKED_WITH_3D: only TRACKED is a match
    l[0, 1] = F32(64.0)
    r[0, 1] = F32(66.0)
    cam = nrs.make_camera(0, PRM)
    xyz, status = nrs.stereo_from_tracks(cam, 2000.0, l, r, st)
    o_xyz, o_status = E.stereo_from_tracks(PRM, 2000.0, l, r, st)
    assert np.array_equal(status, o_status)
    assert np.array_equal(xyz.view(np.uint32), o_xyz.view(np.uint32))
    assert status[0] == E.OK and status[1] == E.ROW_DIFFERENCE and status[2] == E.ZERO_DISPARITY
    assert status[3] == E.NOT_TRACKED and status[4] == E.NOT_TRACKED and (status[5:] == E.OK).all()
