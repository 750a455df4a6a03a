"""nrs_dbscan3d and nrs_init_stereo (include/nrs.h "f8") against tests/stereo_init_oracle.py.  Every comparison is exact: integers and
fp32 bits.  The clustering on the device is the fixed-point formulation (minimum-label propagation over the core points), the oracle is the
sequential textbook algorithm: two different algorithms that must agree label for label."""
import numpy as np
import pytest

import eval_oracle as E
import nrs
import nrs_synth as S
import stereo_cases as SC
import stereo_init_oracle as SO

pytestmark = pytest.mark.gpu
F32 = np.float32

CLUSTER_CASES = S.make_cluster_cases()
PRM = np.array([383.19, 383.05, 155.97, 124.34], F32)
BF = 400.0
# 96 x 64: a band of disparity 0 (zero-disparity and far keypoints: beyond z_max) and one of disparity 8, whose keypoints sit at disparities
#   8, 8.25, 8.5 and 8.75: z_min is EXACTLY the depth of 8.5, so those are excluded by the strict comparison, 8.75 lies below the gate
# 203 x 131 with a row stride: bands at 8, 16, 4, 10 (depths 50, 25, 100, 40): z_min = 40 excludes the integer keypoints of the last band
#   exactly on it, the others lie beyond either end; the gated points fall into two clusters and noise
SCENES = {"96x64": dict(wh=(96, 64), disp=(0, 8), n=40, pad=0, z_min=float(F32(BF) / F32(8.5)), z_max=60.0, eps=3.0, min_points=2),
          "203x131": dict(wh=(203, 131), disp=(8, 16, 4, 10, 6), n=90, pad=5, z_min=40.0, z_max=60.0, eps=2.0, min_points=3)}
FIELDS = ("verdict", "n_matched", "n_gated", "n_clusters", "n_noise", "n_selected")
ARRAYS = ("match_status", "code", "raw_label", "label", "selected")


@pytest.mark.parametrize("case", CLUSTER_CASES, ids=[c["name"] for c in CLUSTER_CASES])
def test_dbscan3d_matches_the_sequential_oracle(ctx, case):
    for nc in (True, False):
        raw, lab, counts = ctx.dbscan3d(case["xyz"], case["eps"], case["min_points"], nc)
        o_raw, o_lab, o_counts = SO.dbscan3d(case["xyz"], case["eps"], case["min_points"], nc)
        print(case["name"], nc, "counts", list(counts), "oracle", list(o_counts))
        assert np.array_equal(raw, o_raw), (case["name"], nc)
        assert np.array_equal(lab, o_lab), (case["name"], nc)
        assert np.array_equal(counts, o_counts), (case["name"], nc)


LARGE = SC.LARGE_CLUSTER_CASES


@pytest.mark.parametrize("case", LARGE, ids=[c["name"] for c in LARGE])
def test_dbscan3d_past_one_chunk_and_one_trip(ctx, case):
    """the carried count of the root compaction (roots in the second and third chunk of 1024), the second to fourth trip of the
    lane-strided word loops (more than 4096 points) and the limit of 16384 points; tests/test_stereo_init_oracle_cpu.py asserts that every
    case holds its property"""
    exp = SC.cluster_expected(case["name"])
    for nc in (True, False):
        raw, lab, counts = ctx.dbscan3d(case["xyz"], case["eps"], case["min_points"], nc)
        o_raw, o_lab, o_counts = exp[nc]
        print(case["name"], nc, "counts", list(counts), "oracle", list(o_counts))
        assert np.array_equal(raw, o_raw), (case["name"], nc)
        assert np.array_equal(lab, o_lab), (case["name"], nc)
        assert np.array_equal(counts, o_counts), (case["name"], nc)


def test_dbscan3d_at_the_limit_twice_then_a_small_set_in_the_same_buffer(ctx):
    full = SC.cluster_case("full16384")
    assert len(full["xyz"]) == nrs.DBSCAN_MAX_POINTS
    a = ctx.dbscan3d(full["xyz"], full["eps"], full["min_points"], True)
    b = ctx.dbscan3d(full["xyz"], full["eps"], full["min_points"], True)
    for x, y, o in zip(a, b, SC.cluster_expected("full16384")[True]):
        assert x.tobytes() == y.tobytes() and np.array_equal(x, o)
    small = next(c for c in CLUSTER_CASES if c["name"] == "blobs63")
    for nc in (True, False):
        r = ctx.dbscan3d(small["xyz"], small["eps"], small["min_points"], nc)
        for x, o in zip(r, SO.dbscan3d(small["xyz"], small["eps"], small["min_points"], nc)):
            assert np.array_equal(x, o), nc


def test_dbscan3d_refusals(ctx):
    xyz = np.zeros((4, 3), F32)
    for kw in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(min_points=0), dict(n=-1),
               dict(n=nrs.DBSCAN_MAX_POINTS + 1)):
        with pytest.raises(nrs.NrsError) as e:
            ctx.dbscan3d(xyz, **kw)
        assert e.value.code == -1, kw
    raw, lab, counts = ctx.dbscan3d(xyz)                               # the context still works
    assert list(raw) == [-1] * 4 and list(lab) == [0] * 4 and list(counts) == [0, 4, 4]


@pytest.fixture(scope="module", params=list(SCENES), ids=list(SCENES))
def scene(request):
    c = SCENES[request.param]
    p = S.make_stereo_pair(c["wh"], 3, c["disp"], c["n"], row_pad=c["pad"])
    p["opts"] = dict(bf=BF, z_min=c["z_min"], z_max=c["z_max"], eps=c["eps"], min_points=c["min_points"])
    p["oracle"] = SO.init_stereo(PRM, p["left"], p["right"], p["xy"], **p["opts"])
    return p


def _run(ctx, p, **over):
    cam = nrs.make_camera(0, PRM)
    opts = dict(p["opts"], **over)
    if "left_rows" in p:
        return ctx.init_stereo(cam, p["left_rows"], p["right_rows"], p["xy"], width=p["wh"][0], **opts)
    return ctx.init_stereo(cam, p["left"], p["right"], p["xy"], **opts)


def _same(r, o):
    for k in FIELDS:
        assert int(r[k]) == int(o[k]), (k, r[k], o[k])
    for k in ARRAYS:
        assert np.array_equal(r[k], o[k]), k
    assert np.array_equal(np.isnan(r["xyz"]), np.isnan(o["xyz"]))
    ok = o["match_status"] == E.OK
    assert np.array_equal(r["xyz"][ok].view(np.uint32), o["xyz"][ok].view(np.uint32))
    assert r["selected_xyz"].tobytes() == o["selected_xyz"].tobytes()
    assert F32(r["median_depth"]).tobytes() == F32(o["median_depth"]).tobytes() or (np.isnan(r["median_depth"]) and np.isnan(o["median_depth"]))


def test_init_stereo_matches_the_oracle_exactly(ctx, scene):
    o = scene["oracle"]
    print({k: o[k] for k in FIELDS}, "codes", np.bincount(o["code"], minlength=4))
    # the scene holds what it is made for: every code but (on the small scene) 3, every planted matcher status, a keypoint exactly on z_min
    assert o["verdict"] == 0 and o["n_selected"] >= 3 and (o["code"] == 1).any() and (o["code"] == 2).any()
    assert {E.OUT_OF_BOUNDS, E.SATURATED}.issubset(set(o["match_status"]))
    z = o["xyz"][:, 2]
    on_min = (o["match_status"] == E.OK) & (z == F32(scene["opts"]["z_min"]))
    assert on_min.any() and np.all(o["code"][on_min] == 2)
    with np.errstate(invalid="ignore"):
        assert ((o["code"] == 2) & (z < F32(scene["opts"]["z_min"]))).any() and ((o["code"] == 2) & (z > F32(scene["opts"]["z_max"]))).any()
    _same(_run(ctx, scene), o)


def test_init_stereo_scene_with_other_clusters_and_noise(ctx):
    p = dict(SCENES["203x131"])
    sc = S.make_stereo_pair(p["wh"], 3, p["disp"], p["n"], row_pad=p["pad"])
    sc["opts"] = dict(bf=BF, z_min=p["z_min"], z_max=p["z_max"], eps=p["eps"], min_points=p["min_points"])
    for nc in (1, 0):
        o = SO.init_stereo(PRM, sc["left"], sc["right"], sc["xy"], noise_competes=nc, **sc["opts"])
        assert o["n_clusters"] >= 2 and o["n_noise"] > 0 and (o["code"] == 3).any()
        _same(_run(ctx, sc, noise_competes=nc), o)


def test_init_stereo_holds_the_matcher_refactor(ctx, scene):
    """xyz / match_status are what nrs_stereo_match_pattern returns for the same inputs"""
    cam = nrs.make_camera(0, PRM)
    if "left_rows" in scene:
        xyz, st, _, _ = ctx.stereo_match_pattern(cam, BF, scene["left_rows"], scene["right_rows"], scene["xy"], width=scene["wh"][0])
    else:
        xyz, st, _, _ = ctx.stereo_match_pattern(cam, BF, scene["left"], scene["right"], scene["xy"])
    r = _run(ctx, scene)
    assert np.array_equal(st, r["match_status"]) and xyz.tobytes() == r["xyz"].tobytes()
    assert np.array_equal(st, scene["expect_status"])


def test_init_stereo_plain_form_gives_identical_bits(ctx, scene):
    a = _run(ctx, scene)
    nrs.debug_set("NRS_STEREO_NO_MFMA", "1")
    try:
        b = _run(ctx, scene)
    finally:
        nrs.debug_set("NRS_STEREO_NO_MFMA", None)
    _same(b, scene["oracle"])
    for k in ARRAYS + ("xyz", "selected_xyz"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_init_stereo_verdict_when_nothing_passes_the_gate(ctx, scene):
    o = SO.init_stereo(PRM, scene["left"], scene["right"], scene["xy"], **dict(scene["opts"], z_min=1e5, z_max=2e5))
    r = _run(ctx, scene, z_min=1e5, z_max=2e5)
    assert o["verdict"] == 1 and r["verdict"] == 1 and r["n_gated"] == 0 and r["n_selected"] == 0 and len(r["selected"]) == 0
    assert np.isnan(r["median_depth"])
    _same(r, o)
    r = ctx.init_stereo(nrs.make_camera(0, PRM), scene["left"], scene["right"], np.zeros((0, 2), F32))      # no keypoints: the same verdict
    assert r["verdict"] == 1 and r["n_matched"] == 0


def test_init_stereo_refusals(ctx, scene):
    nan, inf = float("nan"), float("inf")
    bad = [dict(struct_size=0), dict(struct_size=8), dict(result_struct_size=4), dict(n=nrs.DBSCAN_MAX_POINTS + 1), dict(eps=0.0), dict(eps=-2.5),
           dict(eps=nan), dict(eps=inf), dict(min_points=0), dict(z_min=50.0, z_max=50.0), dict(z_min=60.0, z_max=50.0), dict(z_min=nan),
           dict(n=-1), dict(stride_l=scene["wh"][0] - 1)]
    for kw in bad:
        with pytest.raises(nrs.NrsError) as e:
            _run(ctx, scene, **kw)
        assert e.value.code == -1, kw
    cam = nrs.make_camera(0, PRM)
    with pytest.raises(nrs.NrsError) as e:                             # the matcher's own: an image below 32 x 32
        ctx.init_stereo(cam, np.zeros((24, 40), np.uint8), np.zeros((24, 40), np.uint8), scene["xy"])
    assert e.value.code == -1
    _same(_run(ctx, scene), scene["oracle"])                           # the context still works


# ---- three chunks of keypoints: the carried counts of k_si_gate (over the keypoints) and k_si_select (over the gated points), rows of the
# clustering wider than the words in use.  tests/test_stereo_cases_cpu.py asserts the scene's conditions without a device too
@pytest.fixture(scope="module")
def big():
    p = SC.init_scene_three_chunks()
    SC.init_three_chunks_holds(p)                                      # before the device is asked
    return p


def _run_big(ctx, p, nc=1):
    return ctx.init_stereo(nrs.make_camera(0, PRM), p["left"], p["right"], p["xy"], noise_competes=nc, **p["opts"])


@pytest.mark.parametrize("nc", [1, 0], ids=["noise_competes", "noise_apart"])
def test_init_stereo_with_three_chunks_of_keypoints(ctx, big, nc):
    o = big["oracle"][nc]
    print({k: o[k] for k in FIELDS}, "codes", np.bincount(o["code"], minlength=4))
    _same(_run_big(ctx, big, nc), o)


def test_init_stereo_three_chunks_plain_form_gives_identical_bits(ctx, big):
    a = _run_big(ctx, big)
    nrs.debug_set("NRS_STEREO_NO_MFMA", "1")
    try:
        b = _run_big(ctx, big)
    finally:
        nrs.debug_set("NRS_STEREO_NO_MFMA", None)
    _same(b, big["oracle"][1])
    for k in ARRAYS + ("xyz", "selected_xyz"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_init_stereo_three_chunks_on_the_resident_pair_and_the_matcher_alone(ctx, big):
    cam = nrs.make_camera(0, PRM)
    dev = nrs.Context()
    try:
        out = dev.front_process_stereo(big["left"], big["right"], outputs=("gray", "gray_right"))
        assert np.array_equal(out["gray"], big["left"]) and np.array_equal(out["gray_right"], big["right"])
        for nc in (1, 0):
            _same(dev.init_stereo_front(cam, big["xy"], noise_competes=nc, **big["opts"]), big["oracle"][nc])
    finally:
        dev.close()
    xyz, st, _, _ = ctx.stereo_match_pattern(cam, BF, big["left"], big["right"], big["xy"])
    r = _run_big(ctx, big)
    assert np.array_equal(st, r["match_status"]) and xyz.tobytes() == r["xyz"].tobytes()
