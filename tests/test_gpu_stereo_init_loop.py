"""GPU: a sequence started from a stereo pair -- Shi-Tomasi on the left image, nrs_init_stereo, FrameLoop.from_stereo_initialization and two
tracked frames with mapping, on nrs_synth.make_stereo_init_sequence (320 x 240), against the same loop over the oracles
(oracle/shi_oracle.py, tests/stereo_init_oracle.py over tests/eval_oracle.py, tests/map_loop_backend.py).

The extractor, the matcher and the clustering are exact, so both runs select the same keypoints with the same positions; the tracked frames
then agree as the mono start's do (tests/test_gpu_init_loop.py): the same statuses, nearly every point tracked, a reprojection error below a
pixel -- and, both loops starting from identical maps, poses within the tolerance tests/test_gpu_frame_loop_mapping.py holds the two
backends to: 2e-6 on the quaternion, and its 2e-5 on the translation in a map of median depth 3 taken to this metric map of median depth
60 mm, 4e-4 mm.

The metric claim: the recovered depth of every selected point is the planted one to the matcher's resolution.  The keypoints are integer,
so the template is cut at the keypoint itself; the matcher returns the integer disparity nearest to the true one (0.5 px) and the true
disparity varies by less than 1 px over a 15 px window of this surface (slope 8/15 mm per mm, 0.16 mm per px, 1.5 mm per px of disparity),
which moves the best integer by at most another 0.5 px: |bf / z - planted disparity| <= 1 px."""
import functools

import numpy as np
import pytest

import nrs
import nrs_frame_loop as FL
import nrs_synth as S
import stereo_init_oracle as SO
from map_loop_backend import OPTS, RAD_PER_PIXEL, MappingOracleBackend

pytestmark = pytest.mark.gpu
F32 = np.float32
MAX_FEATURES = 250                                                     # thinned evenly, as MonoInitializer does (the oracle matcher is slow)
MIN_SELECTED = 100


class StereoOracleBackend(MappingOracleBackend):
    def init_stereo(self, left, right, kp, **options):
        kp = np.asarray(kp, F32).reshape(-1, 2)
        r = SO.init_stereo(self.prm, left, right, kp, **options)
        r["selected_keypoints"] = kp[r["selected"]].copy()
        return r


def _start(backend, sq):
    xy, _ = backend.extract_features(sq["images"][0], None, None)
    xy = np.asarray(xy, F32).reshape(-1, 2)
    if len(xy) > MAX_FEATURES:
        xy = xy[(np.arange(MAX_FEATURES) * len(xy)) // MAX_FEATURES]
    r = backend.init_stereo(sq["images"][0], sq["right"], xy, bf=sq["bf"], z_min=sq["z_min"], z_max=sq["z_max"], eps=sq["eps"],
                            min_points=sq["min_points"])
    return xy, r


def _loop(backend, sq, r):
    proj = lambda pc: FL.project_f32(sq["model"], sq["prm"], pc)
    loop = FL.FrameLoop.from_stereo_initialization(backend, proj, sq["wh"], r, sq["images"][0], mapping=True, rad_per_pixel=RAD_PER_PIXEL,
                                                   camera=(sq["model"], sq["prm"]))
    for f in (1, 2):
        assert loop.track_image(sq["images"][f])
    return loop


@functools.lru_cache(maxsize=None)
def oracle_run():
    """computed once, on the CPU, before anything runs on the device: (scene, keypoints, result, loop)"""
    sq = S.make_stereo_init_sequence()
    b = StereoOracleBackend(sq["model"], sq["prm"], OPTS, dense_graph=True)
    xy, r = _start(b, sq)
    assert r["verdict"] == 0 and r["n_selected"] >= MIN_SELECTED, "the ORACLE alone must select %d points: %d" % (MIN_SELECTED, r["n_selected"])
    return sq, xy, r, _loop(b, sq, r)


def test_a_sequence_starts_from_a_stereo_pair():
    sq, o_xy, o, o_loop = oracle_run()
    proj = lambda pc: FL.project_f32(sq["model"], sq["prm"], pc)
    gb = FL.GpuBackend(nrs, sq["model"], sq["prm"], OPTS, dense_graph=True)
    try:
        g_xy, g = _start(gb, sq)
        assert np.array_equal(g_xy, o_xy)
        print("selected %d of %d keypoints (%d matched, %d gated, %d clusters, %d noise), median depth %.4f" %
              (g["n_selected"], len(g_xy), g["n_matched"], g["n_gated"], g["n_clusters"], g["n_noise"], g["median_depth"]))
        # the selected set equals the oracle's, bit for bit
        for k in ("verdict", "n_matched", "n_gated", "n_clusters", "n_noise", "n_selected"):
            assert int(g[k]) == int(o[k]), k
        for k in ("match_status", "code", "raw_label", "label", "selected"):
            assert np.array_equal(g[k], o[k]), k
        assert g["selected_xyz"].tobytes() == o["selected_xyz"].tobytes() and np.array_equal(g["selected_keypoints"], o["selected_keypoints"])
        assert F32(g["median_depth"]) == F32(o["median_depth"]) and g["n_selected"] >= MIN_SELECTED
        # metric scale: planted depths to the matcher's integer-disparity resolution (see the module's header)
        d_true = sq["disparity_at"](g["selected_keypoints"])
        d_rec = sq["bf"] / g["selected_xyz"][:, 2].astype(np.float64)
        known = ~np.isnan(d_true)
        err = np.abs(d_rec - d_true)[known]
        print("disparity error: max %.3f px over %d of %d selected points" % (err.max(), known.sum(), len(known)))
        assert known.sum() >= 0.8 * len(known) and err.max() <= 1.0
        z_true = sq["bf"] / d_true[known]
        assert np.max(np.abs(g["selected_xyz"][known, 2] - z_true) / z_true) <= 1.0 / d_true[known].min()
        # the tail of Tracking::StereoMapInitialization, then two tracked frames
        loop = _loop(gb, sq, g)
        n = g["n_selected"]
        assert loop.scale == 1.0 and len(loop.map_pos) >= n and loop.init_median_depth == F32(o["median_depth"])
        # the first tracked frame finds no unmapped keyframe: FrameMapping, not the skipped KeyFrameMapping of the mono start
        for lp in (loop, o_loop):
            assert lp.log[0]["mapping"]["skipped"] is None and "n_rigid" in lp.log[0]["mapping"]
        for f in (0, 1):
            a, b = loop.log[f], o_loop.log[f]
            assert a["n_tracked"] > 0.9 * n
            assert np.array_equal(a["status_by_map"], b["status_by_map"]) and a["lost"] == b["lost"] and a["keyframe"] == b["keyframe"]
            dq = np.max(np.abs(a["pose_q"].astype(np.float64) - b["pose_q"]))
            dt = np.max(np.abs(a["pose_t"].astype(np.float64) - b["pose_t"]))
            print("frame %d: pose against the oracle loop: q %.3g, t %.3g mm" % (f + 1, dq, dt))
            assert dq <= 2e-6 and dt <= 4e-4
        last = loop.log[-1]
        ok = last["status_by_map"] == FL.TRACKED_WITH_3D
        uv = proj(FL.se3f_act((last["pose_q"], last["pose_t"]), last["pos_by_map"][ok]))
        m = loop.map_index >= 0
        assert np.median(np.linalg.norm(uv - loop.kp[m][loop.status[m] == FL.TRACKED_WITH_3D], axis=1)) < 1.0
        # metric: the camera moved `step` mm per frame sideways; the recovered translation is that, in mm, with no rescale
        t_true = np.asarray(sq["t"][2], np.float64)
        assert np.linalg.norm(last["pose_t"] - t_true) < 0.5 * np.linalg.norm(t_true) + 0.1
    finally:
        gb.close()


def test_from_stereo_initialization_keyframe_state_and_refusals():
    sq, o_xy, o, _ = oracle_run()
    proj = lambda pc: FL.project_f32(sq["model"], sq["prm"], pc)
    gb = FL.GpuBackend(nrs, sq["model"], sq["prm"], OPTS, dense_graph=True)
    flat = FL.GpuBackend(nrs, sq["model"], sq["prm"], OPTS)
    try:
        with pytest.raises(ValueError):
            FL.FrameLoop.from_stereo_initialization(flat, proj, sq["wh"], o, sq["images"][0])
        with pytest.raises(ValueError):
            FL.FrameLoop.from_stereo_initialization(gb, proj, sq["wh"], dict(o, verdict=1, n_selected=0), sq["images"][0])
        loop = FL.FrameLoop.from_stereo_initialization(gb, proj, sq["wh"], o, sq["images"][0], mapping=True, rad_per_pixel=RAD_PER_PIXEL,
                                                       camera=(sq["model"], sq["prm"]), keyframe_ba=True)
        # ONE keyframe (tracking.cc:283-286), already taken from the queue by the initialisation's own DoMapping
        assert list(loop.keyframes) == [0] and loop.unmapped.ids == [] and loop.unmapped_keyframes == 0
        kf = loop.keyframes[0]
        assert np.array_equal(kf.kp, o["selected_keypoints"]) and kf.pos.tobytes() == o["selected_xyz"].tobytes()
        assert np.array_equal(kf.pose[0], [0, 0, 0, 1]) and not kf.pose[1].any() and np.all(loop.status == FL.TRACKED_WITH_3D)
        assert abs(float(loop.graph.sigma if hasattr(loop.graph, "sigma") else 10.5) - 10.5) < 1e-6
        assert loop.track_image(sq["images"][1])
        assert "ba" not in loop.log[0]["mapping"] and "n_rigid" in loop.log[0]["mapping"]            # FrameMapping on the first frame
    finally:
        gb.close()
        flat.close()
