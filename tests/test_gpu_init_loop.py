"""GPU: a sequence started from images -- nrs_frame_loop.MonoInitializer over the C ABI (Shi-Tomasi, LK, nrs_init_essential) against the same
class over the oracles (oracle/shi_oracle.py, oracle/lk_oracle.py, tests/init_oracle.py) on nrs_synth.make_init_sequence (320 x 240, at most
400 features, 8 frames), then FrameLoop.from_initialization and two tracked frames.

LK and Shi-Tomasi are bit-exact, so both runs reset on the same frames, hand the same arrays to the solve and report the same verdicts; the
map points are the same set; pose, positions, scale and sigma agree within the end-to-end tolerances of tests/init_cases.py (derived there
from HYP_E_TOL: the two fp64 SVD routes may differ before the fp32 rounding of E)."""
import numpy as np
import pytest

import init_cases as IC
import init_oracle as IO
import nrs
import nrs_frame_loop as FL
from frame_loop_backend import OracleBackend

pytestmark = pytest.mark.gpu
F32 = np.float32


class InitOracleBackend(OracleBackend):
    def init_essential(self, ref_xy, cur_xy, status, n_matches, **options):
        return IO.initialize(self.model, self.prm, ref_xy, cur_xy, status, n_matches, **options)


def _run(backend, sq, max_images, n_frames):
    mo = FL.MonoInitializer(backend, max_images=max_images, max_features=400, radians_per_pixel=F32(sq["radians_per_pixel"]))
    for f in range(n_frames):
        r = mo.process_new_image(sq["images"][f], sq["mask"])
        if r is not None:
            return mo, r, f
    return mo, None, n_frames


def _same_logs(g, o):
    assert len(g.log) == len(o.log)
    for f, (a, b) in enumerate(zip(g.log, o.log)):
        assert (a["reset"], a["n_features"], a["n_tracks"], a["verdict"]) == (b["reset"], b["n_features"], b["n_tracks"], b["verdict"]), (f, a, b)
        for k in ("ref_xy", "cur_xy", "status"):
            assert (k in a) == (k in b) and (k not in a or np.array_equal(a[k], b[k])), (f, k)


def _quat_R(q):
    return FL.se3f_act((np.asarray(q, F32), np.zeros(3, F32)), np.eye(3, dtype=F32)).T.astype(np.float64)


def test_a_sequence_starts_from_images():
    sq = IC.init_sequence()
    proj = lambda pc: FL.project_f32(sq["model"], sq["prm"], pc)
    om, o, fo = _run(InitOracleBackend(sq["model"], sq["prm"], IC.LOOP_KLT, dense_graph=True), sq, 30, 8)
    gb = FL.GpuBackend(nrs, sq["model"], sq["prm"], IC.LOOP_KLT, dense_graph=True)
    try:
        gm, g, fg = _run(gb, sq, 30, 8)
        assert o is not None and g is not None and fg == fo and 2 <= fg <= 5
        _same_logs(gm, om)
        assert [e["reset"] for e in gm.log] == [True] + [False] * fg and gm.log[-1]["verdict"] == 0
        assert any(e["verdict"] not in (None, 0) for e in gm.log)                       # the first baselines are too short: failed verdicts first
        assert np.array_equal(g["index"], o["index"]) and len(g["index"]) >= 100          # the same map points
        assert np.array_equal(g["current_keypoints"], o["current_keypoints"]) and np.array_equal(g["reference_keypoints"], o["reference_keypoints"])
        dR = np.max(np.abs(_quat_R(g["pose_q"]) - _quat_R(o["pose_q"])))
        dt = np.max(np.abs(g["pose_t"].astype(np.float64) - o["pose_t"]))
        xo = o["current_landmark_positions"].astype(np.float64)
        rel = np.max(np.linalg.norm(g["current_landmark_positions"] - xo, axis=1) / np.linalg.norm(xo, axis=1))
        print("pose: R %.3g, t %.3g (tolerance %.3g); positions %.3g relative (tolerance %.3g)" % (dR, dt, IC.POSE_E2E_TOL, rel, IC.XYZ_E2E_RTOL))
        assert dR <= IC.POSE_E2E_TOL and dt <= IC.POSE_E2E_TOL and rel <= IC.XYZ_E2E_RTOL
        # the motion is the true one: unit translation direction within a few degrees (LK noise over a 1 mm baseline)
        t_true = sq["t"][fg] / np.linalg.norm(sq["t"][fg])
        assert float(np.dot(g["pose_t"], t_true)) > 0.99
        # the tail of Tracking::MonocularMapInitialization, then two tracked frames
        loop = FL.FrameLoop.from_initialization(gb, proj, sq["wh"], g, sq["images"][fg])
        depths = o["current_landmark_positions"][:, 2]
        k = len(depths) // 2
        scale_o = F32(3) / np.sort(depths)[k]
        sig_o = F32(F32(FL.sigma_f32(depths) * scale_o) * F32(3))
        print("scale %.8g against %.8g, graph sigma %.8g against %.8g" % (loop.scale, scale_o, loop.init_sigma_graph, sig_o))
        assert abs(loop.scale - scale_o) <= IC.XYZ_E2E_RTOL * scale_o and abs(loop.init_sigma_graph - sig_o) <= 2 * IC.XYZ_E2E_RTOL * sig_o + 1e-6
        assert abs(np.median(loop.pos[:, 2]) - 3.0) < 0.05 and np.all(loop.status == FL.TRACKED_WITH_3D)
        for f in (fg + 1, fg + 2):
            assert loop.track_image(sq["images"][f])
            assert loop.log[-1]["n_tracked"] > 0.9 * len(g["index"])
        last = loop.log[-1]
        ok = last["status_by_map"] == FL.TRACKED_WITH_3D
        uv = proj(FL.se3f_act((last["pose_q"], last["pose_t"]), last["pos_by_map"][ok]))
        assert np.median(np.linalg.norm(uv - loop.kp[loop.map_index >= 0][loop.status[loop.map_index >= 0] == FL.TRACKED_WITH_3D], axis=1)) < 1.0
    finally:
        gb.close()


def test_the_reference_is_renewed_on_the_same_frames():
    """max_images = 2: ResetInitialization on frames 0 and 3, the device-driven run and the oracle-driven one alike"""
    sq = IC.init_sequence()
    om, o, _ = _run(InitOracleBackend(sq["model"], sq["prm"], IC.LOOP_KLT), sq, 2, 5)
    gb = FL.GpuBackend(nrs, sq["model"], sq["prm"], IC.LOOP_KLT)
    try:
        gm, g, _ = _run(gb, sq, 2, 5)
    finally:
        gb.close()
    assert o is None and g is None
    _same_logs(gm, om)
    assert [e["reset"] for e in gm.log] == [True, False, False, True, False]
