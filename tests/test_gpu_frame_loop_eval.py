"""FrameLoop.evaluate (py/nrs_frame_loop.py): six frames of a synthetic sequence with depth images.  Per frame the recorded rmse and
scale equal, exactly, those of the oracle's evaluator (tests/eval_oracle.py) fed the loop's own pose, positions and keypoints."""
import numpy as np
import pytest

import eval_oracle as E
import nrs
import nrs_frame_loop as FL
import nrs_synth as S

pytestmark = pytest.mark.gpu
OPTS = dict(win=21, max_level=4, max_iters=10, epsilon=1e-4, min_eig=1e-4)


def test_six_frames_are_scored_as_the_oracle_scores_them():
    frames = 6
    sq = S.make_frame_sequence(220, frames, 9, S.PINHOLE)
    gb = FL.GpuBackend(nrs, sq["model"], sq["prm"], OPTS)
    try:
        proj = lambda pc: FL.project_f32(sq["model"], sq["prm"], pc)
        loop = FL.FrameLoop(gb, proj, sq["wh"], sq["scale"], sq["kp0"], sq["X0"], sq["graph"], sq["pose_q"][0], sq["pose_t"][0],
                            sq["images"][0], images_to_insert_keyframe=2)
        for f in range(frames):
            if f:
                assert loop.track_image(sq["images"][f])
            depth = S.make_depth_image(sq, f)
            rec = loop.evaluate(depth=depth)
            m = loop.status == FL.TRACKED_WITH_3D
            gt, st = E.depth_ground_truth(sq["model"], sq["prm"], depth, loop.kp[m])
            rmse, scale, counts, gw = E.eval_frame(np.concatenate(loop.pose), loop.pos[m], gt, st, True)
            assert rec["rc"] == 0 and rec["n"] == int(m.sum()) and rec["counts"] == tuple(counts), f
            assert np.float32(rec["rmse"]).tobytes() == np.float32(rmse).tobytes(), (f, rec["rmse"], rmse)
            assert np.float32(rec["scale"]).tobytes() == np.float32(scale).tobytes(), (f, rec["scale"], scale)
            assert np.array_equal(np.isnan(loop.ground_truth), np.isnan(gw))
            assert np.array_equal(loop.ground_truth[st == 0].view(np.uint32), gw[st == 0].view(np.uint32)), f
            assert abs(float(scale) - 1.0) < 0.05 and float(rmse) < 0.05, (f, rmse, scale)     # the map is at the scene's scale
        assert len(loop.rmse) == frames
    finally:
        gb.close()
