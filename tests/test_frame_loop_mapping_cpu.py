"""The frame loop with mapping=True (nr-slam_amd/py/nrs_frame_loop.py: Mapping::DoMapping's FrameMapping branch + UpdateTriangulatedPoints)
driven by the oracle backend over tests/map_oracle.py, no GPU: 25 frames at 320 x 240, a keyframe every sixth frame."""
import numpy as np

import map_loop_backend as B
import nrs_frame_loop as FL


def test_the_map_grows_and_the_new_points_are_tracked():
    loop, b = B.oracle_run()
    log = loop.log
    sq = B.sequence()
    n0 = sq["n_points"]
    assert len(log) == B.N_FRAMES - 1 and sum(L["keyframe"] for L in log) >= 2
    # KeyFrameMapping is skipped, and said so, on the first frame (the initialisation's second keyframe) and on every keyframe frame
    for f, L in enumerate(log):
        assert (L["mapping"]["skipped"] == "KeyFrameMapping") == (f == 0 or L["keyframe"]), f
    assert log[-1]["map_size"] - n0 >= 5 and len(loop.map_pos) == log[-1]["map_size"]
    grew = [f for f, L in enumerate(log) if L["mapping"]["triangulated"]]
    assert grew and all(log[f]["mapping"]["mode"] in (1, 2) for f in grew)
    size, n_new, n_took_part = n0, 0, 0
    for f, L in enumerate(log):
        new = np.arange(size, size + len(L["mapping"]["triangulated"]))
        size += len(new)
        assert L["map_size"] == size
        # AddGeometryToKeypoint: JUST_TRIANGULATED after the mapping of the frame ...
        assert (L["status_after_mapping"][new] == FL.JUST_TRIANGULATED).all()
        assert not (L["status_by_map"] == FL.JUST_TRIANGULATED).any()          # ... and never when a frame's tracking has run:
        if len(new) and f + 1 < len(log):                                       # UpdateTriangulatedPoints made them TRACKED_WITH_3D first,
            f_map, f_status, n_map = b.deform_calls[f + 1]                      # so they take part in a2 on the next frame
            assert n_map == size
            n_new += len(new)                                                   # (LK may lose a point on that very frame: counted over all of them)
            n_took_part += int(np.isin(new, f_map[f_status == FL.TRACKED_WITH_3D]).sum())
    assert n_new >= 5 and n_took_part >= 0.8 * n_new
    # the triangulated keypoint ids are ids of extracted corners (fresh class_ids, beyond the initial map's), each triangulated once
    ids = [i for L in log for i in L["mapping"]["triangulated"]]
    assert min(ids) >= n0 and len(set(ids)) == len(ids)
    # later frames still track most of the grown map
    assert log[-1]["n_tracked"] > 0.8 * log[-1]["map_size"]
    # TemporalBuffer: pop before insert at size() > 20 -- 21 snapshots, never more
    assert len(loop.tbuf.snaps) == 21


def test_temporal_buffer_pops_before_it_inserts():
    tbuf = FL.TemporalBuffer(20)
    for f in range(40):
        tbuf.insert(np.array([5, 9, 11]), np.full((3, 2), f, np.float32), np.zeros((3, 3)), np.array([0, 1, 3]), np.array([0, 0, 0, 1.0]), np.zeros(3),
                    0.001 * f)
        assert len(tbuf.snaps) == min(f + 1, 21)
    tb, mag, ids = tbuf.flat(0, None)
    assert ids.tolist() == [5, 9] and tb["has_kp"].shape == (21, 2) and tb["has_kp"].all() and tb["status"].tolist() == [0, 1]
    assert np.isclose(mag[-1], 0.039) and np.isclose(mag[0], 0.019) and tb["kp_xy"][0, 0, 0] == 19


def test_mapping_off_is_todays_loop():
    sq = B.sequence()
    a = B.run(B.MappingOracleBackend(sq["model"], sq["prm"], B.OPTS, dense_graph=True), False, 8).log
    from frame_loop_backend import OracleBackend
    proj = lambda pc: FL.project_f32(sq["model"], sq["prm"], pc)
    loop = FL.FrameLoop(OracleBackend(sq["model"], sq["prm"], B.OPTS, dense_graph=True), proj, sq["wh"], sq["scale"], sq["kp0"], sq["X0"], sq["graph"],
                        sq["pose_q"][0], sq["pose_t"][0], sq["images"][0], images_to_insert_keyframe=B.KF_EVERY, mapping=False)
    for f in range(1, 8):
        assert loop.track_image(sq["images"][f])
    keys = {"pose_q", "pose_t", "lost", "reused", "n_tracked", "keyframe", "n_2d", "kp_2d", "status_by_map", "pos_by_map"}
    for x, y in zip(a, loop.log):
        assert set(x) == keys and set(y) == keys                   # today's fields, nothing of the mapping
        for k in keys:
            assert np.array_equal(x[k], y[k]) if isinstance(x[k], np.ndarray) else x[k] == y[k], k
    assert not hasattr(loop, "tbuf") and any(L["keyframe"] for L in a)
