"""The frame loop with keyframe_ba=True (nr-slam_amd/py/nrs_frame_loop.py: the keyframe store, the unmapped queue, Mapping::KeyFrameMapping
through the backend's dba_window, Frame::SetFromKeyFrame) driven by the oracle backend of tests/kf_loop_backend.py, no GPU: the 25 frames
at 320 x 240 of tests/map_loop_backend.py, a keyframe every sixth frame."""
import numpy as np
import pytest

import kf_loop_backend as K
import map_loop_backend as B
import nrs_frame_loop as FL


def _same(x, y):
    if isinstance(x, dict):
        return isinstance(y, dict) and set(x) == set(y) and all(_same(x[k], y[k]) for k in x)
    if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
        return np.array_equal(x, y)
    return x == y


def test_keyframe_ba_off_is_todays_loop():
    """keyframe_ba=False through the new constructor argument: the log of map_loop_backend.oracle_run(), entry for entry"""
    sq = B.sequence()
    n = 9                                                          # the first frame and the first keyframe frame (the sixth) are among them
    loop = K.run(B.MappingOracleBackend(sq["model"], sq["prm"], B.OPTS, dense_graph=True), n_frames=n, keyframe_ba=False)
    ref, _ = B.oracle_run()
    assert len(loop.log) == n - 1 and len(ref.log) == B.N_FRAMES - 1
    for f, (a, b) in enumerate(zip(loop.log, ref.log)):
        assert _same(a, b), f
    assert not hasattr(loop, "keyframes") and any(L["mapping"]["skipped"] == "KeyFrameMapping" for L in loop.log)


def test_the_same_frames_take_the_keyframe_branch_and_windows_of_3_4_5_are_solved():
    loop, b, _ = K.oracle_run()
    ref, _ = B.oracle_run()
    kf_frames = [f for f, L in enumerate(loop.log) if "set_from" in L["mapping"]]
    assert kf_frames == [f for f, L in enumerate(ref.log) if L["mapping"]["skipped"] == "KeyFrameMapping"]
    assert kf_frames[0] == 0 and all(loop.log[f]["keyframe"] for f in kf_frames[1:])
    assert all(L["mapping"]["skipped"] is None for L in loop.log)
    # keyframe ids from a counter: the initial keyframe, then one per keyframe frame; each is handed out on its own frame (one id queued)
    assert [loop.log[f]["mapping"]["set_from"] for f in kf_frames] == list(range(len(kf_frames)))
    assert sorted(loop.keyframes) == list(range(len(kf_frames))) and loop.unmapped.ids == []
    bas = [loop.log[f]["mapping"]["ba"] for f in kf_frames]
    assert bas[0] is None and bas[1] is None                       # one and two keyframes: OPT:922-924
    assert [x["n_kf"] for x in bas[2:]] == [3, 4, 5][:len(bas) - 2] and len(bas) >= 5
    for j, (x, w) in enumerate(zip(bas[2:], b.windows)):
        assert x["n_lm"] == sum(len(k) for k in w["kf_points"]) > 0 and x["n_spring"] == len(w["edges"]["sp_d0"]) > 0
        assert x["n_damper"] == len(w["edges"]["dm_w"]) > 0 and x["trials"] >= 5
        # flattened oldest first, the TRACKED_WITH_3D slots in keyframe index order
        for kp, i in zip(w["kf_points"], list(range(j + 3))[-5:]):   # the j-th window: keyframes 0 .. j + 2 exist, the five largest ids
            kf = loop.keyframes[i]
            assert np.array_equal(kp, kf.map_index[kf.status == FL.TRACKED_WITH_3D])
    # frames that map (no keyframe pending) still triangulate: the map grows as it does without BA
    assert loop.log[-1]["map_size"] > B.sequence()["n_points"]


def test_after_a_ba_frame_the_frame_is_the_keyframe():
    loop, b, snaps = K.oracle_run()
    checked = 0
    for f, L in enumerate(loop.log):
        if "set_from" not in L["mapping"] or L["mapping"]["ba"] is None:
            continue
        kf, s = loop.keyframes[L["mapping"]["set_from"]], snaps[f]
        if kf.id != max(loop.keyframes):                           # a later window has moved this keyframe again: compare the last one only
            continue
        checked += 1
        assert np.array_equal(s["pose"][0], kf.pose[0]) and np.array_equal(s["pose"][1], kf.pose[1])
        assert np.array_equal(s["last_pose"][0], kf.pose[0]) and np.array_equal(s["last_pose"][1], kf.pose[1])
        m = kf.status == FL.TRACKED_WITH_3D
        assert m.sum() >= 10 and np.array_equal(s["status"], kf.status) and np.array_equal(s["map_index"], kf.map_index)
        assert np.array_equal(s["pos"], kf.pos) and np.array_equal(s["kp"], kf.kp) and np.array_equal(s["kp_id"], kf.kp_id)
        assert (s["pos"][~m] == 0).all() and (s["map_index"][~m] == -1).all()
        # the BA moved the keyframe: its pose is not the tracked pose the frame had, and its points are not the tracked ones
        assert not np.array_equal(L["pose_t"], kf.pose[1])
        assert not np.array_equal(L["pos_by_map"][kf.map_index[m]], kf.pos[m])
    assert checked == 1


def test_write_back_leaves_map_pos_alone():
    """one BA step on a loop stopped before it: map_pos is bit for bit what it was, the keyframes moved"""
    sq = B.sequence()
    b = K.KeyframeOracleBackend(sq["model"], sq["prm"], B.OPTS, dense_graph=True)
    loop = K.run(b, n_frames=12)                                   # keyframes 0 (initial), 1 (frame 6); frame 12 would insert the third
    loop.insert_keyframe()                                         # a third keyframe of the current frame: a window of three
    before = loop.map_pos.copy()
    kf_before = {i: (kf.pos.copy(), kf.pose[1].copy()) for i, kf in loop.keyframes.items()}
    ba = loop.keyframe_mapping()
    assert ba["n_kf"] == 3 and np.array_equal(loop.map_pos, before)
    for i, kf in loop.keyframes.items():
        assert kf.pos.dtype == np.float32 and kf.pose[0].dtype == np.float32 and kf.pose[1].dtype == np.float32
        assert not np.array_equal(kf.pos, kf_before[i][0]) and not np.array_equal(kf.pose[1], kf_before[i][1])
        assert np.isclose(np.linalg.norm(kf.pose[0].astype(np.float64)), 1.0, atol=1e-6)
        assert (kf.pos[kf.status == FL.TRACKED] == 0).all()


def test_unmapped_queue_returns_the_front_and_pops_the_back():
    q = FL.UnmappedQueue()
    assert q.next() is None
    for i in (3, 5, 8):
        q.push(i)
    assert q.next() == 3 and q.ids == [3, 5]                       # map.cc:62-72: front(), then pop_back()
    assert q.next() == 3 and q.ids == [3]
    q.push(9)
    assert q.next() == 3 and q.ids == [3]                          # keyframe 9 is never mapped
    assert q.next() == 3 and q.ids == []
    assert q.next() is None


def test_both_keyframes_of_the_initialisation_are_inserted():
    """from_initialization with keyframe_ba: the reference frame's keyframe (id 0, identity pose, reference keypoints and positions) and the
    current frame's (id 1); the initialisation's own DoMapping leaves the reference keyframe queued"""
    class _B:                                                      # the calls from_initialization makes, nothing behind them
        dense = True

        def make_graph(self, graph, X0):
            return dict(graph)

        def klt_set_reference(self, im, pts):
            pass

        def klt_get_templates(self, n):
            return [None] * n

        def dba_window(self, *a):
            raise AssertionError("not called")
    rng = np.random.default_rng(3)
    n = 12
    X = np.column_stack([rng.uniform(-1, 1, (n, 2)), rng.uniform(4, 6, n)]).astype(np.float32)
    res = dict(reference_keypoints=rng.uniform(0, 300, (n, 2)).astype(np.float32), current_keypoints=rng.uniform(0, 300, (n, 2)).astype(np.float32),
               reference_landmark_positions=X, current_landmark_positions=(X + 0.01).astype(np.float32),
               pose_q=np.array([0, 0, 0, 1], np.float32), pose_t=np.array([0.1, 0, 0], np.float32))
    loop = FL.FrameLoop.from_initialization(_B(), None, (320, 240), res, None, mapping=True, rad_per_pixel=1e-3, camera=(0, None), keyframe_ba=True)
    assert sorted(loop.keyframes) == [0, 1] and loop.unmapped.ids == [0]
    k0, k1 = loop.keyframes[0], loop.keyframes[1]
    s = np.float32(loop.scale)
    assert np.array_equal(k0.kp, res["reference_keypoints"]) and np.array_equal(k0.pos, (X * s).astype(np.float32))
    assert np.array_equal(k0.pose[0], [0, 0, 0, 1]) and np.array_equal(k0.pose[1], [0, 0, 0])
    assert np.array_equal(k1.kp, res["current_keypoints"]) and np.array_equal(k1.pos, loop.pos) and np.array_equal(k1.pose[1], loop.pose[1])
    assert (k0.status == FL.TRACKED_WITH_3D).all() and np.array_equal(k0.map_index, np.arange(n)) and np.array_equal(k1.map_index, np.arange(n))


def test_keyframe_ba_needs_mapping_and_a_backend_that_solves_windows():
    sq = B.sequence()
    args = (None, sq["wh"], sq["scale"], sq["kp0"], sq["X0"], sq["graph"], sq["pose_q"][0], sq["pose_t"][0], sq["images"][0])
    with pytest.raises(ValueError, match="mapping=True"):
        FL.FrameLoop(K.KeyframeOracleBackend(sq["model"], sq["prm"], B.OPTS, dense_graph=True), *args, keyframe_ba=True)
    with pytest.raises(ValueError, match="dba_window"):
        FL.FrameLoop(B.MappingOracleBackend(sq["model"], sq["prm"], B.OPTS, dense_graph=True), *args, mapping=True, rad_per_pixel=B.RAD_PER_PIXEL,
                     camera=(sq["model"], sq["prm"]), keyframe_ba=True)
