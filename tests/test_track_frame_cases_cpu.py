"""a2 on frames that are a permuted, partial view of the map (tests/track_frame_cases.py), without a GPU:
  * the NumPy oracle and the C++ restatement (oracle/nrs_cpu_track.hpp) agree on such a frame, flat graph, plain and embedded -- the
    assertions and tolerances of tests/test_oracle_cpp_track_cpu.py, which passes f_map = arange(n) throughout;
  * the scenes of tests/test_gpu_track_frames.py reach the branches they were made for.  These are conditions on the ORACLE's walks
    (track_frame_cases.replay_walks / replay_lost_walks), checked so that a scene cannot silently stop reaching its branch.

Values of the committed seeds (the assertions below are the floors):
  Scene A (1200 map points, sigma 0.434, 170 slots, 129 optimised, 18 lost points; lists of ~300 entries):
    longest walk 365 entries; stops: 106 x "eleven" (100 beyond entry 64, 67 beyond 128), 8 x "bad" (7 beyond 64: entry 71, after the
    70 NEUTRAL ones), 15 x "exhausted" (13 beyond 64, 10 beyond 128, the longest list 277); the lost point in the frame's hole
    (map point 839) is first met at 0-based position 115 of the list that finds it, map point 887 at 85.  In embedded mode (40
    nodes) the lists a source serves without the passed-over connections are walked to entry 400 at most, 110 walks beyond entry 128.
  Scene B (260 map points, sigma 0.6, the whole map within 1.4 sigma; 18 lost points): map point 135 forces the stage-2 retry: 239 kept
    entries, 3 optimised neighbours among the first 32, the eleventh at entry 51; the other 17 lost points keep 199 entries and end at
    their 12th.  Every stage-1 walk there stops at "eleven" within its first 64 entries."""
import collections

import numpy as np
import pytest

import nrs_cpu as CPU
import nrs_oracle as O
import track_frame_cases as T
from test_oracle_cpp_track_cpu import _same_leading_trials


@pytest.fixture(scope="module")
def cpu_lib():
    CPU.build()
    return CPU.load()


def test_frame_view_is_a_permuted_partial_view():
    tp, fr = T.flat_case()
    fm = fr["f_map"]
    mapped = fm >= 0
    ids = fm[mapped]
    assert len(np.unique(ids)) == len(ids) == 300 and (~mapped).sum() == 25
    assert np.any(np.diff(ids) < 0) and not mapped[:-25].all()      # neither ascending nor with the unmapped slots at the end
    assert np.array_equal(fr["f_pos"][mapped], tp["X_prev"][ids]) and np.array_equal(fr["f_uv"][mapped], tp["uv"][ids])
    assert not fr["f_pos"][~mapped].any() and not fr["f_uv"][~mapped].any() and (fr["f_status"][~mapped] == O.TRACKED).all()
    st = collections.Counter(fr["f_status"][mapped].tolist())
    assert st[O.JUST_TRIANGULATED] == 3 and st[O.TRACKED] > 0 and st[O.TRACKED_WITH_3D] > 200
    changed = fr["f_status"][mapped] != tp["status"][ids]
    assert changed.sum() == 3 and (tp["status"][ids][changed] == O.TRACKED_WITH_3D).all()
    srt = T.make_frame_view(tp, 300, 25, 7, permute=False)
    assert np.all(np.diff(srt["f_map"][srt["f_map"] >= 0]) > 0)


def test_restatements_agree_on_a_permuted_partial_frame(cpu_lib):
    tp, fr = T.flat_case()
    otr = []
    o = O.track_deform_solve(tp["model"], tp["prm"], tp["graph"], tp["X_prev"], fr["f_map"], fr["f_status"], fr["f_uv"], fr["f_pos"],
                             tp["pose_q"], tp["pose_t"], tp["scale"], otr)
    r = CPU.track_deform_solve(tp["model"], tp["prm"], tp["graph"], tp["X_prev"], fr["f_map"], fr["f_status"], fr["f_uv"], fr["f_pos"],
                               tp["pose_q"], tp["pose_t"], tp["scale"], cpu_lib)
    assert len(o["lost"]) > 0
    assert np.array_equal(r["f_status"], o["f_status"]) and r["lost"] == list(o["lost"])
    assert np.allclose(r["pose_q"], o["pose_q"], atol=1e-9) and np.allclose(r["pose_t"], o["pose_t"], atol=1e-8)
    assert np.allclose(r["f_pos"], o["f_pos"], atol=1e-6) and np.allclose(r["map_pos"], o["map_pos"], atol=1e-6)
    for k in ("e_status",):
        assert np.array_equal(r["graph"][k], o["graph"][k])
    for k in ("e_w", "e_max", "e_min"):
        assert np.allclose(r["graph"][k], o["graph"][k], atol=1e-6)
    assert abs(r["median"] - o["median"]) <= 1e-6
    assert _same_leading_trials(r["trace"], otr, len(otr)) > 10
    assert r["stats"]["n_factor"] == r["stats"]["n_trials"] > 0


def test_embedded_restatements_agree_on_a_permuted_partial_frame(cpu_lib):
    import embedded_oracle as E
    import skin_oracle as K
    tp, fr = T.flat_case()
    eligible = np.zeros(len(tp["X_prev"]), bool)
    eligible[T.optimised_ids(fr)] = True
    node = T.node_flags(fr, K.select_nodes(tp["X_prev"], 60, eligible))
    per_map_id = np.zeros(len(tp["X_prev"]), np.uint8)
    per_map_id[fr["f_map"][node == 1]] = 1
    assert node.sum() == 60 and not np.array_equal(node[:len(per_map_id)], per_map_id[:len(node)])   # laid out per slot, not per map id
    otr = []
    o = E.track_deform_solve_embedded(tp["model"], tp["prm"], tp["graph"], tp["X_prev"], fr["f_map"], fr["f_status"], fr["f_uv"], fr["f_pos"], node,
                                      tp["pose_q"], tp["pose_t"], tp["scale"], otr)
    r = CPU.track_deform_solve_embedded(tp["model"], tp["prm"], tp["graph"], tp["X_prev"], fr["f_map"], fr["f_status"], fr["f_uv"], fr["f_pos"], node,
                                        tp["pose_q"], tp["pose_t"], tp["scale"], cpu_lib)
    n_opt = len(T.optimised_ids(fr))
    assert (r["n_nodes"], r["n_skinned"]) == (o["n_nodes"], o["n_skinned"]) and r["n_skinned"] > 0.3 * n_opt
    assert np.array_equal(r["f_status"], o["f_status"]) and r["lost"] == list(o["lost"])
    assert np.allclose(r["pose_q"], o["pose_q"], atol=1e-9) and np.allclose(r["pose_t"], o["pose_t"], atol=1e-8)
    assert np.allclose(r["f_pos"], o["f_pos"], atol=1e-6) and np.allclose(r["map_pos"], o["map_pos"], atol=1e-6)
    assert np.array_equal(r["graph"]["e_status"], o["graph"]["e_status"])
    for k in ("e_w", "e_max", "e_min"):
        assert np.allclose(r["graph"][k], o["graph"][k], atol=1e-6)
    assert abs(r["median"] - o["median"]) <= 1e-6
    assert _same_leading_trials(r["trace"], otr, len(otr)) > 8


def test_scene_a_reaches_the_later_chunks_of_the_walk():
    sc, before, good, o, otr = T.dense_oracle_run("A")
    fr = sc["frame"]
    walks, lost_first = T.replay_walks(before, fr["f_map"], fr["f_status"])
    assert sorted(lost_first) == o["lost"]                          # the replay is the oracle's walk
    assert [w["id"] for w in walks] == T.optimised_ids(fr).tolist() and np.any(np.diff(T.optimised_ids(fr)) < 0)
    stops = collections.Counter(w["how"] for w in walks)
    print("scene A: N %d, longest walk %d, stops %s, lost %d" % (len(walks), max(w["visited"] for w in walks), dict(stops), len(o["lost"])))
    for how in ("eleven", "bad", "exhausted"):
        v = [w["visited"] for w in walks if w["how"] == how]
        print("  %-9s %3d walks, %3d beyond entry 64, %3d beyond 128, longest %d" % (how, len(v), sum(x > 64 for x in v), sum(x > 128 for x in v), max(v)))
    print("  lost points first met at position >= 64:", {k: v for k, v in lost_first.items() if v >= 64})
    assert max(w["visited"] for w in walks) > 128
    assert any(w["how"] == "eleven" and w["visited"] > 64 for w in walks)
    assert any(w["how"] == "bad" and w["visited"] > 64 for w in walks)
    assert any(w["how"] == "exhausted" for w in walks)
    assert any(pos >= 64 for pos in lost_first.values()) and lost_first[sc["hole_pt"]] >= 64
    # cap_per_point 16 grows 16 -> 64 -> 256 -> 1024: a walk that needs more than 256 entries makes grow() run three times
    assert any(w["visited"] > 256 for w in walks)
    # the history's UpdateVertex calls did something: BAD connections exist, and the special points' lists end in them
    assert (before.st == O.GRAPH_BAD).sum() > 1000 and all(g.min() >= 0 for g in good)


def test_scene_a_embedded_walks_are_long_on_the_served_lists():
    import skin_oracle as K
    sc, before, good, o, otr = T.dense_oracle_run("A")
    fr, tp = sc["frame"], sc["tp"]
    eligible = np.zeros(len(tp["X_prev"]), bool)
    eligible[T.optimised_ids(fr)] = True
    node = T.node_flags(fr, K.select_nodes(tp["X_prev"], 40, eligible))
    walks, _ = T.replay_walks(before, fr["f_map"], fr["f_status"], node)
    print("scene A embedded: longest served walk %d, %d beyond entry 128" % (max(w["listed"] for w in walks), sum(w["listed"] > 128 for w in walks)))
    assert sum(w["listed"] > 128 for w in walks) > 10 and all(w["listed"] <= w["visited"] for w in walks)
    assert any(w["listed"] < w["visited"] for w in walks)           # connections are passed over: the `skip` bytes matter


def test_scene_b_reaches_the_stage_2_retry():
    sc, before, good, o, otr = T.dense_oracle_run("B")
    fr = sc["frame"]
    assert len(otr) == 3 and sc["retry_pt"] in o["lost"]            # stage 2 ran
    lw = T.replay_lost_walks(o["graph"], fr["f_map"], fr["f_status"], o["lost"])
    for k, v in lw.items():
        print("scene B: lost point %d keeps %d entries, %d optimised among the first 32, the eleventh at %s%s"
              % (k, len(v["kept"]), v["n_opt_first32"], v["eleventh"], "  <- retry" if T.stage2_retries(v) else ""))
    retry = [k for k, v in lw.items() if T.stage2_retries(v)]
    inside = [k for k, v in lw.items() if v["eleventh"] is not None and v["eleventh"] < 32]
    assert sc["retry_pt"] in retry and len(inside) >= 1
    v = lw[sc["retry_pt"]]
    # its nearest BAD connections lead to points that are not optimised, the farther ones to optimised points
    first_bad = next(k for k, e in enumerate(v["kept"]) if e[2] == O.GRAPH_BAD)
    assert first_bad < 11 and not any(e[1] for e in v["kept"][first_bad:32]) and v["eleventh"] is not None and 32 < v["eleventh"] <= 128
    # stage 1 of this scene stays in the first chunk (cap_per_point = n never retries there)
    walks, _ = T.replay_walks(before, fr["f_map"], fr["f_status"])
    assert all(w["how"] == "eleven" for w in walks)
