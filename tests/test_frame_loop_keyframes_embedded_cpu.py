"""The frame loop with mapping=True, keyframe_ba=True in the embedded-deformation mode, driven by the oracle backend of
tests/kf_embedded_loop_backend.py, no GPU: the 25 frames of tests/map_loop_backend.py with 40 of the initial map points as nodes."""
import numpy as np

import kf_embedded_loop_backend as KE
import map_loop_backend as B


def test_the_embedded_oracle_loop_maps_and_solves_windows_of_3_4_5():
    loop, b = KE.oracle_run()
    n0 = B.sequence()["n_points"]
    assert len(loop.log) == B.N_FRAMES - 1 and all(L["mapping"]["skipped"] is None for L in loop.log)
    # the node set is the initial map's: 40 nodes, every map point added by mapping skinned
    assert loop.log[-1]["map_size"] == len(loop.map_pos) > n0
    assert len(b.node_flag) == len(loop.map_pos) and b.node_flag[:n0].sum() == KE.N_NODES and not b.node_flag[n0:].any()
    bas = [L["mapping"]["ba"] for L in loop.log if "set_from" in L["mapping"]]
    assert bas[0] is None and bas[1] is None                       # one and two keyframes: OPT:922-924
    assert [x["n_kf"] for x in bas[2:]] == [3, 4, 5] == [len(w["kf_points"]) for w in b.windows]
    new_skinned = 0
    for x, w in zip(bas[2:], b.windows):
        e = w["edges"]
        n_obs = sum(len(k) for k in w["kf_points"])
        assert x["n_lm"] == n_obs and x["n_spring"] == len(e["sp_d0"]) > 0 and x["n_damper"] == len(e["dm_w"]) > 0 and x["trials"] >= 5
        pts = np.concatenate(w["kf_points"])
        assert 0 < len(e["lm_obs"]) < n_obs and len(e["sk_obs"]) > 0 and (w["flag"][pts[e["lm_obs"]]] == 1).all() and (w["flag"][pts[e["sk_obs"]]] == 0).all()
        new_skinned += int((pts[e["sk_obs"]] >= n0).sum())
        # a map point added by mapping that reaches no node copy: the oracle leaves it out of the skinned list (it constrains nothing)
        bound = np.zeros(n_obs, bool)
        bound[e["lm_obs"]] = True
        bound[e["sk_obs"]] = True
        assert (w["flag"][pts[~bound]] == 0).all()
    assert new_skinned > 0                                         # a skinned observation of a map point added by mapping


def test_the_ba_moves_the_keyframes_it_solves():
    loop, b = KE.oracle_run()
    last = max(loop.keyframes)
    kf = loop.keyframes[last]
    L = next(L for L in loop.log if L["mapping"].get("set_from") == last)
    assert L["mapping"]["ba"] is not None and not np.array_equal(L["pose_t"], kf.pose[1])
    assert kf.pos.dtype == np.float32 and np.isfinite(kf.pos).all()
