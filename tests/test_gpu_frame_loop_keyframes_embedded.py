"""GPU: the frame loop with mapping=True, keyframe_ba=True on a GpuBackend(n_nodes=40) -- nrs_track_deform_solve_embedded on a graph that
grows, nrs_dba_solve_window_rg_embedded on the keyframes -- against the same loop over the oracle backend of
tests/kf_embedded_loop_backend.py, frame by frame: the comparisons and tolerances of tests/test_gpu_frame_loop_keyframes.py."""
import numpy as np
import pytest

import kf_embedded_loop_backend as KE
import kf_loop_backend as K
import map_loop_backend as B
import nrs
import nrs_frame_loop as FL

pytestmark = pytest.mark.gpu


def test_embedded_keyframe_ba_loop_matches_the_oracle_loop():
    sq = B.sequence()
    gb = FL.GpuBackend(nrs, sq["model"], sq["prm"], B.OPTS, n_nodes=KE.N_NODES)
    try:
        gloop = K.run(gb)
        gflag = gb.node_flag.copy()
    finally:
        gb.close()
    oloop, ob = KE.oracle_run()
    n_map = len(oloop.map_pos)
    assert np.array_equal(gflag[:n_map], ob.node_flag) and not gflag[n_map:].any()
    assert len(gloop.log) == len(oloop.log) == B.N_FRAMES - 1
    windows = []
    for f, (g, o) in enumerate(zip(gloop.log, oloop.log), 1):
        assert g["mapping"]["skipped"] is None and o["mapping"]["skipped"] is None, f
        assert g["mapping"]["triangulated"] == o["mapping"]["triangulated"] and g["mapping"]["mode"] == o["mapping"]["mode"], f
        assert ("set_from" in g["mapping"]) == ("set_from" in o["mapping"]), f
        if "set_from" in o["mapping"]:
            assert g["mapping"]["set_from"] == o["mapping"]["set_from"], f
            gba, oba = g["mapping"]["ba"], o["mapping"]["ba"]
            assert (gba is None) == (oba is None), f
            if oba is not None:
                assert all(gba[k] == oba[k] for k in ("n_kf", "n_lm", "n_spring", "n_damper")), (f, gba, oba)
                windows.append(oba["n_kf"])
        assert g["map_size"] == o["map_size"], f
        assert np.array_equal(g["status_by_map"], o["status_by_map"]) and np.array_equal(g["status_after_mapping"], o["status_after_mapping"]), f
        assert g["lost"] == o["lost"] and g["reused"] == o["reused"] and g["keyframe"] == o["keyframe"] and g["n_2d"] == o["n_2d"], f
        assert np.allclose(g["pose_q"], o["pose_q"], atol=2e-6, rtol=0) and np.allclose(g["pose_t"], o["pose_t"], atol=2e-5, rtol=0), f
        assert np.allclose(g["pos_by_map"], o["pos_by_map"], atol=2e-4, rtol=0), f
    assert windows == [3, 4, 5]
    # the keyframes the two loops end with: the optimised poses and positions
    assert sorted(gloop.keyframes) == sorted(oloop.keyframes)
    for i in gloop.keyframes:
        a, b = gloop.keyframes[i], oloop.keyframes[i]
        assert np.array_equal(a.map_index, b.map_index) and np.array_equal(a.status, b.status)
        assert np.allclose(a.pose[0], b.pose[0], atol=2e-6, rtol=0) and np.allclose(a.pose[1], b.pose[1], atol=2e-5, rtol=0)
        assert np.allclose(a.pos, b.pos, atol=2e-4, rtol=0)
