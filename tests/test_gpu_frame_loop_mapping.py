"""GPU: the frame loop with mapping=True through the C ABI (nrs_map_frame, nrs_rgraph_resize, nrs_map_grow_graph, the template archive)
against the same loop over the oracle backend and tests/map_oracle.py (tests/map_loop_backend.py), frame by frame."""
import numpy as np
import pytest

import map_loop_backend as B
import nrs
import nrs_frame_loop as FL

pytestmark = pytest.mark.gpu


def test_mapping_loop_matches_the_oracle_loop():
    sq = B.sequence()
    gb = FL.GpuBackend(nrs, sq["model"], sq["prm"], B.OPTS, dense_graph=True)
    try:
        gloop = B.run(gb, True)
        cap = gb.rg.cap
    finally:
        gb.close()
    oloop, _ = B.oracle_run()
    assert len(gloop.log) == len(oloop.log) == B.N_FRAMES - 1
    for f, (g, o) in enumerate(zip(gloop.log, oloop.log), 1):
        assert g["mapping"]["skipped"] == o["mapping"]["skipped"], f
        assert g["mapping"]["triangulated"] == o["mapping"]["triangulated"] and g["mapping"]["mode"] == o["mapping"]["mode"], f
        assert g["map_size"] == o["map_size"], f
        assert np.array_equal(g["status_by_map"], o["status_by_map"]) and np.array_equal(g["status_after_mapping"], o["status_after_mapping"]), f
        assert g["lost"] == o["lost"] and g["reused"] == o["reused"] and g["keyframe"] == o["keyframe"] and g["n_2d"] == o["n_2d"], f
        assert np.allclose(g["pose_q"], o["pose_q"], atol=2e-6, rtol=0) and np.allclose(g["pose_t"], o["pose_t"], atol=2e-5, rtol=0), f
        assert np.allclose(g["pos_by_map"], o["pos_by_map"], atol=2e-4, rtol=0), f
    n0 = sq["n_points"]
    assert gloop.log[-1]["map_size"] - n0 >= 5
    assert cap >= gloop.log[-1]["map_size"] and cap % n0 == 0      # the graph grew in doubled steps
