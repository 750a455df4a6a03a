"""GPU: what a refused one-call BA window says and leaves behind, for each of the four entry points (nr-slam_amd/csrc/nrs_dba.hip), on the
300-point, 4-keyframe window of tests/embedded_window_cases.py and its 40-node embedded form.  An empty window is refused with
NRS_ERR_INVALID under the name of the entry point that was called; the window an earlier call left resident still answers where the entry
point checks its arguments before it drops that window (nrs_dba_solve_window, nrs_dba_solve_window_rg), and is gone where it drops it
first (the two embedded calls)."""
import numpy as np
import pytest

import embedded_window_cases as W
import nrs

pytestmark = pytest.mark.gpu

# entry point -> does the window of an earlier call survive a refused call?
CALLS = {"nrs_dba_solve_window": True, "nrs_dba_solve_window_rg": True, "nrs_dba_solve_window_embedded": False, "nrs_dba_solve_window_rg_embedded": False}


@pytest.mark.parametrize("name", list(CALLS))
def test_an_empty_window_is_refused_under_the_calls_own_name(ctx, name):
    p, flag, nb = W.window(W.CASES[0], "nodes")
    cam = nrs.make_camera(p["model"], p["prm"])
    qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
    empty = [np.zeros(0, np.int32) for _ in p["kf_points"]]
    xyz, uv = p["lm_xyz"][:0], p["lm_uv"][:0]
    rg = nrs.RGraph(ctx, p["n_points"], 1.0)                        # (never read: the window is refused before the graph serves a list)
    try:
        ctx.dba_solve_window(cam, qt, p["kf_points"], p["lm_xyz"], p["lm_uv"], p["nbr"], p["scale"], 1)      # a window is resident ...
        before = ctx.dba_stats()
        assert before["rows"] > 0
        with pytest.raises(nrs.NrsError) as e:
            if name == "nrs_dba_solve_window":
                ctx.dba_solve_window(cam, qt, empty, xyz, uv, p["nbr"], p["scale"], 1)
            elif name == "nrs_dba_solve_window_rg":
                ctx.dba_solve_window_rg(cam, qt, empty, xyz, uv, rg, p["scale"], 1)
            elif name == "nrs_dba_solve_window_embedded":
                ctx.dba_solve_window_embedded(cam, qt, empty, xyz, uv, flag, nb, p["scale"], 1)
            else:
                ctx.dba_solve_window_rg_embedded(cam, qt, empty, xyz, uv, rg, np.zeros(p["n_points"], np.uint8), p["scale"], 1)
        assert e.value.code == -1
        assert str(e.value).split("): ", 1)[1] == name + ": empty window"
        if CALLS[name]:                                             # ... and still answers
            assert ctx.dba_stats() == before
        else:                                                       # ... and is gone
            with pytest.raises(nrs.NrsError) as e2:
                ctx.dba_stats()
            assert e2.value.code == -5
    finally:
        rg.close()
