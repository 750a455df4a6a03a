#!/usr/bin/env python3
"""Wall time of the one-call BA windows (nrs_dba_solve_window, _rg, _embedded, _rg_embedded) on the windows of tools/solve_fingerprint.py's
one-call cases: per case two warm-up calls, then the median (and the smallest and largest) of N calls on one context, in ms.  The calls
return after their download, so the wall time of the call is the whole of it: host set-up, launches, solve, copies.  Run it once per
library (NRS_LIB=<path> selects one), alternating the libraries in one session, and compare the columns.

    python tools/one_call_window_time.py [N = 25] [substring of the case names] [--laps]

--laps: after a case's timed calls, N more with NRS_TIMING=1 on the context; the library then writes its stage laps ("[nrs] embedded
window construction / set-up / solve + download <ms>") to stderr -- redirect it to a file and take the medians per stage from there."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (os.path.join(ROOT, "nr-slam_amd", "py"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)
import nrs  # noqa: E402
import nrs_synth as S  # noqa: E402
import embedded_window_cases as W  # noqa: E402
import window_rg_cases as RGW  # noqa: E402
import window_rg_embedded_cases as RGE  # noqa: E402


def qt_of(p):
    return np.concatenate([p["poses_q"], p["poses_t"]], 1)


def resident_graph(ctx, c):
    ids = np.arange(c["n"], dtype=np.int32)
    rg = nrs.RGraph(ctx, c["n"], c["sigma"], RGW.STRETCH_TH)
    rg.add_edges(c["X0"], ids, ids)
    rg.update(c["X1"], ids)
    return rg


def timed(ctx, name, call, n, laps):
    for _ in range(2):
        call()
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        ms.append(1e3 * (time.perf_counter() - t0))
    print("%-34s median %8.3f ms   min %8.3f   max %8.3f   n=%d" % (name, float(np.median(ms)), min(ms), max(ms), n), flush=True)
    if laps:
        ctx.debug_set("NRS_TIMING", "1")
        for _ in range(n):
            call()
        ctx.debug_set("NRS_TIMING", None)


def main(argv):
    laps = "--laps" in argv
    args = [a for a in argv if a != "--laps"]
    n = int(args[0]) if args else 25
    only = args[1] if len(args) > 1 else ""
    ctx = nrs.Context()

    def run(name, call):
        if only in name:
            timed(ctx, name, call, n, laps)

    p = S.make_dba_problem(300, 4, 32)
    cam, qt = nrs.make_camera(p["model"], p["prm"]), qt_of(p)
    run("window 300x4", lambda: ctx.dba_solve_window(cam, qt, p["kf_points"], p["lm_xyz"], p["lm_uv"], p["nbr"], p["scale"], 5))
    for case in ("900x6_kb8", "120x3"):
        if only not in "rg window " + case and only not in "rg embedded " + case:
            continue
        c = RGW.case(case)
        q = c["p"]
        rg = resident_graph(ctx, c)
        cam_q, qt_q = nrs.make_camera(q["model"], q["prm"]), qt_of(q)
        run("rg window " + case, lambda: ctx.dba_solve_window_rg(cam_q, qt_q, q["kf_points"], q["lm_xyz"], q["lm_uv"], rg, q["scale"], 5))
        if case == RGE.CASES[0]:
            flag = RGE.case(case)["flag"]
            run("rg embedded " + case, lambda: ctx.dba_solve_window_rg_embedded(cam_q, qt_q, q["kf_points"], q["lm_xyz"], q["lm_uv"], rg, flag, q["scale"], 5))
        rg.close()
    e, flag_e, nb = W.window(W.CASES[0], "nodes")
    cam_e, qt_e = nrs.make_camera(e["model"], e["prm"]), qt_of(e)
    run("embedded 300x4x40", lambda: ctx.dba_solve_window_embedded(cam_e, qt_e, e["kf_points"], e["lm_xyz"], e["lm_uv"], flag_e, nb, e["scale"], 5))
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
