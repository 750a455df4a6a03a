"""What the calls of the device-resident RegularizationGraph cost at the tracked-fps size: 4446 points, all pairs (include/nrs.h nrs_rgraph_*).

Per-call medians of wall clock (every call ends in a wait for the stream) in one process on one context, after a warm-up:
  add_edges            every point against every point
  update_one_pass      half of the points, each once: the pass over the stored triangle
  update_per_vertex    the same list with its first id once more: a duplicate takes the per-vertex form
  get_edges_mirror     GetEdges of every point, 128 entries per point: the full-matrix mirrors are built and scanned
  get_edges_triangle   the same under NRS_RG_NO_MIRROR
  a2_frame             nrs_track_deform_solve_rg on the frame of tests/test_gpu_track5k.py (pinhole), the graph put back before every call
and a digest of what the calls returned, so that two libraries (NRS_LIB) can be held to one another.  One JSON line.
    python tools/rgraph_probe.py [--reps 20] [--warm 3] [--out profiles/rgraph_probe.jsonl]"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nr-slam_amd", "py"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "golden")]
import nrs  # noqa: E402
from make_track5k_golden import make_inputs, N_POINTS, CASES  # noqa: E402


def timed(fn, reps, warm, before=None):
    ms, out = [], None
    for k in range(warm + reps):
        if before:
            before()
        t0 = time.perf_counter()
        out = fn()
        if k >= warm:
            ms.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(ms)), 4), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = N_POINTS
    _, model, seed = CASES[0]
    tp, hist, upd, _ = make_inputs(n, seed, model)
    cam = nrs.make_camera(tp["model"], tp["prm"])
    ids = np.arange(n, dtype=np.int32)
    dup = np.concatenate([upd, upd[:1]]).astype(np.int32)
    assert 4 * len(upd) >= n and 8 * n >= n >= 512
    ctx = nrs.Context()
    g = nrs.RGraph(ctx, n, tp["graph"]["sigma"], tp["graph"]["stretch_th"])
    med, digest = {}, hashlib.sha256()

    def put_back():
        g.add_edges(tp["X_prev"], ids, ids)
        g.update(hist, upd)

    med["add_edges"], _ = timed(lambda: g.add_edges(tp["X_prev"], ids, ids), a.reps, a.warm)
    med["update_one_pass"], good = timed(lambda: g.update(hist, upd), a.reps, a.warm)
    digest.update(good.tobytes())
    med["update_per_vertex"], good = timed(lambda: g.update(hist, dup), a.reps, a.warm)
    digest.update(good.tobytes())
    for leg, switch in (("get_edges_mirror", None), ("get_edges_triangle", 1)):
        nrs.debug_set("NRS_RG_NO_MIRROR", switch)
        try:
            med[leg], lists = timed(lambda: g.get_edges(ids, 128), a.reps, a.warm)
        finally:
            nrs.debug_set("NRS_RG_NO_MIRROR", None)
        cnt = lists[0]
        digest.update(cnt.tobytes())
        keep = np.arange(128)[None, :] < np.minimum(cnt, 128)[:, None]      # the returned prefixes
        for x in lists[1:]:
            digest.update(np.where(keep, x, 0).tobytes())

    def frame():
        return ctx.track_deform_solve_rg(cam, g, tp["X_prev"], ids, tp["status"], tp["uv"], tp["X_prev"], tp["pose_q"], tp["pose_t"], tp["scale"], None, 128)

    med["a2_frame"], r = timed(frame, a.reps, a.warm, before=put_back)
    for k in ("pose_q", "pose_t", "f_pos", "f_status", "map_pos"):
        digest.update(np.ascontiguousarray(r[k]).tobytes())
    digest.update(g.rows(ids[::97])[3].tobytes())
    line = dict(device=ctx.device_name(), library=os.path.basename(os.path.dirname(nrs.LIB_PATH)) + "/" + os.path.basename(nrs.LIB_PATH), n_points=n, reps=a.reps,
                warm=a.warm, lost=len(r["lost"]), median_ms=med, digest=digest.hexdigest()[:16])
    g.close()
    ctx.close()
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
