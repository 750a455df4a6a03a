"""Timing probe of the stereo map initialisation (include/nrs.h f8; DESIGN.md section 4 "Stereo map initialisation").

nrs_init_stereo at 640 x 480 on nrs_synth.make_stereo_init_sequence, with the keypoints the extractor (nrs_shi_extract) leaves on the left
image -- all of them, no thinning -- and nrs_dbscan3d alone on the gated points.

Clock: time.perf_counter around the call, which ends in a stream synchronise.  5 warm-up calls, then medians and the 10th / 90th
percentiles over --reps calls.  Writes one JSON line per setting to stdout and to --out.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "nr-slam_amd", "py"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import nrs                      # noqa: E402
import nrs_synth as S           # noqa: E402


def stats(ts):
    a = np.asarray(ts) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4))


def timed(fn, warmup, reps):
    ts, r = [], None
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        r = fn()
        if i >= warmup:
            ts.append(time.perf_counter() - t0)
    return ts, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sq = S.make_stereo_init_sequence(n_points=2000, wh=(640, 480), bf=4800.0)      # the same disparities in pixels per mm of depth as at 320 x 240
    ctx = nrs.Context()
    cam = nrs.make_camera(sq["model"], sq["prm"])
    xy, _, _ = ctx.shi_extract(sq["images"][0], None, None)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    opts = dict(bf=sq["bf"], z_min=sq["z_min"], z_max=sq["z_max"], eps=sq["eps"], min_points=sq["min_points"])
    lines = []
    ts, r = timed(lambda: ctx.init_stereo(cam, sq["images"][0], sq["right"], xy, **opts), a.warmup, a.reps)
    lines.append(json.dumps(dict(wh=[640, 480], n_keypoints=len(xy), n_matched=r["n_matched"], n_gated=r["n_gated"], n_clusters=r["n_clusters"],
                                 n_selected=r["n_selected"], reps=a.reps, warmup=a.warmup,
                                 clock="time.perf_counter around the synchronous call", nrs_init_stereo=stats(ts))))
    print(lines[-1], flush=True)
    gated = r["xyz"][r["code"] != 1][r["code"][r["code"] != 1] != 2]
    ts, d = timed(lambda: ctx.dbscan3d(gated, sq["eps"], sq["min_points"], True), a.warmup, a.reps)
    lines.append(json.dumps(dict(n_points=len(gated), clusters=int(d[2][0]), reps=a.reps, warmup=a.warmup, nrs_dbscan3d=stats(ts))))
    print(lines[-1], flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
