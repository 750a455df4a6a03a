"""Timing probe of the flow-track clustering (include/nrs.h f6 nrs_flow_tracks_cluster; DESIGN.md section 4 "Flow-track clustering").

nrs_flow_tracks_cluster at n = 1k / 4k / 16k tracks x L = 11 / 31 keypoints, on both forms of the neighbour stage: the LDS tiles (the
default) and a wave per point (NRS_DBND_NO_TILE).  The tracks are two motions and a share of wanderers, as in tests/flow_cluster_cases.py.
The two forms must return the same labels, or the probe stops.

Clock: time.perf_counter around the synchronous call (upload, launches, download, stream synchronise), one process.  2 warm-up calls, then
the median of 7 calls, the forms alternating call by call.  --budget seconds of wall clock for the whole run: a setting that would start
past it is written as skipped, not measured (run it under `timeout` as well).  Writes one JSON line per setting to stdout and to --out.
Needs a GPU: there is no fallback."""
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

SWITCH = "NRS_DBND_NO_TILE"


def make_tracks(n, length, seed):
    rng = np.random.default_rng(seed)
    step = np.zeros((n, length - 1, 2))
    a, b = int(0.4 * n), int(0.8 * n)
    step[:a] = (0.8, 0.1)
    step[a:b] = (-0.5, 0.6)
    step[:b] += rng.uniform(-0.05, 0.05, (b, length - 1, 2))
    step[b:] = rng.uniform(-3, 3, (n - b, length - 1, 2))
    start = rng.uniform([100, 100], [540, 380], (n, 2))
    xy = np.concatenate([start[:, None, :], start[:, None, :] + np.cumsum(step, 1)], 1)
    return np.ascontiguousarray(xy[rng.permutation(n)], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1024,4096,16384")
    ap.add_argument("--lengths", default="11,31")
    ap.add_argument("--budget", type=float, default=240.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_cluster_probe.jsonl"))
    a = ap.parse_args()
    t_start = time.perf_counter()
    ctx = nrs.Context()
    lines = []
    for n in [int(v) for v in a.sizes.split(",")]:
        for length in [int(v) for v in a.lengths.split(",")]:
            rec = dict(n_tracks=n, length=length, dim=2 * (length - 1), reps=a.reps, warmup=a.warmup, device=ctx.device_name(),
                       clock="time.perf_counter around the synchronous call, the two forms alternating")
            if time.perf_counter() - t_start > a.budget:
                rec["skipped"] = "the run's budget of %g s was spent" % a.budget
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
                continue
            tracks = make_tracks(n, length, 100 + length)
            ts = {"tiles": [], "plain": []}
            out = {}
            for i in range(a.warmup + a.reps):
                for form in ("tiles", "plain"):
                    ctx.debug_set(SWITCH, "1" if form == "plain" else None)
                    t0 = time.perf_counter()
                    out[form] = ctx.flow_tracks_cluster(tracks, flows=False)
                    if i >= a.warmup:
                        ts[form].append(time.perf_counter() - t0)
            ctx.debug_set(SWITCH, None)
            if not (np.array_equal(out["tiles"][0], out["plain"][0]) and np.array_equal(out["tiles"][1], out["plain"][1])):
                raise SystemExit("the two forms differ at n = %d, L = %d" % (n, length))
            rec.update(clusters=int(out["tiles"][1][0]), noise=int(out["tiles"][1][1]))
            for form, v in ts.items():
                ms = np.asarray(v) * 1e3
                rec[form] = dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(ms.min()), 4), max_ms=round(float(ms.max()), 4))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
