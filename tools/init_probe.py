"""Timing probe of the monocular map initialisation (include/nrs.h f6; DESIGN.md section 4 "map initialisation").

nrs_init_essential at n = 4000 keypoints (the reference's max_features; 10 % outliers, 5 % untracked) for n_hypotheses 16 / 256 / 4096,
the library's sampler, no parity taps downloaded by the caller; against tests/init_oracle.py (NumPy, one CPU core) at 16 hypotheses.

Clock: time.perf_counter around the call, which ends in a stream synchronise.  5 warm-up calls, then medians and the 10th / 90th
percentiles over --reps calls per setting.  Writes one JSON line per setting to stdout and to --out.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "nr-slam_amd", "py"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import nrs                      # noqa: E402
import nrs_synth as S           # noqa: E402
import init_oracle as IO        # noqa: E402


def stats(ts):
    a = np.asarray(ts) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    p = S.make_init_pair(n=4000, seed=6, outlier_frac=0.1, untracked_frac=0.05)
    rpp = 1.0 / float(p["prm"][0])
    ctx = nrs.Context()
    cam = nrs.make_camera(p["model"], p["prm"])
    lines = []
    for nh in (16, 256, 4096):
        ts, r = [], None
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            r = ctx.init_essential(cam, p["ref_xy"], p["cur_xy"], p["status"], p["n_matches"], taps=False, n_hypotheses=nh, radians_per_pixel=rpp)
            if i >= a.warmup:
                ts.append(time.perf_counter() - t0)
        lines.append(json.dumps(dict(n=4000, n_hypotheses=nh, verdict=r["verdict"], score=r["score"], reps=a.reps, warmup=a.warmup,
                                     clock="time.perf_counter around the synchronous call", nrs_init_essential=stats(ts))))
        print(lines[-1], flush=True)
    ctx.close()
    t0 = time.perf_counter()
    o = IO.initialize(p["model"], p["prm"], p["ref_xy"], p["cur_xy"], p["status"], p["n_matches"], n_hypotheses=16, radians_per_pixel=np.float32(rpp))
    lines.append(json.dumps(dict(n=4000, n_hypotheses=16, verdict=int(o["verdict"]), numpy_restatement_cpu_ms=round((time.perf_counter() - t0) * 1e3, 1), runs=1)))
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
