"""Timing probe of the stereo pattern matcher (include/nrs.h nrs_stereo_match_pattern; DESIGN.md 4 "Evaluation (f7)") at 640 x 480 with
1000 keypoints: ms per call of the matrix-core form and of the plain form (NRS_STEREO_NO_MFMA=1), the share of the int8 matrix peak the
first reaches, and the time of the NumPy restatement (tests/eval_oracle.py) on a reduced keypoint count.

Clock: time.perf_counter around the call, which uploads both images, runs its five launches and ends in a stream synchronise.  Warm-up
rounds first, then the two forms alternate inside one loop; medians and the 10th / 90th percentiles over --reps rounds.  The share of
the peak counts the padded GEMM (2 * positions * keypoints * 256 operations) against --peak-tops (default 5000: twice the bf16 dense
peak of an MI355X) -- a whole-call figure, uploads included.  One JSON line to stdout and to --out.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "nr-slam_amd", "py"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import nrs                      # noqa: E402
import nrs_synth as S           # noqa: E402
import eval_oracle as E         # noqa: E402


def stats(ts):
    a = np.asarray(ts) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wh", default="640x480")
    ap.add_argument("--keypoints", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--oracle-keypoints", type=int, default=4)
    ap.add_argument("--peak-tops", type=float, default=5000.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = (int(v) for v in a.wh.split("x"))
    p = S.make_stereo_pair((w, h), 3, (9, 0, 4, 17), a.keypoints)
    xy = p["xy"]
    prm = np.array([383.19, 383.05, w / 2.0, h / 2.0], np.float32)
    cam = nrs.make_camera(0, prm)
    ctx = nrs.Context()
    forms = (("mfma", None), ("plain", "1"))
    res, t = {}, {k: [] for k, _ in forms}
    for r in range(a.warmup + a.reps):
        for name, sw in forms:
            ctx.debug_set("NRS_STEREO_NO_MFMA", sw)
            t0 = time.perf_counter()
            out = ctx.stereo_match_pattern(cam, 2000.0, p["left"], p["right"], xy)
            dt = time.perf_counter() - t0
            if r >= a.warmup:
                t[name].append(dt)
            res[name] = out
    ctx.close()
    same = all(x.tobytes() == y.tobytes() for x, y in zip(res["mfma"], res["plain"]))
    k = min(a.oracle_keypoints, len(xy))
    t0 = time.perf_counter()
    ora = E.stereo_match_pattern(prm, 2000.0, p["left"], p["right"], xy[:k])
    t_ora = time.perf_counter() - t0
    agree = all(np.array_equal(x[:k], y, equal_nan=True) for x, y in zip(res["mfma"], ora))
    Wr, Hr = E.search_dims(w, h)
    ops = 2.0 * Wr * Hr * len(xy) * 256
    rec = dict(probe="stereo_probe", wh=[w, h], keypoints=len(xy), positions=Wr * Hr, reps=a.reps, mfma=stats(t["mfma"]), plain=stats(t["plain"]),
               forms_identical=bool(same), oracle_agrees=bool(agree), gemm_tera_ops=round(ops / 1e12, 4),
               int8_peak_share=round(ops / (np.median(t["mfma"]) * a.peak_tops * 1e12), 5), peak_tops=a.peak_tops,
               numpy_oracle=dict(keypoints=k, seconds=round(t_ora, 3)), status_counts=np.bincount(res["mfma"][1], minlength=8).tolist())
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
