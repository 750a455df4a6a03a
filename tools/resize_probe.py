"""Timing probe of the frame resize on the device (include/nrs.h nrs_front_process_raw; DESIGN.md 4 "Frame resize").

At the two HD shapes a caller of the Endomapper app's path meets -- 1440 x 1080 -> 720 x 540 and 1920 x 1080 -> 960 x 540, three
channels, both the box branch -- and, for the general branch, at 1441 x 1081 -> 720 x 540, per call, nothing downloaded:

  (a) nrs_front_process_raw on the raw frame, fused (the default) and with NRS_RESIZE_OWN_LAUNCH=1
  (b) nrs_front_process on the already-resized frame: the FLOOR.  (a) - (b) is what the device resize and the four times larger upload cost

The host cv::resize that (a) replaces is not timed: there is no OpenCV here, so no speed-up is claimed.

Clock: time.perf_counter around calls that end in a stream synchronise (every entry point here does).  `--warmup` rounds, then the three
forms alternate inside one loop; medians and the 10th / 90th percentiles over `--reps` rounds.  Writes one JSON line per shape to stdout
and appends them to --out.  Needs a GPU: there is no fallback."""
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
import resize_oracle as RO      # noqa: E402

SHAPES = (((1440, 1080), (720, 540)), ((1920, 1080), (960, 540)), ((1441, 1081), (720, 540)))


def stats(ts):
    a = np.asarray(ts) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4))


def probe(src, dst, reps, warm):
    (sw, sh), (dw, dh) = src, dst
    rng = np.random.default_rng(5)
    raw = np.ascontiguousarray(np.repeat(np.clip(np.rint(S._texture(sh, sw, rng, 0)), 0, 254).astype(np.uint8)[:, :, None], 3, 2))
    raw[:, :, 1] = raw[:, ::-1, 0]                                 # (the channels differ)
    small = np.ascontiguousarray(RO.resize(raw, dw, dh))          # (packed: the binding would otherwise copy it on every call)
    ctx, base = nrs.Context(), nrs.Context()
    ctx.front_resize_configure(src, dst)
    out = ctx.front_process_raw(raw, outputs=("resized", "gray"))
    assert np.array_equal(out["resized"], small)                   # the three forms do the same work
    assert np.array_equal(out["gray"], base.front_process(small, outputs=("gray",))["gray"])
    t_fused, t_own, t_base = [], [], []
    for r in range(warm + reps):
        ctx.debug_set("NRS_RESIZE_OWN_LAUNCH", None)
        t0 = time.perf_counter()
        ctx.front_process_raw(raw, outputs=False)
        t1 = time.perf_counter()
        ctx.debug_set("NRS_RESIZE_OWN_LAUNCH", "1")
        t2 = time.perf_counter()
        ctx.front_process_raw(raw, outputs=False)
        t3 = time.perf_counter()
        base.front_process(small, outputs=False)
        t4 = time.perf_counter()
        if r >= warm:
            t_fused.append(t1 - t0); t_own.append(t3 - t2); t_base.append(t4 - t3)
    box = ctx.front_resize_taps()["box"]
    ctx.close()
    base.close()
    a, o, b = stats(t_fused), stats(t_own), stats(t_base)
    return dict(raw="%dx%d" % src, resized="%dx%d" % dst, channels=3, branch="box" if box else "general", reps=reps, warmup=warm,
                clock="time.perf_counter around synchronous calls", upload_bytes_raw=sw * sh * 3, upload_bytes_resized=dw * dh * 3,
                a_raw_fused=a, a_raw_own_launch=o, b_resized_frame_floor=b,
                fused_minus_floor_median_ms=round(a["median_ms"] - b["median_ms"], 4), own_minus_fused_median_ms=round(o["median_ms"] - a["median_ms"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))), help="indices into SHAPES, in the order to run them")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_probe.jsonl"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for src, dst in (SHAPES[i] for i in a.shapes):
        line = json.dumps(probe(src, dst, a.reps, a.warmup))
        print(line, flush=True)
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
