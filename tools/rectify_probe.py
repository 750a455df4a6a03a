"""Timing probe of the stereo rectification on the device (include/nrs.h nrs_front_process_stereo_raw; DESIGN.md 4 "Stereo rectification").

At the Hamlyn loader's shape -- raw eyes of 720 x 288, rectified eyes of 720 x 515, three channels -- with a designed camera whose
distortion has the magnitude of that dataset's calibrations (k1 about -0.3, k2 about 0.1, tangential terms of 1e-3) and a rectifying
rotation of a few hundredths of a radian per eye (no dataset's numbers), per call, nothing downloaded:

  (a) nrs_front_process_stereo_raw on the raw pair, fused (the default) and with NRS_RECT_OWN_LAUNCH=1
  (b) nrs_front_process_stereo on the pre-rectified pair: the code path as it was before the rectification existed, the BASELINE
  (c) (b) plus tests/rect_oracle.py's NumPy remap of both eyes: what a caller who rectifies on the host pays (a caller with OpenCV pays
      less for the remap than NumPy does: (c) is an upper bound of that cost, (b) its lower bound)

Clock: time.perf_counter around calls that end in a stream synchronise (every entry point here does).  `--warmup` rounds, then the three
device forms alternate inside one loop; medians and the 10th / 90th percentiles over `--reps` rounds; the NumPy remap is timed over
`--host-reps` rounds of its own.  Writes one JSON line to stdout and appends it to --out.  Needs a GPU: there is no fallback."""
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
import rect_cases as RC         # noqa: E402
import rect_oracle as RO        # noqa: E402

SRC, DST = (720, 288), (720, 515)


def camera():
    """both eyes: a 720 x 288 camera with barrel distortion, turned a little, into a 720 x 515 rectified frame"""
    P = RC.cam(400, 360, 257)
    left = RC.eye(RC.cam(390, 355, 150, 195), P, RC.rot(0.01, -0.02, 0.004), (-0.3, 0.1, 0.001, -0.0015))
    right = RC.eye(RC.cam(392, 362, 147, 196), P, RC.rot(-0.008, 0.015, -0.003), (-0.28, 0.09, -0.0012, 0.001))
    return left, right


def stats(ts):
    a = np.asarray(ts) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4))


def probe(reps, warm, host_reps):
    (sw, sh), (dw, dh) = SRC, DST
    rng = np.random.default_rng(5)
    raws = [np.ascontiguousarray(np.repeat(np.clip(np.rint(S._texture(sh, sw, rng, 0)), 0, 254).astype(np.uint8)[:, :, None], 3, 2)) for _ in range(2)]
    left, right = camera()
    maps = [RO.build_map(e, dw, dh) for e in (left, right)]
    rect = [RO.remap(r, *m) for r, m in zip(raws, maps)]
    ctx, base = nrs.Context(), nrs.Context()
    ctx.front_rectify_configure(SRC, DST, left, right)
    out = ctx.front_process_stereo_raw(raws[0], raws[1], outputs=("rect_left", "rect_right", "gray"))
    assert np.array_equal(out["rect_left"], rect[0]) and np.array_equal(out["rect_right"], rect[1])      # the three forms do the same work
    assert np.array_equal(out["gray"], base.front_process_stereo(rect[0], rect[1], outputs=("gray",))["gray"])
    inside = float((RO.taps_outside(*maps[0], sw, sh) == 0).mean())
    t_fused, t_own, t_base = [], [], []
    for r in range(warm + reps):
        ctx.debug_set("NRS_RECT_OWN_LAUNCH", None)
        t0 = time.perf_counter()
        ctx.front_process_stereo_raw(raws[0], raws[1], outputs=False)
        t1 = time.perf_counter()
        ctx.debug_set("NRS_RECT_OWN_LAUNCH", "1")
        t2 = time.perf_counter()
        ctx.front_process_stereo_raw(raws[0], raws[1], outputs=False)
        t3 = time.perf_counter()
        base.front_process_stereo(rect[0], rect[1], outputs=False)
        t4 = time.perf_counter()
        if r >= warm:
            t_fused.append(t1 - t0); t_own.append(t3 - t2); t_base.append(t4 - t3)
    t_host = []
    for r in range(host_reps):
        t0 = time.perf_counter()
        RO.remap(raws[0], *maps[0]); RO.remap(raws[1], *maps[1])
        t_host.append(time.perf_counter() - t0)
    ctx.close()
    base.close()
    b, hst = stats(t_base), stats(t_host)
    return dict(raw="%dx%d" % SRC, rectified="%dx%d" % DST, channels=3, reps=reps, warmup=warm, host_reps=host_reps,
                clock="time.perf_counter around synchronous calls", fully_inside_fraction=round(inside, 3),
                upload_bytes_raw_pair=2 * sw * sh * 3, upload_bytes_rectified_pair=2 * dw * dh * 3,
                a_raw_fused=stats(t_fused), a_raw_own_launch=stats(t_own), b_prerectified_pair_baseline=b, numpy_remap_both_eyes_cpu=hst,
                c_baseline_plus_numpy_remap_median_ms=round(b["median_ms"] + hst["median_ms"], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_probe.jsonl"))
    a = ap.parse_args()
    line = json.dumps(probe(a.reps, a.warmup, a.host_reps))
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
