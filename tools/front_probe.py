"""Timing probe of the image front end (include/nrs.h f5).

Per frame size -- 640x480 and 736x552 (the endomapper frames; data/endomapper/settings.yaml itself carries no size, 736x552 is the
size nrs_synth uses for that calibration: principal point x 2, rounded to the CLAHE grid) -- with the filter set of
data/endomapper/filters.txt ("BrightFilter 225" + a predefined mask):

  (a) nrs_front_process, every output downloaded
  (b) a keyframe frame, resident:  nrs_front_process without outputs + nrs_klt_track_front + nrs_shi_extract_front +
      nrs_klt_set_reference_front          against
      the same frame through the host-pointer entry points (nrs_klt_track, nrs_shi_extract, nrs_klt_set_reference; unchanged by the
      front end) fed host-made grey image and Global mask -- the time of making those on the host is (c), reported separately
  (c) tests/front_oracle.py (NumPy) on the CPU: grey + CLAHE + masks of one frame

Clock: time.perf_counter around calls that end in a stream synchronise (every entry point here does).  5 warm-up rounds, then the
two forms of (b) alternate inside one loop; medians and the 10th / 90th percentiles over `--reps` rounds.  Writes one JSON line per
size to stdout and to --out.  Needs a GPU: there is no fallback."""
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
import front_oracle as FO       # noqa: E402


def frame(w, h, seed):
    rng = np.random.default_rng(seed)
    g = np.clip(np.rint(S._texture(h, w, rng, 0)), 0, 254).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for cy, cx, r in ((h // 3, w // 2, h // 10), (2 * h // 3, w // 4, h // 14)):
        g[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 255                  # specular highlights
    disk = np.where(((yy - h / 2) / (0.56 * h)) ** 2 + ((xx - w / 2) / (0.56 * w)) ** 2 <= 1.0, 255, 0).astype(np.uint8)
    g[disk == 0] = 0                                                       # the endoscope's black corners
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2)), disk


def stats(ts):
    a = np.asarray(ts) * 1e3
    return dict(median_ms=round(float(np.median(a)), 4), p10_ms=round(float(np.percentile(a, 10)), 4), p90_ms=round(float(np.percentile(a, 90)), 4))


def probe(w, h, reps, warm):
    img, disk = frame(w, h, 3)
    img2 = np.ascontiguousarray(np.roll(img, (2, 3), (0, 1)))
    filters = [("bright", 225), ("predefined", disk)]
    dev, host = nrs.Context(), nrs.Context()
    for c in (dev, host):
        c.klt_configure()
        c.shi_configure(5)
    dev.front_configure(filters)
    o = dev.front_process(img)
    pts = host.shi_extract(o["clahe"], None, o["global"])[0]
    dev.shi_extract_front(None, nrs.FRONT_CLAHE, True)
    o2 = dev.front_process(img2)
    t_a, t_res, t_host = [], [], []
    st0 = np.zeros(len(pts), np.int32)
    for r in range(warm + reps):
        dev.front_process(img)
        dev.klt_set_reference_front(pts, nrs.FRONT_GRAY, True)
        host.klt_set_reference(o["gray"], pts, o["global"])
        t0 = time.perf_counter()
        dev.front_process(img2)
        t1 = time.perf_counter()
        # (b) resident: one upload, three hand-overs
        dev.front_process(img2, outputs=False)
        xy, st, _, _ = dev.klt_track_front(pts, st0, nrs.FRONT_GRAY)
        held = xy[st == 0]
        dev.shi_extract_front(held, nrs.FRONT_GRAY, True)
        dev.klt_set_reference_front(held, nrs.FRONT_GRAY, True)
        t2 = time.perf_counter()
        # (b) host pointers: three uploads of the image, two of the mask (the inputs exist already: (c) is what making them costs)
        xy, st, _, _ = host.klt_track(o2["gray"], pts, st0)
        held = xy[st == 0]
        host.shi_extract(o2["gray"], held, o2["global"])
        host.klt_set_reference(o2["gray"], held, o2["global"])
        t3 = time.perf_counter()
        if r >= warm:
            t_a.append(t1 - t0); t_res.append(t2 - t1); t_host.append(t3 - t2)
    dev.close(); host.close()
    t_c = []
    of = [(FO.BRIGHT, 225), (FO.PREDEFINED, disk)]
    for r in range(3):
        t0 = time.perf_counter()
        FO.front_process(img2, of)
        t_c.append(time.perf_counter() - t0)
    return dict(size="%dx%d" % (w, h), n_points=int(len(pts)), reps=reps, warmup=warm, clock="time.perf_counter around synchronous calls",
                a_front_process_all_outputs=stats(t_a), b_resident_keyframe_frame=stats(t_res), b_host_pointer_keyframe_frame=stats(t_host),
                c_numpy_restatement_cpu=stats(t_c))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [json.dumps(probe(w, h, a.reps, a.warmup)) for w, h in ((640, 480), (736, 552))]
    for line in lines:
        print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
