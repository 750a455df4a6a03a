"""Times one nrs_map_frame call against nrs_triangulate_batch alone on the same buffer (the deformable leg: the floor of the call) at
~350 ids x 12 snapshots and ~5k ids x 21.  Medians of a handful of calls after a warm-up; wall clock around the synchronous calls.
    python tools/map_frame_probe.py [--reps 7] [--out profiles/map_frame_probe.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nr-slam_amd", "py"), os.path.join(ROOT, "oracle")]
import nrs  # noqa: E402
import nrs_synth as S  # noqa: E402


def median_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = nrs.Context()
    lines = ["device: %s" % ctx.device_name()]
    for label, kw in (("350 ids x 12", dict(n_frames=12, seed=3)), ("5k ids x 21", dict(n_frames=21, seed=3, spacing=6.6, cand_frac=0.97))):
        tb = S.make_mapping_buffer(**kw)
        cam = nrs.make_camera(tb["model"], tb["prm"])
        cand = np.nonzero(tb["status"] == 1)[0].astype(np.int32)
        r = ctx.map_frame(cam, tb, tb["deform_mag"], tb["rad_per_pixel"])
        m = median_ms(lambda: ctx.map_frame(cam, tb, tb["deform_mag"], tb["rad_per_pixel"]), a.reps)
        t = median_ms(lambda: ctx.triangulate_batch(cam, tb, cand, 5), a.reps)
        lines.append("%-14s ids %5d candidates %5d rigid ok %4d deformable ok %4d mode %d | map_frame %.3f ms (min %.3f max %.3f) | "
                     "triangulate_batch %.3f ms (min %.3f max %.3f) | difference %.3f ms"
                     % (label, tb["has_kp"].shape[1], len(cand), r["n_rigid"], r["n_deformable"], r["mode"], *m, *t, m[0] - t[0]))
    ctx.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
