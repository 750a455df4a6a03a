"""Timing probe of the stereo map initialisation (include/nrs.h f8; DESIGN.md section 4 "Stereo map initialisation").

nrs_init_stereo at 640 x 480 on nrs_synth.make_stereo_init_sequence, with the keypoints the extractor (nrs_shi_extract) leaves on the left
image -- all of them, no thinning -- and nrs_dbscan3d alone on the gated points.

Clock: time.perf_counter around the call, which ends in a stream synchronise.  5 warm-up calls, then medians and the 10th / 90th
percentiles over --reps calls.  Writes one JSON line per setting to stdout and to --out.  Needs a GPU: there is no fallback.

--resident: the stereo pair held on the device (nrs_front_process_stereo, nrs_init_stereo_front) against the host path it replaces; see
resident() below."""
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


def baseline_context(path):
    """a Context on ANOTHER build of the library (--baseline-lib: the parent commit's, which has no resident-pair entry points), loaded
    next to this one; only the calls the baseline legs make are used on it"""
    import ctypes as C
    c = nrs.Context.__new__(nrs.Context)
    c.lib = C.CDLL(path)
    c.lib.nrs_last_error.restype = C.c_char_p
    c.lib.nrs_destroy.restype = None
    opt = nrs.Options(-1, C.sizeof(nrs.Options), 0.0, 0, 0, 0, 0, 0, 0, 0)
    c.h = C.c_void_p()
    rc = c.lib.nrs_create(C.byref(c.h), C.byref(opt))
    if rc != nrs.OK:
        raise nrs.NrsError(rc, "nrs_create on %s" % path)
    return c


def resident(a):
    """--resident: the stereo pair held on the device (include/nrs.h nrs_front_process_stereo) against the path it replaces, 640 x 480 x 3.
      (a) front end     nrs_front_process_stereo (pair launches; and with NRS_FRONT_PER_EYE) against two nrs_front_process calls
      (b) start         nrs_front_process_stereo + nrs_init_stereo_front against two nrs_front_process calls with the grey bytes
                        downloaded + nrs_init_stereo on them
    The variants ALTERNATE inside every repetition; the whole measurement is repeated --rounds times and every round's median is
    reported, so that the run-to-run spread stands next to the differences.  Nothing but what a leg needs is downloaded."""
    sq = S.make_stereo_init_sequence(n_points=2000, wh=(640, 480), bf=4800.0)
    left = np.ascontiguousarray(np.repeat(sq["images"][0][:, :, None], 3, 2))
    right = np.ascontiguousarray(np.repeat(sq["right"][:, :, None], 3, 2))
    ctx = nrs.Context()
    base = baseline_context(a.baseline_lib) if a.baseline_lib else ctx
    cam = nrs.make_camera(sq["model"], sq["prm"])
    xy = np.asarray(ctx.shi_extract(sq["images"][0], None, None)[0], np.float32).reshape(-1, 2)
    opts = dict(bf=sq["bf"], z_min=sq["z_min"], z_max=sq["z_max"], eps=sq["eps"], min_points=sq["min_points"])

    def pair(per_eye):
        ctx.debug_set("NRS_FRONT_PER_EYE", per_eye)
        ctx.front_process_stereo(left, right, outputs=False)

    def two_calls():
        base.front_process(left, outputs=False)
        base.front_process(right, outputs=False)

    def start_resident():
        ctx.debug_set("NRS_FRONT_PER_EYE", None)
        ctx.front_process_stereo(left, right, outputs=False)
        return ctx.init_stereo_front(cam, xy, **opts)

    def start_host():
        gl = base.front_process(left, outputs=("gray",))["gray"]
        gr = base.front_process(right, outputs=("gray",))["gray"]
        return base.init_stereo(cam, gl, gr, xy, **opts)

    legs = [("front_pair", lambda: pair(None)), ("front_per_eye", lambda: pair("1")), ("front_two_calls", two_calls),
            ("start_resident", start_resident), ("start_host", start_host)]
    ra, rb = start_resident(), start_host()
    assert all(np.array_equal(np.asarray(ra[k]), np.asarray(rb[k]), equal_nan=True) for k in ra), "the two starts differ"
    lines, order = [], np.random.default_rng(1)
    for rnd in range(a.rounds):
        ts = {name: [] for name, _ in legs}
        behind_start = {name: [] for name, _ in legs[:3]}          # a front-end leg's calls that came right behind a start_* leg
        prev = ""
        for i in range(a.warmup + a.reps):
            for k in order.permutation(len(legs)):                 # (shuffled: a call pays for the allocations the one before it has just
                name, fn = legs[k]                                 # freed, so no leg may always follow the same one)
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if i >= a.warmup:
                    (behind_start if prev.startswith("start_") and name in behind_start else ts)[name].append(dt)
                prev = name
        rec = dict(wh=[640, 480], channels=3, n_keypoints=len(xy), n_selected=int(ra["n_selected"]), round=rnd, reps=a.reps, warmup=a.warmup,
                   clock="time.perf_counter around the synchronous calls, variants alternating inside a repetition in a shuffled order; "
                         "front_* legs: calls right behind a start_* leg are reported apart (behind_start)",
                   baseline="another build of the library (--baseline-lib)" if a.baseline_lib else "this library")
        rec.update({name: stats(v) for name, v in ts.items()})
        rec["behind_start"] = {name: dict(stats(v), calls=len(v)) for name, v in behind_start.items() if v}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    ctx.close()
    if base is not ctx:
        base.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resident", action="store_true", help="time the resident stereo pair against the host path it replaces")
    ap.add_argument("--rounds", type=int, default=3, help="--resident: repetitions of the whole measurement")
    ap.add_argument("--baseline-lib", default=None, help="--resident: a libnrs_hip.so of another build for the host-path legs")
    a = ap.parse_args()
    if a.resident:
        lines = resident(a)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return
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
