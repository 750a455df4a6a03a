"""What feeding frame mapping costs per frame, host buffer against resident buffer, at the tracked-fps size: 4446 keypoint ids, 21 snapshots.

Two paths, alternating frame by frame in one process on one context, both buffers full (every insert pops):
  host      nrs_frame_loop.TemporalBuffer.insert + .flat (the dense table rebuilt in NumPy) + nrs_map_frame (six pageable uploads)
  resident  nrs_tbuf_insert (one pinned upload of the frame) + nrs_map_frame_tbuf (the table rebuilt on the device)
The mapping kernels are the same launches on the same tables in both, so their time cancels; the buffer is make_mapping_buffer's at 6.6 px
spacing cut to 4446 ids, a tenth of them 2D-only tracks (the candidates): at that density most candidates leave at the close-features
test, so the kernels are short and the figures are about the feed, which is the subject.

Pass 1: wall clock around the calls, medians after a warm-up.  Pass 2: the same frames under NRS_TIMING=1 (the library waits for the
stream at every mark, so its sum is above pass 1's wall clock): the library's stages (upload / flatten / mapping kernels / download)
read from its stderr lines, next to the Python-side stages (insert, flat).  One JSON line per path and pass.
    python tools/tbuf_probe.py [--reps 40] [--warm 8] [--out profiles/tbuf_probe.jsonl]"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "nr-slam_amd", "py"), os.path.join(ROOT, "oracle")]
import nrs  # noqa: E402
import nrs_frame_loop as FL  # noqa: E402
import nrs_synth as S  # noqa: E402

N_IDS, N_SNAPS = 4446, 21


def frames_of(tb):
    """the buffer's snapshots as frames to insert, cycled: slots unfiltered, ids = rows"""
    out = []
    for f in range(tb["n_frames"]):
        rows = np.nonzero(tb["has_kp"][f])[0]
        out.append(dict(ids=rows.astype(np.int64), xy=tb["kp_xy"][f, rows].copy(), pos=tb["lm_xyz"][f, rows].copy(),
                        status=np.where(tb["has_lm"][f, rows], 0, 1).astype(np.int32), pose=tb["poses"][f].copy(), mag=tb["deform_mag"][f]))
    return out


def med(v):
    return round(float(np.median(v)), 4) if len(v) else None


def run(ctx, cam, tb, frames, rpp, reps, warm, timing):
    host, res = FL.TemporalBuffer(20), nrs.TBuf(ctx, 20)
    t = dict(host=dict(insert=[], flat=[], call=[], total=[]), resident=dict(insert=[], call=[], total=[]))
    same = True
    for k in range(N_SNAPS + warm + reps):
        s = frames[k % len(frames)]
        rec = k >= N_SNAPS + warm
        # host path
        t0 = time.perf_counter()
        host.insert(s["ids"], s["xy"], s["pos"], s["status"], s["pose"][:4], s["pose"][4:], s["mag"])
        t1 = time.perf_counter()
        flat, mag, ids = host.flat(tb["model"], tb["prm"])
        t2 = time.perf_counter()
        rh = ctx.map_frame(cam, flat, mag, rpp)
        t3 = time.perf_counter()
        # resident path
        res.insert(s["ids"], s["xy"], s["pos"], s["status"], s["pose"], s["mag"])
        t4 = time.perf_counter()
        rr = res.map_frame(cam, rpp)
        t5 = time.perf_counter()
        same = same and np.array_equal(ids[rh["cand"]], rr["cand"]) and np.array_equal(ids[rh["accepted_ids"]], rr["accepted_ids"]) and \
            rh["accepted_xyz"].tobytes() == rr["accepted_xyz"].tobytes() and rh["mode"] == rr["mode"]
        if rec:
            for name, v in (("insert", t1 - t0), ("flat", t2 - t1), ("call", t3 - t2), ("total", t3 - t0)):
                t["host"][name].append(1e3 * v)
            for name, v in (("insert", t4 - t3), ("call", t5 - t4), ("total", t5 - t3)):
                t["resident"][name].append(1e3 * v)
    info = res.info()
    res.close()
    return t, same, info, len(rr["cand"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warm", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tb = S.make_mapping_buffer(n_frames=N_SNAPS, seed=3, spacing=6.6, cand_frac=0.1)
    assert tb["has_kp"].shape[1] >= N_IDS
    for k in ("has_kp", "has_lm", "status"):
        tb[k] = np.ascontiguousarray(tb[k][..., :N_IDS])
    for k in ("kp_xy", "lm_xyz"):
        tb[k] = np.ascontiguousarray(tb[k][:, :N_IDS])
    frames = frames_of(tb)
    ctx = nrs.Context()
    cam = nrs.make_camera(tb["model"], tb["prm"])
    rpp = tb["rad_per_pixel"]
    lines = []
    flat_bytes = N_SNAPS * N_IDS * 22 + 4 * N_IDS + 32 * N_SNAPS
    frame_bytes = int(np.mean([32 + 28 * int((f["status"] <= 1).sum()) for f in frames]))
    # ---- pass 1: wall clock
    t, same, info, n_cand = run(ctx, cam, tb, frames, rpp, a.reps, a.warm, False)
    base = dict(device=ctx.device_name(), n_ids=info[1], n_snapshots=info[0], n_candidates=n_cand, reps=a.reps, warm=a.warm, same_results=bool(same))
    for path in ("host", "resident"):
        lines.append(dict(base, **{"pass": "wall", "path": path, "upload_bytes_per_frame": flat_bytes if path == "host" else frame_bytes,
                                   "median_ms": {k: med(v) for k, v in t[path].items()}, "min_ms": {k: round(float(np.min(v)), 4) for k, v in t[path].items()}}))
    # ---- pass 2: the library's stages (NRS_TIMING=1 writes them to stderr: read from a file descriptor of our own)
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            nrs.debug_set("NRS_TIMING", "1")
            t2, same2, _, _ = run(ctx, cam, tb, frames, rpp, a.reps, a.warm, True)
            nrs.debug_set("NRS_TIMING", None)
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    stages = {}
    for m in re.finditer(r"\[nrs\] (nrs_map_frame(?:_tbuf)?) (.+?)\s+([0-9.]+) ms", text):
        stages.setdefault(m.group(1), {}).setdefault(m.group(2).strip(), []).append(float(m.group(3)))
    for path, who in (("host", "nrs_map_frame"), ("resident", "nrs_map_frame_tbuf")):
        st = {k: med(v[-a.reps:]) for k, v in stages.get(who, {}).items()}
        lines.append(dict(base, **{"pass": "NRS_TIMING", "path": path, "same_results": bool(same2), "python_median_ms": {k: med(v) for k, v in t2[path].items()},
                                   "library_stage_median_ms": st}))
    ctx.close()
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
