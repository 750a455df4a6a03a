"""PointReuse, two-context path against the one-call path (include/nrs.h nrs_point_reuse), on the sequence of bench.py's tracked_fps leg and
a FrameLoop built as bench.py builds it (5000 points, all-pairs graph, 31 timed frames after one warm-up frame): the same frames twice,
GpuBackend(device_reuse=False) and GpuBackend(device_reuse=True).  Per run: median and p95 of the point-reuse stage (FrameLoop.point_reuse
as a whole: host projection and bookkeeping included) and of the whole frame, and the candidate counts.

    python tools/point_reuse_probe.py [--points 5000] [--frames 31] [--out profiles/point_reuse_probe.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "nr-slam_amd", "py"), os.path.join(ROOT, "oracle"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def run(sq, frames, device_reuse):
    import nrs
    import nrs_frame_loop as FL
    opts = dict(win=21, max_level=4, max_iters=10, epsilon=1e-4, min_eig=1e-4)
    gb = FL.GpuBackend(nrs, sq["model"], sq["prm"], opts, dense_graph=True, cap_per_point=128, device_reuse=device_reuse)
    loop = FL.FrameLoop(gb, lambda pc: FL.project_f32(sq["model"], sq["prm"], pc), sq["wh"], sq["scale"], sq["kp0"], sq["X0"], sq["graph"],
                        sq["pose_q"][0], sq["pose_t"][0], sq["images"][0])
    t_reuse, t_frame, n_cand, n_acc = [], [], [], []
    inner = loop.point_reuse

    def timed(im, lost):
        t0 = time.perf_counter()
        r = inner(im, lost)
        t_reuse.append(time.perf_counter() - t0)
        n_cand.append(len(loop.last_reuse["cand_id"]))
        n_acc.append(int(loop.last_reuse["accepted"].sum()))
        return r
    loop.point_reuse = timed
    for f in range(1, frames + 2):
        t0 = time.perf_counter()
        loop.track_image(sq["images"][f])
        t_frame.append(time.perf_counter() - t0)
    second_context = gb._ctx_reuse is not None
    calls = gb.n_device_reuse
    gb.close()
    ms_r, ms_f = 1e3 * np.asarray(t_reuse[1:]), 1e3 * np.asarray(t_frame[1:])      # (the first frame warms the code objects up)
    return dict(device_reuse=device_reuse, frames=len(ms_f), reuse_median=float(np.median(ms_r)), reuse_p95=float(np.percentile(ms_r, 95)),
                frame_median=float(np.median(ms_f)), frame_p95=float(np.percentile(ms_f, 95)), cand=n_cand[1:], accepted=n_acc[1:],
                second_context=second_context, device_calls=calls,
                log=[(tuple(L["lost"]), L["reused"], L["n_tracked"], L["keyframe"]) for L in loop.log])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--frames", type=int, default=31)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_reuse_probe.txt"))
    a = ap.parse_args()
    import nrs_synth as S
    sq = S.make_frame_sequence(a.points, a.frames + 2, 21)
    rows = [run(sq, a.frames, False), run(sq, a.frames, True)]
    lines = ["PointReuse: two-context path (device_reuse off) against nrs_point_reuse (device_reuse on); %d points, %d timed frames, all-pairs graph"
             % (sq["n_points"], rows[0]["frames"]),
             "%-14s %14s %12s %14s %12s %10s %10s %8s" % ("device_reuse", "reuse med ms", "reuse p95", "frame med ms", "frame p95", "cand/frame", "acc/frame", "ctx 2")]
    for r in rows:
        lines.append("%-14s %14.3f %12.3f %14.3f %12.3f %10.1f %10.1f %8s" % ("on" if r["device_reuse"] else "off", r["reuse_median"], r["reuse_p95"],
                                                                              r["frame_median"], r["frame_p95"], np.mean(r["cand"]), np.mean(r["accepted"]),
                                                                              "made" if r["second_context"] else "never"))
    same = rows[0]["log"] == rows[1]["log"] and rows[0]["cand"] == rows[1]["cand"] and rows[0]["accepted"] == rows[1]["accepted"]
    lines.append("candidates per frame (min / max): %d / %d; device calls with the switch on: %d" % (min(rows[1]["cand"]), max(rows[1]["cand"]), rows[1]["device_calls"]))
    lines.append("both runs: lost sets, reused counts, tracked counts, keyframes, candidate and accepted counts per frame %s" % ("EQUAL" if same else "DIFFER"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
