"""Times the keyframe BA of the frame loop as ONE call on the device-resident graph (nrs_dba_solve_window_rg) against what feeding the
existing call costs: GetEdges of every point at capacity - 1 (nrs_rgraph_get_edges: the whole lists through the host), the CSR made of
them, nrs_dba_solve_window.  A 5-keyframe window (every keyframe without its own third of the points) at about 1k and 5k map points, the
graph all-pairs with one update.  Wall clock around the synchronous calls, medians after a warm-up; the two results are compared bit for bit.
--nodes M: the EMBEDDED window instead -- M nodes at 5000 points, M / 5 at 1000 (farthest-point sampling, nrs_synth.pick_nodes): the one call
nrs_dba_solve_window_rg_embedded against the same GetEdges of every point at capacity - 1, its download and nrs_dba_solve_window_embedded.
    python tools/kf_ba_probe.py [--reps 7] [--nodes M] [--out profiles/kf_ba_probe.txt]"""
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
    ap.add_argument("--nodes", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = nrs.Context()
    lines = ["device: %s" % ctx.device_name()]
    for n in (1000, 5000):
        p = S.make_dba_problem(n, 5, 21, S.PINHOLE, dropout=1.0 / 3.0)
        X0 = np.asarray(p["scene"]["X0"], np.float32)
        rng = np.random.default_rng(n)
        ext = float(np.linalg.norm(X0.max(0) - X0.min(0)))
        sigma = 0.7 * ext / 1.5
        X1 = (np.asarray(p["scene"]["Xk_true"][-1], np.float64) + rng.normal(0, 0.02 * sigma, (n, 3))).astype(np.float32)
        ids = np.arange(n, dtype=np.int32)
        rg = nrs.RGraph(ctx, n, sigma, 0.06)
        rg.add_edges(X0, ids, ids)
        rg.update(X1, ids)
        cam = nrs.make_camera(p["model"], p["prm"])
        qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)

        m_nodes = max(1, a.nodes * n // 5000) if a.nodes > 0 else 0
        flag = S.pick_nodes(p["scene"]["X0"], m_nodes) if m_nodes else None

        def one_call():
            if flag is not None:
                return ctx.dba_solve_window_rg_embedded(cam, qt, p["kf_points"], p["lm_xyz"], p["lm_uv"], rg, flag, p["scale"], 5)
            return ctx.dba_solve_window_rg(cam, qt, p["kf_points"], p["lm_xyz"], p["lm_uv"], rg, p["scale"], 5)

        def through_the_host():
            cnt, col, w, d0, st = rg.get_edges(ids, n - 1)
            rowptr = np.zeros(n + 1, np.int32)
            rowptr[1:] = np.cumsum(cnt)
            keep = np.arange(n - 1)[None, :] < cnt[:, None]
            g = dict(rowptr=rowptr, col=col[keep], w=w[keep], d0=d0[keep], status=st[keep])
            if flag is not None:
                return ctx.dba_solve_window_embedded(cam, qt, p["kf_points"], p["lm_xyz"], p["lm_uv"], flag, g, p["scale"], 5)
            return ctx.dba_solve_window(cam, qt, p["kf_points"], p["lm_xyz"], p["lm_uv"], g, p["scale"], 5)

        r1 = one_call()
        st = ctx.dba_window_rg_stats()
        if flag is not None:
            e = ctx.dba_window_edges_embedded()
            ns, nd = len(e["sp_d0"]), len(e["dm_w"])
            what = "%d observations (%d nodes: %d node copies, %d skinned)" % (sum(len(k) for k in p["kf_points"]), m_nodes, len(e["lm_obs"]), len(e["sk_obs"]))
        else:
            ns, nd = ctx.dba_window_edge_counts()
            what = "%d landmarks" % sum(len(k) for k in p["kf_points"])
        m = median_ms(one_call, a.reps)
        head = "%5d points x 5 keyframes: %s, %d springs, %d dampers; prefix %d after %d round(s)" % (n, what, ns, nd, st["cap"], st["rounds"])
        try:
            r2 = through_the_host()
        except nrs.NrsError as e:                                  # (lists longer than GetEdges sorts in one workgroup's LDS on this device)
            lines.append("%s | one call %.2f ms (min %.2f max %.2f) | full lists through the host: not available (%s)" % (head, *m, e))
            rg.close()
            continue
        same = np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
        h = median_ms(through_the_host, a.reps)
        lines.append("%s | one call %.2f ms (min %.2f max %.2f) | full lists through the host %.2f ms (min %.2f max %.2f) | same bits: %s"
                     % (head, *m, *h, same))
        rg.close()
    ctx.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
