"""Embedded BA window at C2 x 500: LM iterations / s and PCG iterations per optimize(5) of
  - the unsharded keyframe-block factorisation (embedded_solver = 1),
  - the sharded path at world 1 over RCCL with sharded_kft = 0 (block-Jacobi PCG) and 1 (the factorisation),
  - 2 and 4 thread ranks on one GPU with sharded_kft = 1 (a COST figure of the hand-overs and all-reduces, not scaling).
usage: python tools/sharded_kft_probe.py [reps]"""
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nr-slam_amd/py"))
import nrs  # noqa: E402
import nrs_synth as S  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
p = S.make_dba_problem("C2")
flag, nb = S.embedded_problem(p, 500)
e = nrs.dba_build_edges_embedded(p["kf_points"], flag, nb)
w = S.embedded_window(p, e)
cam = nrs.make_camera(p["model"], p["prm"])
qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)


def timed(ctx):
    """one warm-up optimize(5), then `reps` timed reset + optimize(5): (LM it/s of the fastest, PCG iterations per optimize(5), kft on)"""
    ctx.dba_upload_embedded(cam, qt, w, e, p["scale"])
    on = ctx.debug_kft_info()["on"]
    tr = nrs.Trace()
    ctx.dba_optimize(5, tr)
    ts = []
    for _ in range(reps):
        ctx.dba_reset()
        t0 = time.perf_counter()
        ctx.dba_optimize(5)
        ts.append(time.perf_counter() - t0)
    return tr.iterations / min(ts), sum(t["inner"] for t in tr.trials), on


def report(name, rate, inner, on):
    print("%-34s %7.1f LM it/s  %5d PCG it / optimize(5)  factorisation %s" % (name, rate, inner, on), flush=True)


c = nrs.Context(embedded_solver=1)
report("unsharded, embedded_solver 1", *timed(c))
c.close()
for skft in (0, 1):
    c = nrs.Context(embedded_solver=1, sharded_kft=skft)
    c.comm_init_rccl(1, 0, nrs.comm_unique_id())
    report("RCCL world 1, sharded_kft %d" % skft, *timed(c))
    c.close()
for world in (2, 4):
    group = nrs.LocalGroup(world)
    res = [None] * world

    def rank(r):
        c = nrs.Context(embedded_solver=1, sharded_kft=1)
        c.comm_init_local(group, r)
        res[r] = timed(c)
        c.close()

    th = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(900)
    group.close()
    report("%d thread ranks, sharded_kft 1" % world, *res[0])
