"""Set-up time and resident bytes per rank of ONE sharded window (thread ranks on one GPU), the two constructions side by side:
the device path (csrc/nrs_engine_devpack.hpp on a communicator) and the host path (NRS_HOST_PACK=1), alternating, medians of
`reps` uploads after one warm-up of each.
  python tools/shard_pack_probe.py [workload] [world] [reps]"""
import os, sys, threading, time, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nr-slam_amd/py"))
import numpy as np, nrs, nrs_synth as S
name = sys.argv[1] if len(sys.argv) > 1 else "C4"
world = int(sys.argv[2]) if len(sys.argv) > 2 else 8
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
n, k, seed, model = S.CONFIGS[name]
p = S.make_dba_problem(n, k, seed, model)
e = nrs.dba_build_edges(p["kf_points"], p["nbr"])
cam = nrs.make_camera(p["model"], p["prm"])
qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
c = nrs.Context()
t0 = time.perf_counter(); c.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"]); t1 = time.perf_counter()
st = c.dba_stats(); c.close()
print({"workload": name, "ranks": 1, "upload_s": t1 - t0, "device_GB": st["device_bytes"] / 1e9, "spring_slots": st["spring_slots"]}, flush=True)


def one(host):
    """one sharded upload (fresh contexts) + one LM iteration; per rank: seconds in the upload, what it holds, which path built it"""
    nrs.debug_set("NRS_HOST_PACK", "1" if host else None)
    group = nrs.LocalGroup(world)
    res = [None] * world
    def rank_main(r):
        cc = nrs.Context(); cc.comm_init_local(group, r)
        t0 = time.perf_counter(); cc.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"]); t1 = time.perf_counter()
        s = cc.dba_stats(); dev = cc.dba_pack_hash()[21] if name != "C4" else -1      # (the hash downloads every array: not at C4)
        tr = nrs.Trace(); t2 = time.perf_counter(); cc.dba_optimize(1, tr); t3 = time.perf_counter()
        res[r] = dict(rank=r, upload_s=t1 - t0, device_GB=s["device_bytes"] / 1e9, spring_slots=s["spring_slots"], packed_rows=s["packed_rows"], optimize1_s=t3 - t2, device_built=dev)
        cc.close()
    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(world)]
    [t.start() for t in th]; [t.join(600) for t in th]
    group.close()
    nrs.debug_set("NRS_HOST_PACK", None)
    return res


one(False); one(True)                                               # warm-up: scratch allocations, code objects
runs = {False: [], True: []}
for _ in range(reps):
    for host in (False, True):
        runs[host].append(one(host))
print("%-5s %14s %14s %8s %10s %12s %8s" % ("rank", "device_pack_s", "host_pack_s", "ratio", "device_GB", "packed_rows", "built"))
for r in range(world):
    dv = statistics.median(x[r]["upload_s"] for x in runs[False]); hs = statistics.median(x[r]["upload_s"] for x in runs[True])
    last = runs[False][-1][r]
    print("%-5d %14.4f %14.4f %8.2f %10.3f %12d %8s" % (r, dv, hs, hs / dv, last["device_GB"], last["packed_rows"], {1: "device", 0: "host", -1: "?"}[last["device_built"]]))
print({"workload": name, "world": world, "reps": reps, "optimize1_s_median": statistics.median(x[0]["optimize1_s"] for x in runs[False])})
