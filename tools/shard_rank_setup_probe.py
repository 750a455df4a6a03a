"""Set-up of ONE rank of a sharded window on its own (no contention for the host or the device): where its time goes (NRS_TIMING=1
marks), the device path (csrc/nrs_engine_devpack.hpp on a communicator) and the host path (NRS_HOST_PACK=1) side by side,
alternating, medians of `reps` set-ups after one warm-up of each.  The upload ends in an agreement with the other ranks, which do
not exist here, so every set-up runs on a thread that is left waiting; its time is the sum of its marks, read from this process's
stderr (redirected to a file).
  python tools/shard_rank_setup_probe.py [workload] [world] [rank] [reps]"""
import os, re, sys, tempfile, threading, time, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nr-slam_amd/py"))
os.environ["NRS_TIMING"] = "1"
import numpy as np, nrs, nrs_synth as S
name = sys.argv[1] if len(sys.argv) > 1 else "C4"
world = int(sys.argv[2]) if len(sys.argv) > 2 else 8
rank = int(sys.argv[3]) if len(sys.argv) > 3 else 3
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
limit_s = float(os.environ.get("PROBE_LIMIT_S", "120"))
n, k, seed, model = S.CONFIGS[name]
p = S.make_dba_problem(n, k, seed, model)
e = nrs.dba_build_edges(p["kf_points"], p["nbr"])
cam = nrs.make_camera(p["model"], p["prm"])
qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
log = tempfile.NamedTemporaryFile("w+", suffix=".txt")
sys.stderr.flush(); os.dup2(log.fileno(), 2)
MARK = re.compile(r"\[nrs\] (?:rank \d+/\d+ )?(device pack|engine_create) (.+?)\s+([0-9.]+) ms")
LAST = {"device pack": "final arrays", "engine_create": "pinned+sync"}


def one(host):
    """marks of one set-up: [(path, stage, ms)] up to the path's last mark"""
    nrs.debug_set("NRS_HOST_PACK", "1" if host else None)
    start = os.path.getsize(log.name)
    group = nrs.LocalGroup(world)
    cc = nrs.Context(); cc.comm_init_local(group, rank)
    th = threading.Thread(target=lambda: cc.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"]), daemon=True)
    th.start()
    t_end = time.time() + limit_s
    want = "engine_create" if host else "device pack"
    while time.time() < t_end:
        time.sleep(0.02)
        with open(log.name) as fh:
            fh.seek(start)
            marks = [(m.group(1), m.group(2).strip(), float(m.group(3))) for m in MARK.finditer(fh.read())]
        if any(path == want and stage == LAST[want] for path, stage, _ in marks):
            return marks
    print("no final mark within %.0f s" % limit_s, flush=True)
    os._exit(1)


one(False); one(True)
runs = {False: [], True: []}
for _ in range(reps):
    for host in (False, True):
        runs[host].append(one(host))
for host in (False, True):
    tot = [sum(ms for _, _, ms in r) for r in runs[host]]
    print("%s path: set-up %.1f ms (median of %d; min %.1f, max %.1f)" % ("host" if host else "device", statistics.median(tot), reps, min(tot), max(tot)), flush=True)
    stages = []
    for path, stage, _ in runs[host][-1]:
        if (path, stage) not in stages: stages.append((path, stage))
    for path, stage in stages:
        v = statistics.median(sum(ms for p2, s2, ms in r if (p2, s2) == (path, stage)) for r in runs[host])
        print("    %-14s %-20s %9.2f ms  %5.1f %%" % (path, stage, v, 100.0 * v / statistics.median(tot)), flush=True)
dv = statistics.median(sum(ms for _, _, ms in r) for r in runs[False]); hs = statistics.median(sum(ms for _, _, ms in r) for r in runs[True])
print({"workload": name, "world": world, "rank": rank, "device_setup_ms": dv, "host_setup_ms": hs, "host_over_device": hs / dv}, flush=True)
os._exit(0)                                        # (the set-up threads wait for ranks that do not exist)
