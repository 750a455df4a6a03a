"""What a caller pays for ONE embedded BA window (a new one at every keyframe, mapping.cc:56-58), C2 x 500 nodes by default:
  three   host build (nrs_dba_build_edges_embedded) + gather (nrs_synth.embedded_window) + nrs_dba_solve_embedded
  one     nrs_dba_solve_window_embedded (the lists built on the device), timed as a whole
  marks   the one call under NRS_TIMING=1: its stage marks -- construction (kernels plus the copy back; and its parts: uploads, count pass
          + scans, emit pass + gathers, copy back), set-up, solve + download
  --ranks N   instead: the one call on N thread ranks (nrs.LocalGroup, contexts on one GPU), a device column (NRS_SHARD_EMBWIN_DEVICE=1: every rank
          builds its share of the lists on its device) and a host column (the default: every rank the host builder over the whole window).  Per rank:
          the call's time, the skinned observations it holds, the bytes of its lists' staging and of the skinned arrays in it; per
          column the construction marks of all ranks (NRS_TIMING=1, switched on after the warm-up)
Each figure is the median of five runs after a warm-up, on a context with the same options.  Every step runs in a process of its own
under `timeout`, and a failed step ends the script.
usage: python tools/embedded_window_probe.py [config, default C2] [n_nodes, default 500] [--ranks N]      (internal: --step NAME)"""
import json, os, re, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nr-slam_amd/py"))
RANKS = int(sys.argv[sys.argv.index("--ranks") + 1]) if "--ranks" in sys.argv else 0
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in ("--ranks", "--step")]
name = args[0] if len(args) > 0 else "C2"
m = int(args[1]) if len(args) > 1 else 500
STEPS = (("ranks-device", 300), ("ranks-host", 300)) if RANKS else (("three", 240), ("one", 240), ("marks", 240))
RUNS = 5


def med(x):
    return sorted(x)[len(x) // 2]


def ranks_step(which, p, flag, nb, cam, qt):
    """the one call on RANKS thread ranks; a rank that fails ends the step (the others leave their barrier through the group's abort)"""
    import threading, nrs
    group = nrs.LocalGroup(RANKS)
    rows, errs = [None] * RANKS, []

    def rank_main(r):
        try:
            c = nrs.Context()
            c.comm_init_local(group, r)
            c.debug_set("NRS_SHARD_EMBWIN_DEVICE", None if which == "ranks-host" else "1")       # (off: a communicator takes the host builder)
            tt = []
            for run in range(RUNS + 1):
                if run == 1:
                    c.debug_set("NRS_TIMING", "1")
                t0 = time.perf_counter(); tr = nrs.Trace(64)
                c.dba_solve_window_embedded(cam, qt, p["kf_points"], p["lm_xyz"], p["lm_uv"], flag, nb, p["scale"], 5, tr)
                if run:
                    tt.append(time.perf_counter() - t0)
            e, sl, sk = c.dba_window_edges_embedded(), c.dba_window_slice_embedded(), c.dba_skin_stats()
            rows[r] = dict(rank=r, total_ms=1e3 * med(tt), on_device=e["on_device"], keyframes=[sl["k0"], sl["k1"]], skinned_held=sl["sk_held"], skinned_window=len(e["sk_obs"]),
                           stage_bytes=sl["stage_bytes"], skinned_stage_bytes=sl["sk_stage_bytes"], skin_buffer_bytes=int(sk[2]), trials=len(tr.trials))
            c.close()
        except Exception as ex:
            errs.append((r, repr(ex)))

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(RANKS)]
    for t in th:
        t.start()
    for t in th:
        t.join(240)
    if errs or any(t.is_alive() for t in th) or any(x is None for x in rows):
        sys.exit("ranks step failed: %s" % errs)
    print(json.dumps(dict(step=which, workload="%s embedded, %d nodes, %d thread ranks" % (name, m, RANKS), ranks=rows)), flush=True)


def step(which):
    import numpy as np, nrs, nrs_synth as S
    p = S.make_dba_problem(name)
    flag, nb = S.embedded_problem(p, m)
    cam = nrs.make_camera(p["model"], p["prm"]); qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
    if which.startswith("ranks-"):
        return ranks_step(which, p, flag, nb, cam, qt)
    if which == "marks":
        nrs.debug_set("NRS_TIMING", "1")
    ctx = nrs.Context()
    out = dict(step=which, workload="%s embedded, %d nodes" % (name, m))
    if which == "three":
        tb, tg, ts, tt = [], [], [], []
        for r in range(RUNS + 1):
            t0 = time.perf_counter(); e = nrs.dba_build_edges_embedded(p["kf_points"], flag, nb)
            t1 = time.perf_counter(); w = S.embedded_window(p, e)
            t2 = time.perf_counter(); tr = nrs.Trace(64); ctx.dba_solve_embedded(cam, qt, w, e, p["scale"], 5, tr)
            t3 = time.perf_counter()
            if r:
                tb.append(t1 - t0); tg.append(t2 - t1); ts.append(t3 - t2); tt.append(t3 - t0)
        out.update(host_build_ms=1e3 * med(tb), gather_ms=1e3 * med(tg), solve_embedded_ms=1e3 * med(ts), total_ms=1e3 * med(tt))
    else:
        tt = []
        for r in range(RUNS + 1):
            print("[probe] run %d" % r, file=sys.stderr, flush=True)
            t0 = time.perf_counter(); tr = nrs.Trace(64)
            ctx.dba_solve_window_embedded(cam, qt, p["kf_points"], p["lm_xyz"], p["lm_uv"], flag, nb, p["scale"], 5, tr)
            if r:
                tt.append(time.perf_counter() - t0)
        e = ctx.dba_window_edges_embedded()
        out.update(total_ms=1e3 * med(tt), on_device=e["on_device"], kft=bool(ctx.debug_kft_info()["on"]))
    out.update(node_copies=len(e["lm_obs"]), skinned_obs=len(e["sk_obs"]), springs=len(e["sp_ij"]), dampers=len(e["dm_idx"]), trials=len(tr.trials))
    ctx.close()
    print(json.dumps(out), flush=True)


if "--step" in sys.argv:
    step(sys.argv[sys.argv.index("--step") + 1])
    sys.exit(0)
res = {}
for which, limit in STEPS:
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), name, str(m), "--step", which] + (["--ranks", str(RANKS)] if RANKS else []),
                       capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit("step %s failed with status %d: nothing further is run" % (which, r.returncode))
    res[which] = json.loads(r.stdout.strip().splitlines()[-1])
    if RANKS:                                                        # construction marks of every rank's timed runs (the warm-up has none)
        marks = [float(g.group(1)) for g in re.finditer(r"\[nrs\] embedded window construction\s+([0-9.]+) ms", r.stderr)]
        res[which]["construction_ms"] = dict(min=min(marks), median=med(marks), max=max(marks), n=len(marks)) if marks else None
        print(json.dumps(res[which]), flush=True)
        continue
    if which == "marks":                                             # stage marks of runs 1..5 (run 0 is the warm-up)
        stages, run = {}, -1
        for line in r.stderr.splitlines():
            g = re.match(r"\[probe\] run (\d+)", line)
            if g:
                run = int(g.group(1))
            g = re.match(r"\[nrs\] embedded (window|lists) (.*?)\s+([0-9.]+) ms", line)
            if g and run >= 1:                                       # (lists: the parts of the construction)
                stages.setdefault(("lists: " if g.group(1) == "lists" else "") + g.group(2), []).append(float(g.group(3)))
        res[which]["stage_ms"] = {k: med(v) for k, v in stages.items()}
    print(json.dumps(res[which]), flush=True)
if RANKS:
    for r in range(RANKS):
        d, h = res["ranks-device"]["ranks"][r], res["ranks-host"]["ranks"][r]
        print("rank %d keyframes [%d, %d): device %.2f ms, %d of %d skinned held, staging %d B (skinned %d B) | host %.2f ms, %d held, staging %d B (skinned %d B)" % (
            r, d["keyframes"][0], d["keyframes"][1], d["total_ms"], d["skinned_held"], d["skinned_window"], d["stage_bytes"], d["skinned_stage_bytes"],
            h["total_ms"], h["skinned_held"], h["stage_bytes"], h["skinned_stage_bytes"]))
    print("construction (all ranks, synchronising marks): device %s | host %s" % (res["ranks-device"]["construction_ms"], res["ranks-host"]["construction_ms"]))
    sys.exit(0)
a, b = res["three"]["total_ms"], res["one"]["total_ms"]
print("three steps %.2f ms (host build %.2f + gather %.2f + nrs_dba_solve_embedded %.2f), one call %.2f ms: %s" % (
    a, res["three"]["host_build_ms"], res["three"]["gather_ms"], res["three"]["solve_embedded_ms"], b,
    "the one call is %.2fx faster" % (a / b) if b < a else "the one call is NOT faster (%.2fx)" % (a / b)))
print("one call under NRS_TIMING=1 (synchronising marks): " + ", ".join("%s %.2f ms" % kv for kv in res["marks"]["stage_ms"].items()))
