#!/usr/bin/env python3
"""Bit fingerprints of a fixed list of solves through py/nrs.py: per case a SHA-256 over the full LM trial trace (iter, trial, accepted,
early, inner, lam, chi, chi_new, rho as raw bytes) and the downloaded poses and points.  Run it once per library (NRS_LIB=<path> selects
one) and compare the outputs: a change that is meant to leave every launch and every number alone gives the same lines.  The bits depend
on the compiler, so the output is a record (profiles/), not a golden test.

    python tools/solve_fingerprint.py [substring of the case names | -substring: all but those] > fingerprint.txt

The group `switches` (SWITCH_TRIPLES below) is a step of its own: `... "switches: "`, and `... "-switches: "` for the rest."""
import hashlib
import os
import struct
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "nr-slam_amd", "py"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import nrs  # noqa: E402
import nrs_synth as S  # noqa: E402
import embedded_window_cases as W  # noqa: E402
import window_rg_cases as RGW  # noqa: E402
import window_rg_embedded_cases as RGE  # noqa: E402


def digest(trials, *arrays):
    h = hashlib.sha256()
    for t in trials:
        h.update(struct.pack("<iiiiidddd", t["iter"], t["trial"], int(t["accepted"]), int(t["early"]), t["inner"], t["lam"], t["chi"], t["chi_new"], t["rho"]))
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return "%s trials=%d inner=%d" % (h.hexdigest(), len(trials), sum(t["inner"] for t in trials))


def window(n, k, seed, env=(), steps=1, pack=False, **opts):
    p = S.make_dba_problem(n, k, seed)
    e = nrs.dba_build_edges(p["kf_points"], p["nbr"])
    cam = nrs.make_camera(p["model"], p["prm"])
    qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
    for name in env:
        nrs.debug_set(name, env[name])
    try:
        c = nrs.Context(**opts)
        c.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"])
        head = pack_digest(c) if pack else ""
        trials = []
        for _ in range(steps):                                        # (the second step's batches are sized by the first's predictors)
            c.dba_reset()
            tr = nrs.Trace()
            c.dba_optimize(5, tr)
            trials += tr.trials
        pq, xyz = c.dba_download()
        c.close()
    finally:
        nrs.debug_clear()
    return head + digest(trials, pq, xyz)


def pack_digest(c):
    """the 24 words of nrs_dba_pack_hash (the checksums of every packed array; word 21: built on the device) as one short hash"""
    return "pack=%s " % hashlib.sha256(np.ascontiguousarray(c.dba_pack_hash()).tobytes()).hexdigest()[:16]


def with_switches(env, fn):
    """fn() with the switches of env set for the contexts it creates (and for the live ones)"""
    for name in env:
        nrs.debug_set(name, env[name])
    try:
        return fn()
    finally:
        nrs.debug_clear()


def frame(direct, **opts):
    tp = S.make_tracking_problem(1150, 7)
    cam = nrs.make_camera(tp["model"], tp["prm"])
    fm = np.arange(1150, dtype=np.int32)
    c = nrs.Context(direct_solve=direct, **opts)
    trials, out = [], []
    for _ in range(2):                                                # (the second frame's speculative batches are sized by the first's runs)
        tr = nrs.Trace(1024)
        r = c.track_deform_solve(cam, tp["graph"], tp["X_prev"], fm, tp["status"], tp["uv"], tp["X_prev"], tp["pose_q"], tp["pose_t"], tp["scale"], tr)
        trials += tr.trials
        out += [r["pose_q"], r["pose_t"], r["f_pos"], r["f_status"], r["map_pos"]]
    c.close()
    return digest(trials, *out)


def embedded(solver, **opts):
    p, flag, nb = W.window(W.CASES[0], "nodes")
    e = nrs.dba_build_edges_embedded(p["kf_points"], flag, nb)
    w = S.embedded_window(p, e)
    c = nrs.Context(embedded_solver=solver, **opts)
    tr = nrs.Trace()
    pq, xyz, sk = c.dba_solve_embedded(nrs.make_camera(p["model"], p["prm"]), np.concatenate([p["poses_q"], p["poses_t"]], 1), w, e, p["scale"], 5, tr)
    c.close()
    return digest(tr.trials, pq, xyz, sk)


def run_ranks(group, world, rank_main, out):
    """One thread per rank; a rank that raises or does not finish says so in its place of the line, not a bare None."""
    def guarded(r):
        try:
            rank_main(r)
        except Exception as exc:                                      # (e.g. debug_kft_share where the factorisation was dropped)
            out[r] = "ERROR %s: %s" % (type(exc).__name__, exc)

    th = [threading.Thread(target=guarded, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    group.close()
    return " | ".join("NOT FINISHED" if o is None else str(o) for o in out)


def sharded(world=2, pack=False, **opts):
    p = S.make_dba_problem(300, 4, 41)
    e = nrs.dba_build_edges(p["kf_points"], p["nbr"])
    cam = nrs.make_camera(p["model"], p["prm"])
    qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
    group = nrs.LocalGroup(world)
    out = [None] * world

    def rank_main(r):
        c = nrs.Context(**opts)
        c.comm_init_local(group, r)
        c.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"])
        head = pack_digest(c) if pack else ""
        tr = nrs.Trace()
        c.dba_optimize(5, tr)
        pq, xyz = c.dba_download()
        out[r] = head + digest(tr.trials, pq, xyz)
        c.close()

    return run_ranks(group, world, rank_main, out)


def sharded_embedded(world, **opts):
    """The embedded 300 x 4 x 40 window with the keyframe-block factorisation sharded over `world` thread ranks (sharded_kft = 1)."""
    p, flag, nb = W.window(W.CASES[0], "nodes")
    e = nrs.dba_build_edges_embedded(p["kf_points"], flag, nb)
    w = S.embedded_window(p, e)
    cam = nrs.make_camera(p["model"], p["prm"])
    qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
    group = nrs.LocalGroup(world)
    out = [None] * world

    def rank_main(r):
        c = nrs.Context(embedded_solver=1, sharded_kft=1, **opts)
        c.comm_init_local(group, r)
        tr = nrs.Trace()
        pq, xyz, sk = c.dba_solve_embedded(cam, qt, w, e, p["scale"], 5, tr)
        share = c.debug_kft_share()                                   # (an error where the factorisation is not on: its keyframes and what it carved)
        out[r] = digest(tr.trials, pq, xyz, sk) + " kft k0=%d nk=%d kib=%d" % (share["k0"], share["nk"], share["kib"])
        c.close()

    return run_ranks(group, world, rank_main, out)


# ---- the one-call windows (nrs_dba_solve_window*): validation, edge lists, set-up, solve and download inside one entry point
def _qt(p):
    return np.concatenate([p["poses_q"], p["poses_t"]], 1)


def one_call_window(**opts):
    p = S.make_dba_problem(300, 4, 32)
    c = nrs.Context(**opts)
    tr = nrs.Trace()
    pq, xyz = c.dba_solve_window(nrs.make_camera(p["model"], p["prm"]), _qt(p), p["kf_points"], p["lm_xyz"], p["lm_uv"], p["nbr"], p["scale"], 5, tr)
    c.close()
    return digest(tr.trials, pq, xyz)


def _resident_graph(ctx, c):
    """the device-resident graph of a tests/window_rg_cases.py case: all pairs at the start positions, one update at the perturbed ones"""
    ids = np.arange(c["n"], dtype=np.int32)
    rg = nrs.RGraph(ctx, c["n"], c["sigma"], RGW.STRETCH_TH)
    rg.add_edges(c["X0"], ids, ids)
    rg.update(c["X1"], ids)
    return rg


def one_call_window_rg(name, **opts):
    """900x6_kb8: the smallest case of tests/window_rg_cases.py the device packer builds (4608 padded rows against its threshold of 2048);
    120x3 (768 rows): the smallest that falls to the host packer with the device-built lists copied back"""
    c = RGW.case(name)
    p = c["p"]
    ctx = nrs.Context(**opts)
    rg = _resident_graph(ctx, c)
    tr = nrs.Trace()
    pq, xyz = ctx.dba_solve_window_rg(nrs.make_camera(p["model"], p["prm"]), _qt(p), p["kf_points"], p["lm_xyz"], p["lm_uv"], rg, p["scale"], 5, tr)
    rg.close()
    ctx.close()
    return digest(tr.trials, pq, xyz)


def one_call_embedded(**opts):
    p, flag, nb = W.window(W.CASES[0], "nodes")
    c = nrs.Context(**opts)
    tr = nrs.Trace()
    pq, xyz = c.dba_solve_window_embedded(nrs.make_camera(p["model"], p["prm"]), _qt(p), p["kf_points"], p["lm_xyz"], p["lm_uv"], flag, nb, p["scale"], 5, tr)
    on_device = c.dba_window_edges_embedded()["on_device"]
    c.close()
    return digest(tr.trials, pq, xyz) + " on_device=%d" % on_device


def one_call_embedded_rg(**opts):
    c = RGE.case(RGE.CASES[0])
    p = c["p"]
    ctx = nrs.Context(**opts)
    rg = _resident_graph(ctx, c)
    tr = nrs.Trace()
    pq, xyz = ctx.dba_solve_window_rg_embedded(nrs.make_camera(p["model"], p["prm"]), _qt(p), p["kf_points"], p["lm_xyz"], p["lm_uv"], rg, c["flag"], p["scale"], 5, tr)
    rg.close()
    ctx.close()
    return digest(tr.trials, pq, xyz)


def one_call_sharded(embedded, world=2, env=(), **opts):
    """the one-call window (plain 300 x 4, or its 40-node embedded form) on `world` thread ranks; env: switches set for the ranks' contexts"""
    if embedded:
        p, flag, nb = W.window(W.CASES[0], "nodes")
    else:
        p = S.make_dba_problem(300, 4, 32)
    cam = nrs.make_camera(p["model"], p["prm"])
    group = nrs.LocalGroup(world)
    out = [None] * world

    def rank_main(r):
        c = nrs.Context(**opts)
        c.comm_init_local(group, r)
        tr = nrs.Trace()
        if embedded:
            pq, xyz = c.dba_solve_window_embedded(cam, _qt(p), p["kf_points"], p["lm_xyz"], p["lm_uv"], flag, nb, p["scale"], 5, tr)
            out[r] = digest(tr.trials, pq, xyz) + " on_device=%d" % c.dba_window_edges_embedded()["on_device"]
        else:
            pq, xyz = c.dba_solve_window(cam, _qt(p), p["kf_points"], p["lm_xyz"], p["lm_uv"], p["nbr"], p["scale"], 5, tr)
            out[r] = digest(tr.trials, pq, xyz)
        c.close()

    return with_switches(env, lambda: run_ranks(group, world, rank_main, out))


# ---- the group `switches`: ONE switch set on a small case of a kind on which a test or a tool sets it, one line per triple -- the pack
# hash where the case is a BA window, and the solve digest.  Equal-result A/B tests cannot see two rows of the switch table
# (nr-slam_amd/csrc/nrs_switches.hpp) mapped to each other; the lines of two libraries run on THIS list can.  The list is written out
# here, not read from the table: both libraries must run the same one.  (The four probe switches do nothing in a product build.)
SWITCH_CASES = {
    "window 500x5": lambda env: window(500, 5, 34, env, pack=True),
    "window 5000x8": lambda env: window(5000, 8, 21, env, pack=True),
    "embedded 300x4x40, factorisation": lambda env: with_switches(env, lambda: embedded(1)),
    "embedded 300x4x40, PCG": lambda env: with_switches(env, lambda: embedded(2)),
    "a2 frame, direct solver": lambda env: with_switches(env, lambda: frame(1)),
    "a2 frame, PCG": lambda env: with_switches(env, lambda: frame(2)),
    "sharded 300x4, 2 ranks": lambda env: with_switches(env, lambda: sharded(2, pack=True)),
    "one call, 2 ranks: embedded 300x4x40": lambda env: one_call_sharded(True, env=env),
}
SWITCH_TRIPLES = [
    ("NRS_HOST_PACK", "1", "window 500x5"), ("NRS_NO_FUSED", "1", "window 500x5"), ("NRS_NO_LDS", "1", "window 500x5"), ("NRS_NO_LDS", "0", "window 500x5"),
    ("NRS_FUSED_MAX_ROWS", "0", "window 500x5"), ("NRS_SELL_T", "4", "window 500x5"), ("NRS_NO_EDGE_CHI", "1", "window 500x5"),
    ("NRS_HOST_THREADS", "3", "window 500x5"), ("NRS_POISON", "1", "window 500x5"), ("NRS_CHECK_EVAL", "1", "window 500x5"),
    ("NRS_HOST_PACK", "1", "window 5000x8"), ("NRS_DFORM", "1", "window 5000x8"), ("NRS_TILE_CUT_PCT", "60", "window 5000x8"), ("NRS_NO_ECD", "1", "window 5000x8"),
    ("NRS_NO_H4", "1", "window 5000x8"), ("NRS_RC", "1", "window 5000x8"), ("NRS_RC", "2", "window 5000x8"), ("NRS_RC", "7", "window 5000x8"),
    ("NRS_NT", "1", "window 5000x8"), ("NRS_SPEC_TRIALS", "1", "window 5000x8"), ("NRS_SPEC_FIRST", "2", "window 5000x8"), ("NRS_SPEC_MAX_ROWS", "1000", "window 5000x8"),
    ("NRS_NO_REARM", "1", "window 5000x8"), ("NRS_HOST_THREADS", "1", "window 5000x8"),
    ("NRS_KFT_TWO_LAUNCHES", "1", "embedded 300x4x40, factorisation"), ("NRS_KFT_SCALAR_SWEEP", "1", "embedded 300x4x40, factorisation"),
    ("NRS_KFT_FOUR_WAVES", "1", "embedded 300x4x40, factorisation"), ("NRS_KFT_NO_RESIDUAL_TEST", "1", "embedded 300x4x40, factorisation"),
    ("NRS_SKIN_OP_OWN_LAUNCH", "1", "embedded 300x4x40, PCG"), ("NRS_SKIN_ROWS_OWN_LAUNCH", "1", "embedded 300x4x40, PCG"), ("NRS_HIER", "1", "embedded 300x4x40, PCG"),
    ("NRS_NO_LDS", "1", "embedded 300x4x40, PCG"),
    ("NRS_ND_NO_CACHE", "1", "a2 frame, direct solver"), ("NRS_ND_CHAIN", "1", "a2 frame, direct solver"), ("NRS_ND_LEVELS", "1", "a2 frame, direct solver"),
    ("NRS_ND_THREADS", "256", "a2 frame, direct solver"), ("NRS_ND_STEP32", "0", "a2 frame, direct solver"), ("NRS_ND_BACK_FLAGS", "1", "a2 frame, direct solver"),
    ("NRS_ND_MAX_ROWS", "300", "a2 frame, direct solver"), ("NRS_ND_NO_SPLIT", "1", "a2 frame, direct solver"), ("NRS_SPEC_TRIALS", "0", "a2 frame, direct solver"),
    ("NRS_SPEC_TRIALS", "3", "a2 frame, direct solver"), ("NRS_SPEC_FIXED", "2", "a2 frame, direct solver"), ("NRS_SPEC_FIRST", "3", "a2 frame, direct solver"),
    ("NRS_SPEC_NO_ABORT", "1", "a2 frame, direct solver"), ("NRS_HOST_THREADS", "1", "a2 frame, direct solver"), ("NRS_HOST_WALK", "1", "a2 frame, direct solver"),
    ("NRS_WALK_MAX_PASSES", "2", "a2 frame, direct solver"), ("NRS_COARSE_MIN_TILES", "0", "a2 frame, PCG"),
    ("NRS_SHARD_FULL_VECTORS", "1", "sharded 300x4, 2 ranks"), ("NRS_TILE_CUT_PCT", "60", "sharded 300x4, 2 ranks"),
    ("NRS_HOST_PACK", "1", "sharded 300x4, 2 ranks"), ("NRS_SHARD_EMBWIN_DEVICE", "1", "one call, 2 ranks: embedded 300x4x40"),
]


CASES = [
    ("window 300x4 fused", lambda **o: window(300, 4, 32, **o)),
    ("window 500x5 NRS_NO_FUSED", lambda **o: window(500, 5, 34, {"NRS_NO_FUSED": "1"}, **o)),
    ("window 5000x8 two-kernel, speculative trials", lambda **o: window(5000, 8, 21, steps=2, **o)),
    ("window 5000x8 two-kernel, NRS_SPEC_TRIALS=0", lambda **o: window(5000, 8, 21, {"NRS_SPEC_TRIALS": "0"}, steps=2, **o)),
    ("a2 frame, direct solver, speculative trials", lambda **o: frame(1, **o)),
    ("a2 frame, PCG", lambda **o: frame(2, **o)),
    ("embedded 300x4x40, factorisation", lambda **o: embedded(1, **o)),
    ("embedded 300x4x40, PCG", lambda **o: embedded(2, **o)),
    ("sharded 300x4, 2 thread ranks", lambda **o: sharded(2, **o)),
    ("sharded embedded 300x4x40, factorisation, 2 ranks", lambda **o: sharded_embedded(2, **o)),
    ("sharded embedded 300x4x40, factorisation, 3 ranks", lambda **o: sharded_embedded(3, **o)),
    ("one call: window 300x4", one_call_window),
    ("one call: rg window 900x6_kb8", lambda **o: one_call_window_rg("900x6_kb8", **o)),
    ("one call: rg window 120x3", lambda **o: one_call_window_rg("120x3", **o)),
    ("one call: embedded 300x4x40", one_call_embedded),
    ("one call: rg embedded 900x6_kb8", one_call_embedded_rg),
    ("one call, 2 thread ranks: window 300x4", lambda **o: one_call_sharded(False, **o)),
    ("one call, 2 thread ranks: embedded 300x4x40", lambda **o: one_call_sharded(True, **o)),
    ("one call, 2 ranks, SHARD_EMBWIN: embedded 300x4x40", lambda **o: one_call_sharded(True, env={"NRS_SHARD_EMBWIN_DEVICE": "1"}, **o)),
]
CASES += [("switches: %s=%s, %s" % (sw, v, case), lambda sw=sw, v=v, case=case: SWITCH_CASES[case]({sw: v})) for sw, v, case in SWITCH_TRIPLES]

if __name__ == "__main__":
    only = sys.argv[1] if len(sys.argv) > 1 else ""                  # (a substring of the case names: run those only, e.g. under a tracer)
    for name, fn in [x for x in CASES if (only[1:] not in x[0] if only.startswith("-") else only in x[0])]:
        for mode, opts in (("default", {}),) if name.startswith("switches: ") else (("default", {}), ("exact_trials", {"exact_trials": 1})):
            print("%-50s %-13s %s" % (name, mode, fn(**opts)), flush=True)
