"""Frames that are NOT the whole map in map order, for a2 (CameraPoseAndDeformationOptimization, g2o_optimization.cc:148-557, "OPT"):
a case builder, the two scenes the GPU tests run (tests/test_gpu_track_frames.py) and a replay of the neighbour walks over the ORACLE's
own GetEdges lists, with which tests/test_track_frame_cases_cpu.py proves that a scene reaches the branch it was made for.  Nothing
here reads the library.

With f_map = arange(n) the frame slot, the map id and the row of a GetEdges call are one number and the optimised points come in
ascending id order; here they are five different index spaces (slot, map id, index among the optimised points, vertex, list row)."""
import copy
import functools

import numpy as np

import nrs_oracle as O
import nrs_synth as S
import rgraph_oracle as RG

F32 = np.float32


def make_frame_view(tp, n_in_frame, n_unmapped, seed, permute=True, pool=None, n_just_triangulated=3):
    """A frame that sees n_in_frame of the map points of `tp` (nrs_synth.make_tracking_problem) in a seeded random slot order (permute =
    False: ascending map id), with n_unmapped slots without a map point (f_map = -1, TRACKED, zero uv / position) at random places
    among them.  Statuses, observations and positions are tp's, gathered per slot; n_just_triangulated optimised slots become
    JUST_TRIANGULATED.  pool: the map ids to choose from (default: all).  No map id appears twice (the reference's frame cannot)."""
    rng = np.random.default_rng(seed)
    n = len(tp["status"])
    pool = np.arange(n) if pool is None else np.asarray(pool, np.int64)
    chosen = rng.choice(pool, n_in_frame, replace=False)
    if not permute:
        chosen = np.sort(chosen)
    n_f = n_in_frame + n_unmapped
    mapped = np.ones(n_f, bool)
    mapped[rng.choice(n_f, n_unmapped, replace=False)] = False
    f_map = np.full(n_f, -1, np.int32)
    f_map[mapped] = chosen
    f_status = np.full(n_f, O.TRACKED, np.int32)
    f_status[mapped] = tp["status"][chosen]
    f_uv = np.zeros((n_f, 2), F32)
    f_uv[mapped] = tp["uv"][chosen]
    f_pos = np.zeros((n_f, 3), F32)
    f_pos[mapped] = tp["X_prev"][chosen]
    opt = np.where(mapped & (f_status == O.TRACKED_WITH_3D))[0]
    f_status[rng.choice(opt, min(n_just_triangulated, len(opt) // 4), replace=False)] = O.JUST_TRIANGULATED
    return dict(f_map=f_map, f_status=f_status, f_uv=f_uv, f_pos=f_pos)


def node_flags(frame, node_ids):
    """f_node of the embedded mode: one byte per FRAME SLOT (1: the slot's map point is one of node_ids)"""
    is_node = np.zeros(int(max(frame["f_map"].max(), np.max(node_ids))) + 1, bool)
    is_node[np.asarray(node_ids)] = True
    return ((frame["f_map"] >= 0) & is_node[np.maximum(frame["f_map"], 0)]).astype(np.uint8)


def optimised_ids(frame):
    """map ids of the optimised points, in frame order"""
    m = (frame["f_status"] == O.TRACKED_WITH_3D) & (frame["f_map"] >= 0)
    return frame["f_map"][m].astype(np.int64)


# ---- the walks of OPT:252-279 (stage 1) and OPT:476-553 (stage 2) over the oracle's lists
def _lists_of(graph):
    if isinstance(graph, dict):
        return lambda p: [(o, int(graph["e_status"][e])) for o, e in O.graph_get_edges(graph, p)]

    def dense(p):
        js, w, d0, st = graph.get_edges(p)
        return list(zip(js.tolist(), st.tolist()))
    return dense


def _frame_tables(n_map, f_map, f_status):
    f_map = np.asarray(f_map, np.int64)
    f_status = np.asarray(f_status)
    map_to_frame = -np.ones(n_map, np.int64)
    map_to_frame[f_map[f_map >= 0]] = np.where(f_map >= 0)[0]
    opt_f = np.where((f_status == O.TRACKED_WITH_3D) & (f_map >= 0))[0]
    ids = f_map[opt_f]
    id_to_idx = -np.ones(n_map, np.int64)
    id_to_idx[ids] = np.arange(len(ids))
    return map_to_frame, opt_f, ids, id_to_idx


def replay_walks(graph, f_map, f_status, f_node=None):
    """The walk of every optimised point (frame order) as nrs_oracle.track_deform_solve makes it -- f_node given: as
    embedded_oracle.track_deform_solve_embedded makes it (an optimised point without a vertex is passed over; a point without a vertex
    accepts nodes and pairs with nobody).  graph: the flat dict or a rgraph_oracle.DenseGraph BEFORE a2 (not modified).  Per walk:
      visited : list entries the loop looks at, the one it breaks at included (> 64: the entry lies in a later 64-entry chunk)
      how     : "eleven" (broke with 11 accepted), "bad" (broke at a BAD connection), "exhausted" (the list ended first)
      n_acc   : connections accepted
      listed  : the same count as `visited` on a list that leaves out the connections a walk passes over (embedded mode: those to
                optimised points without a vertex, unless BAD) -- what a source serving such lists holds
    and, over all walks, lost_first[map id] = the lowest 0-based list position at which a walk flags that point as lost."""
    n_map = graph["n"] if isinstance(graph, dict) else graph.n
    lists = _lists_of(graph)
    map_to_frame, opt_f, ids, id_to_idx = _frame_tables(n_map, f_map, f_status)
    f_status = np.asarray(f_status)
    N = len(ids)
    is_node = np.ones(N, bool) if f_node is None else np.asarray(f_node).astype(bool)[opt_f]
    reg = [set() for _ in range(N)]
    walks, lost_first = [], {}
    for idx in range(N):
        n_reg, visited, listed, how = 0, 0, 0, "exhausted"
        for a, (other, st) in enumerate(lists(int(ids[idx]))):
            visited += 1
            io = int(id_to_idx[other])
            passed_over = io >= 0 and not is_node[io]
            if st == O.GRAPH_BAD or not passed_over:
                listed += 1
            if n_reg > O.REGULARIZERS_PER_POINT:
                how = "eleven"
                break
            if st == O.GRAPH_BAD:
                how = "bad"
                break
            fo = map_to_frame[other]
            if fo < 0 or f_status[fo] != O.TRACKED_WITH_3D:
                if fo >= 0 and f_status[fo] != O.JUST_TRIANGULATED:
                    lost_first[other] = min(lost_first.get(other, a), a)
                continue
            if passed_over:
                continue
            if is_node[idx]:
                if io in reg[idx]:
                    continue
                reg[idx].add(io)
                reg[io].add(idx)
            n_reg += 1
        walks.append(dict(id=int(ids[idx]), visited=visited, listed=listed, how=how, n_acc=n_reg))
    return walks, lost_first


def replay_lost_walks(graph_after, f_map, f_status, lost_ids):
    """Stage 2 over the lists of the graph AFTER the oracle's a2 updated it.  Per lost point: `kept` -- its list without what the walk
    cannot see (kept: connections to optimised points, and BAD ones to anyone), as (other, optimised?, status) -- and `eleventh`: the
    1-based position in `kept` of the eleventh optimised neighbour (None: never; the walk breaks at the entry after it)."""
    n_map = graph_after["n"] if isinstance(graph_after, dict) else graph_after.n
    lists = _lists_of(graph_after)
    _, _, _, id_to_idx = _frame_tables(n_map, f_map, f_status)
    out = {}
    for lid in lost_ids:
        kept = [(o, bool(id_to_idx[o] >= 0), st) for o, st in lists(int(lid)) if id_to_idx[o] >= 0 or st == O.GRAPH_BAD]
        pos_opt = [k + 1 for k, e in enumerate(kept) if e[1]]
        out[int(lid)] = dict(kept=kept, eleventh=pos_opt[10] if len(pos_opt) > 10 else None,
                             n_opt_first32=sum(1 for e in kept[:32] if e[1]))
    return out


def stage2_retries(lw):
    """does a prefix of 32 kept entries leave this lost point's walk without its end (replay_lost_walks entry)?"""
    return len(lw["kept"]) > 32 and lw["n_opt_first32"] < 11 and (lw["eleventh"] is None or lw["eleventh"] > 32)


# ---- the flat-graph frame (tests of both restatements and of nrs_track_deform_solve)
FLAT_N, FLAT_SEED = 400, 61


@functools.lru_cache(None)
def flat_case():
    tp = S.make_tracking_problem(FLAT_N, FLAT_SEED)
    fr = make_frame_view(tp, 300, 25, 7)
    return tp, fr


# ---- Scene A: a sparse, permuted frame on a dense map
A_N, A_SEED, A_IN_FRAME, A_UNMAPPED, A_HOLE, A_SPECIAL, A_SPECIAL_NEUTRAL = 1200, 71, 150, 20, 200, 8, 70


def _dist(X, i):
    return np.linalg.norm(X.astype(np.float64) - X[i].astype(np.float64), axis=1)


@functools.lru_cache(None)
def scene_a():
    """1200 map points on the all-pairs graph, sigma such that the median point has 300 connections within 1.5 sigma; the frame sees an
    eighth of the map in random slot order: a walk meets an optimised point at every ~9th entry and reads its list far beyond the first 64.
    History (`updates`: positions, vertex ids -- applied by UpdateVertex in this order):
      1. the stretched patch of test_track_deform_on_the_dense_graph (a random half of the vertices updated);
      2. for A_SPECIAL optimised points one update each in which everything beyond their 70th neighbour had come close to them: ALL their
         far connections are BAD.  The all-pairs graph lists BAD connections only for such a point (a NEUTRAL connection below
         min_weight ends GetEdges before the BAD class, test_break_semantics_and_errors): its list runs 70 NEUTRAL entries, then BAD ones.
    One TRACKED (lost) point sits in a hole of the frame: none of its A_HOLE nearest map points is in the frame, so whoever finds it finds it
    far down a list."""
    tp = S.make_tracking_problem(A_N, A_SEED)
    X = tp["X_prev"]
    n = A_N
    rng = np.random.default_rng(A_SEED)
    d300 = np.array([np.partition(_dist(X, i), 300)[300] for i in range(n)])
    sigma = float(F32(np.median(d300) / 1.5))
    th = tp["graph"]["stretch_th"]
    # the frame: a lost point in a hole
    tracked = np.where(tp["status"] == O.TRACKED)[0]
    centre = np.median(X, axis=0)
    hole_pt = int(tracked[np.argmin(np.linalg.norm(X[tracked] - centre, axis=1))])
    near = np.argsort(_dist(X, hole_pt))[1:A_HOLE + 1]
    pool = np.setdiff1d(np.arange(n), np.concatenate([near, [hole_pt]]))
    fr = make_frame_view(tp, A_IN_FRAME - 1, A_UNMAPPED, A_SEED + 1, pool=pool)
    slot = int(np.where(fr["f_map"] < 0)[0][0])                     # the hole's point takes one more slot, at the first unmapped one's place
    for k, v in (("f_map", hole_pt), ("f_status", O.TRACKED), ("f_uv", tp["uv"][hole_pt]), ("f_pos", X[hole_pt])):
        fr[k] = np.insert(fr[k], slot, v, axis=0)
    # history 1: a patch stretched
    hist = X.copy()
    c0 = hist[3]
    patch = np.linalg.norm(hist - c0, axis=1) < 1.2 * sigma
    hist[patch] = c0 + (hist[patch] - c0) * F32(2.6)
    updates = [(hist, np.sort(rng.choice(n, n // 2, replace=False)).astype(np.int32))]
    # history 2: points whose lists end in BAD connections
    opt = optimised_ids(fr)
    special = rng.choice(opt, A_SPECIAL, replace=False)
    for p in special:
        d = _dist(X, p)
        far = d > np.sort(d)[A_SPECIAL_NEUTRAL]
        h = X.copy()
        h[far] = X[p] + (X[far] - X[p]) * F32(0.1)
        updates.append((h, np.array([p], np.int32)))
    return dict(tp=tp, frame=fr, sigma=sigma, stretch_th=th, updates=updates, hole_pt=hole_pt, special=special)


# ---- Scene B: the stage-2 retry
B_N, B_SEED, B_NEAR_OPT, B_CLUSTER = 260, 81, 3, 40


@functools.lru_cache(None)
def scene_b():
    """260 map points, sigma such that the whole map lies within 1.4 sigma of every point: no NEUTRAL connection falls below min_weight
    and every list shows its BAD class.  One TRACKED point p (a lost point of the frame): its B_NEAR_OPT nearest map points are optimised,
    the next B_CLUSTER are not in the frame, and one history update of vertex p alone -- in which that cluster and all other optimised
    points had come close to p and gone back -- leaves p's connections to them BAD with their longest distance unchanged.  p's stage-2 list:
    3 NEUTRAL optimised neighbours, 40 BAD connections to points that are not optimised, then the BAD ones to optimised points: the
    eleventh optimised neighbour is entry 51.  The frame's other lost points have untouched lists and end at their 12th entry."""
    tp = S.make_tracking_problem(B_N, B_SEED)
    X = tp["X_prev"]
    n = B_N
    full = np.max([_dist(X, i).max() for i in range(n)])
    sigma = float(F32(full / 1.4))
    st = tp["status"]
    centre = np.median(X, axis=0)
    p = None
    for cand in np.argsort(np.linalg.norm(X - centre, axis=1)):     # the most central point whose nearest three map points were observed with 3D
        by_d = np.argsort(_dist(X, cand))[1:]
        if np.all(st[by_d[:B_NEAR_OPT]] == O.TRACKED_WITH_3D):
            p = int(cand)
            break
    assert p is not None
    cluster = by_d[B_NEAR_OPT:B_NEAR_OPT + B_CLUSTER]
    pool = np.setdiff1d(np.arange(n), cluster)
    fr = make_frame_view(tp, len(pool), 12, B_SEED + 1, pool=pool)
    fr["f_status"][np.isin(fr["f_map"], by_d[:B_NEAR_OPT])] = O.TRACKED_WITH_3D
    fr["f_status"][fr["f_map"] == p] = O.TRACKED                    # tracked in the image, without 3D this frame: a lost neighbour
    opt = optimised_ids(fr)
    came_close = np.concatenate([cluster, np.setdiff1d(opt, by_d[:B_NEAR_OPT])])
    h = X.copy()
    h[came_close] = X[p] + (X[came_close] - X[p]) * F32(0.1)
    return dict(tp=tp, frame=fr, sigma=sigma, stretch_th=tp["graph"]["stretch_th"], updates=[(h, np.array([p], np.int32))], retry_pt=p,
                cluster=cluster)


def dense_oracle_graph(sc):
    """the scene's all-pairs graph with its history, before a2"""
    n = len(sc["tp"]["X_prev"])
    ids = np.arange(n)
    D = RG.DenseGraph(n, sc["sigma"], sc["stretch_th"])
    D.add_edges(sc["tp"]["X_prev"], ids, ids)
    good = []
    for pos, upd in sc["updates"]:
        good.append(np.array([D.update_vertex(pos, int(i)) for i in upd]))
    return D, good


@functools.lru_cache(None)
def dense_oracle_run(which):
    """the oracle's a2 on scene "A" / "B", computed once: (scene, graph before, UpdateVertex returns of the history, result, traces);
    result["graph"] is the graph after.  Shared by the tests: read only."""
    sc = scene_a() if which == "A" else scene_b()
    D, good = dense_oracle_graph(sc)
    before = copy.deepcopy(D)
    tp, fr = sc["tp"], sc["frame"]
    otr = []
    o = O.track_deform_solve(tp["model"], tp["prm"], D, tp["X_prev"], fr["f_map"], fr["f_status"], fr["f_uv"], fr["f_pos"], tp["pose_q"],
                             tp["pose_t"], tp["scale"], otr)
    return sc, before, good, o, otr
