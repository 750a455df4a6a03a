"""The designed cases of f2 (DeformableTriangulation, csrc/nrs_triang.hip k_triangulate) that tests/test_triang_cases_cpu.py vets on
the CPU and tests/test_gpu_triang_cases.py runs on the device.  No GPU and no `nrs` import here.

A case = (flat temporal buffer, candidate ids, min_track, what the case intends, the result of oracle/triang_oracle.py per candidate).
Every buffer is cut out of nrs_synth.make_temporal_buffer (same cameras, same depth of 3 units, same pose scale: the 2e-3 position
tolerance of tests/test_gpu_triang.py is 0.07 % of that depth and holds on that scene only) and then edited by hand; `reproj1` and
`reproj2` are hand-made five-snapshot scenes at the same depth with the same pinhole camera.  A candidate is a map point of the
generator made TRACKED (status 1, no landmark): map points are seen from the first snapshot on, so its track is whatever the case
leaves of it.  The candidates of a case are exactly its ids with status 1, so the same buffer goes through nrs_map_frame.

What the oracle does not return (regulariser edge count, LM iterations, final estimates) is read off the graph it hands to its LM:
`_spy` swaps nrs_oracle.lm_optimize for a recording wrapper while one candidate runs.  The gates before the LM are recomputed here from
the oracle's own primitives, in its order, stopping where it stops.

Neighbour cases (`nb_*`): the last snapshot's keypoints are integers (distances exact in fp32), the candidate's own keypoint there is
rounded to an integer.  The k-th hand-placed id has its landmark in the first 21 - k snapshots, so every potential neighbour
contributes another number of regulariser edges (m (m - 1) / 2 for m snapshots) and a wrong member of the list changes dbg[:, 3].
Ids that are not placed are fillers: eligible map points more than 500 px away.

Not held: a NaN keypoint on a NON-candidate neighbour.  The oracle's sort() of (NaN, id) pairs is not defined, so no case has one.

Named cases of the issue that are not here: none.  `nb_edges_of_n` is eight buffers (`nb_edges_of_<n>_lo`: the candidate at id 0 and
the only neighbour at id n - 1; `_hi`: the candidate at id n - 1 and the only neighbour at id 0).  The vote `bad / n > 0.5` is held at
6 of 10 and at 4 of 10 neighbours: exactly 5 of 10 would put the ratio on its threshold, which the margin rule of the CPU test forbids."""
import contextlib
import functools

import numpy as np

import nrs_synth as S
import triang_oracle as T

O = T.O
F32 = np.float32
DEPTH = 3.0                                                        # the scene's depth in map units (make_temporal_buffer: 3 / median z)


def _copy(tb):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in tb.items()}


# ------------------------------------------------------------------------------------------------ cutting the generator's buffer down
@functools.lru_cache(maxsize=None)
def _scene(model, n_frames, seed, baseline):
    return S.make_temporal_buffer(n_frames, seed, model, baseline=baseline)


def _patch(model, n_frames, seed, k, baseline=0.35):
    """the map point nearest the image centre that is seen in every snapshot, as the candidate (id 0), and its k - 1 nearest map points
    with a full track (ids 1 .. k - 1, by distance in the last snapshot); `X0`: the candidate's landmark per snapshot before it was taken"""
    tb = _scene(model, n_frames, seed, baseline)
    full = np.nonzero(tb["has_kp"].all(0) & (tb["status"] == 0))[0]
    last = tb["kp_xy"][-1].astype(np.float64)
    wh = np.array([640.0, 480.0]) if model == S.PINHOLE else np.array([736.0, 552.0])
    c = full[np.argmin(np.linalg.norm(last[full] - wh / 2, axis=1))]
    order = full[np.argsort(np.linalg.norm(last[full] - last[c], axis=1), kind="stable")][:k]
    assert order[0] == c and len(order) == k
    out = dict(n_frames=n_frames, poses=tb["poses"].copy(), has_kp=tb["has_kp"][:, order].copy(), kp_xy=tb["kp_xy"][:, order].copy(),
               has_lm=tb["has_lm"][:, order].copy(), lm_xyz=tb["lm_xyz"][:, order].copy(), status=np.zeros(k, np.int32), model=model,
               prm=tb["prm"], X0=tb["lm_xyz"][:, c].copy())
    _as_candidate(out, 0)
    return out


def _as_candidate(tb, j):
    tb["status"][j] = 1
    tb["has_lm"][:, j] = False


def _take_frames(tb, frames):
    out = _copy(tb)
    for k in ("poses", "has_kp", "kp_xy", "has_lm", "lm_xyz", "X0"):
        out[k] = tb[k][frames].copy()
    out["n_frames"] = len(frames)
    return out


def _behind(tb, f):
    """every landmark of snapshot f reflected through that snapshot's camera centre: behind the camera at the same distance"""
    C = T.se3_inverse(tb["poses"][f].astype(F32))[4:]
    tb["lm_xyz"][f] = (F32(2) * C - tb["lm_xyz"][f]).astype(F32)


def _five_views(turn_oldest, shift):
    """tests/map_cases.py's two views stretched to five snapshots: the point X at the scene's depth seen by five cameras on a line, 15
    rad_per_pixel of parallax between the oldest and the newest, of which the oldest (or the newest) is turned 0.35 rad about y so that it
    sees X near its border; the oldest keypoint is moved `shift` px across the epipolar line.  The mid-point splits the angular error
    evenly, so the pixel error is larger in the turned camera (1 / cos^2 of the off-axis angle): above 5.991 px^2 there, below it in the
    other one.  Id 0 the candidate, id 1 a static map point 60 px from it."""
    prm = S.HAMLYN_PINHOLE
    rpp = float(1.0 / prm[0])
    q = np.array([0.0, np.sin(0.175), 0.0, np.cos(0.175)])
    c, s_ = np.cos(0.35), np.sin(0.35)
    R = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]])
    X, Ct = np.array([0.1, 0.05, 3.0]), np.array([0.0, 15 * rpp * 3.0, 0.0])

    def proj(p):
        return np.array([prm[0] * p[0] / p[2] + prm[2], prm[1] * p[1] / p[2] + prm[3]])
    poses, kp = [], []
    for f in range(5):
        C = Ct * f / 4.0
        turned = f == (0 if turn_oldest else 4)
        Rf = R if turned else np.eye(3)
        poses.append(np.concatenate([q if turned else [0, 0, 0, 1.0], -Rf @ C]))
        kp.append(proj(Rf @ (X - C)))
    kp[0] = kp[0] + [shift, 0.0]
    tb = dict(n_frames=5, poses=np.array(poses, F32), has_kp=np.ones((5, 2), bool), kp_xy=np.zeros((5, 2, 2), F32), has_lm=np.ones((5, 2), bool),
              lm_xyz=np.zeros((5, 2, 3), F32), status=np.array([1, 0], np.int32), model=S.PINHOLE, prm=prm)
    tb["has_lm"][:, 0] = False
    tb["kp_xy"][:, 0] = kp
    tb["kp_xy"][:, 1] = np.array(kp) + [60.0, 0.0]
    tb["lm_xyz"][:, 1] = X + [0.2, 0.0, 0.0]
    return tb


# ------------------------------------------------------------------------------------------------ hand-placed neighbour lists
NB_F = 21


def _nb_buffer(n, cand_id, placed, model=S.PINHOLE):
    """n ids on the 21-snapshot scene.  placed: (id, (dx, dy), kind) in the last snapshot, relative to the candidate; kind: "ok" an
    eligible map point, "status" a map point whose status is not 0, "no_kp" a map point without a keypoint in the last snapshot, "dup"
    the candidate's own column under another id with status 1 (a second candidate at the same pixel)."""
    src = _patch(model, NB_F, 7, 24, baseline=0.3)
    assert len(placed) <= NB_F - 1 and len({p[0] for p in placed} | {cand_id}) == len(placed) + 1
    tb = dict(n_frames=NB_F, poses=src["poses"].copy(), has_kp=np.zeros((NB_F, n), bool), kp_xy=np.zeros((NB_F, n, 2), F32),
              has_lm=np.zeros((NB_F, n), bool), lm_xyz=np.zeros((NB_F, n, 3), F32), status=np.zeros(n, np.int32), model=model, prm=src["prm"])

    def put(dst, col):
        for k in ("has_kp", "kp_xy", "has_lm", "lm_xyz"):
            tb[k][:, dst] = src[k][:, col]
    home = np.round(src["kp_xy"][-1, 0]).astype(F32)
    for j in range(n):                                             # fillers: eligible, beyond 500 px
        put(j, 23)
        tb["kp_xy"][-1, j] = home + np.array([600.0 + j, 7.0], F32)
    put(cand_id, 0)
    tb["kp_xy"][-1, cand_id] = home
    tb["status"][cand_id] = 1
    for k, (j, off, kind) in enumerate(placed):
        put(j, 0 if kind == "dup" else k + 1)
        tb["kp_xy"][-1, j] = home + np.array(off, F32)
        if kind == "dup":
            tb["status"][j] = 1
            continue
        tb["has_lm"][:, j] = np.arange(NB_F) < NB_F - k            # another edge count per placed id; all of them in the first snapshot
        if kind == "status":
            tb["status"][j] = 2
        elif kind == "no_kp":
            tb["has_kp"][-1, j] = False
    return tb


def _ok(ids, offs):
    return [(j, o, "ok") for j, o in zip(ids, offs)]


_TIE = [(30, 40), (-30, 40), (30, -40), (-30, -40), (40, 30), (-40, 30), (40, -30), (-40, -30), (50, 0), (-50, 0), (0, 50), (0, -50),
        (14, 48), (-14, 48), (14, -48), (-14, -48)]               # sixteen offsets at exactly 50 px
_TIE_IDS = [131, 5, 69, 3, 199, 67, 10, 133, 20, 138, 30, 150, 40, 160, 196, 198]   # lanes 3 (3, 67, 131) and 5 (5, 69, 133) three times


def _nb_case(name):
    """(tb, {candidate: intended neighbour list, None = too close}, {candidate: intended code or None = any that is not TR_CLOSE})"""
    if name == "nb_one":
        return _nb_buffer(40, 7, _ok([21], [(300, 400)])), {7: [21]}, {7: None}
    if name == "nb_none_far":
        return _nb_buffer(40, 7, _ok([21], [(301, 400)])), {7: []}, {7: T.E_CLOSE}
    if name == "nb_at_20":
        return _nb_buffer(40, 7, _ok([21], [(12, 16)])), {7: [21]}, {7: None}
    if name == "nb_below_20":
        return _nb_buffer(40, 7, _ok([21], [(12, 15)])), {7: None}, {7: T.E_CLOSE}
    if name == "nb_ineligible_close":
        placed = _ok([30, 2, 17], [(30, 0), (0, -45), (-60, 11)]) + [(5, (5, 5), "status"), (9, (3, -4), "no_kp"), (12, (0, 0), "dup")]
        return _nb_buffer(40, 7, placed), {7: [30, 2, 17], 12: [30, 2, 17]}, {7: None, 12: None}
    if name in ("nb_ties_lanes", "nb_ties_lanes_kb8"):
        # two nearer ones at high ids (25 and 30 px), then the sixteen at 50 px: the nine lowest ids of the tie are taken, the 11th place
        # goes to id 131 (lane 3, third stride) and id 133 (lane 5, third stride) is the first one left out
        placed = _ok([190, 180], [(15, 20), (-18, 24)]) + _ok(_TIE_IDS, _TIE)
        want = [190, 180, 3, 5, 10, 20, 30, 40, 67, 69, 131]
        return _nb_buffer(200, 70, placed, S.KB8 if name.endswith("kb8") else S.PINHOLE), {70: want}, {70: None}
    if name in ("nb_eleven", "nb_twelve"):
        m = 11 if name == "nb_eleven" else 12
        ids = [37, 2, 66, 19, 130, 64, 5, 129, 63, 1, 65, 0][:m]    # id order is not distance order; ids around the lane strides
        offs = [(21 + 4 * k, 0) if k % 2 else (0, -(21 + 4 * k)) for k in range(m)]
        return _nb_buffer(140, 70, _ok(ids, offs)), {70: ids[:11]}, {70: None}
    if name.startswith("nb_edges_of_"):
        n, side = int(name.split("_")[3]), name.split("_")[4]
        c, j = (0, n - 1) if side == "lo" else (n - 1, 0)
        return _nb_buffer(n, c, _ok([j], [(-33, 56)])), {c: [j]}, {c: None}
    raise KeyError(name)


NB_CASES = ["nb_one", "nb_none_far", "nb_at_20", "nb_below_20", "nb_ineligible_close", "nb_ties_lanes", "nb_ties_lanes_kb8", "nb_eleven",
            "nb_twelve"] + ["nb_edges_of_%d_%s" % (n, s) for n in (2, 64, 65, 129) for s in ("lo", "hi")]
CODE_CASES = ["reproj1", "reproj2", "parallax", "short", "short_kb8", "no_neighbour", "neg_depth", "first_bad_decides_a", "first_bad_decides_b",
              "bad_neighbours", "half_bad_neighbours", "bad_error"]
SHAPE_CASES = ["track_1", "track_2", "frames_1", "frames_2", "track_21_gappy", "track_21_gappy_kb8", "first_frame_blind", "no_edges",
               "no_edges_kb8"]
CASES = NB_CASES + CODE_CASES + SHAPE_CASES


def _drift(tb, ids, step=0.6):
    """a spurious velocity of `step` units per snapshot on the landmarks of `ids`, in opposite directions two by two: the sum over the
    neighbours is unchanged in every snapshot (so are the depth seeds and the solved flow), every edge of such a neighbour is off by at
    least `step` units -- 100 step^2 = 36 against the 7.815 of the vote"""
    dirs = [np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]), np.array([0.6, 0.0, 0.8])]
    assert len(ids) % 2 == 0
    for k, j in enumerate(ids):
        v = dirs[k // 2] * (1.0 if k % 2 == 0 else -1.0)
        for f in range(tb["n_frames"]):
            tb["lm_xyz"][f, j] = (tb["lm_xyz"][f, j] + F32(step * f) * v.astype(F32)).astype(F32)


def _build(name):
    """(tb, min_track, {candidate: intended code, None = any that is not TR_CLOSE}, {candidate: intended neighbour list} or None)"""
    if name in NB_CASES:
        tb, nb, want = _nb_case(name)
        return tb, 5, want, nb
    if name in ("reproj1", "reproj2"):
        # 5 px into the turned oldest camera: 6.36 px^2 there (4.70 in the newest, not reached).  4.6 px into the unturned oldest camera
        # with the newest one turned: 5.4 px^2 in the oldest, whose gate comes first and passes, and more in the newest
        tb = _five_views(True, 5.0) if name == "reproj1" else _five_views(False, 4.6)
        return tb, 5, {0: T.E_REPROJ1 if name == "reproj1" else T.E_REPROJ2}, None
    if name == "parallax":
        return _patch(S.PINHOLE, 5, 8, 12, baseline=0.002), 5, {0: T.E_PARALLAX}, None
    if name in ("short", "short_kb8"):
        tb = _patch(S.KB8 if name == "short_kb8" else S.PINHOLE, 6, 5, 14)
        _as_candidate(tb, 1)
        tb["has_kp"][:2, 0] = False                                # four vertices: min_track - 1
        tb["has_kp"][:1, 1] = False                                # five: exactly min_track
        return tb, 5, {0: T.E_SHORT, 1: T.OK}, None
    if name in ("no_neighbour", "neg_depth", "first_bad_decides_a", "first_bad_decides_b", "first_frame_blind"):
        tb = _patch(S.PINHOLE, 5, 3, 12)
        if name == "no_neighbour":
            tb["has_lm"][2] = False
            return tb, 5, {0: T.E_NO_NEIGHBOUR}, None
        if name == "first_frame_blind":
            tb["has_lm"][0] = False
            return tb, 5, {0: T.E_NO_NEIGHBOUR}, None
        if name == "neg_depth":
            _behind(tb, 2)
            return tb, 5, {0: T.E_NEG_DEPTH}, None
        neg, none = (1, 3) if name == "first_bad_decides_a" else (3, 1)
        _behind(tb, neg)
        tb["has_lm"][none] = False
        return tb, 5, {0: T.E_NEG_DEPTH if neg < none else T.E_NO_NEIGHBOUR}, None
    if name in ("bad_neighbours", "half_bad_neighbours"):
        tb = _patch(S.PINHOLE, 5, 3, 11)                           # ten neighbours, all with a landmark in every snapshot
        tb["has_lm"][:, 1:] = True
        _drift(tb, [2, 9, 4, 7, 1, 10] if name == "bad_neighbours" else [2, 9, 4, 7])
        return tb, 5, {0: T.E_BAD_NEIGHBOURS if name == "bad_neighbours" else T.OK}, None
    if name == "bad_error":
        # Static neighbours want all 21 vertices at one world point.  The numeric Jacobian of the reprojection is zero almost everywhere,
        # so the LM follows the regulariser alone and a step is kept whenever the total chi2 falls: the pull of 11 x 20 edges at weight
        # 100 per vertex against 4 px^-2 x (255 px per unit)^2 moves a vertex some per cent of the way.  Seven snapshots (three oldest,
        # four newest) see the point where it is, the fourteen in between see it 200 px (0.78 units) to the side: the edges inside a group
        # stay good (112 of 210 pairs, so the neighbour vote keeps it at 0.467), every vertex ends several px off its ray.
        tb = _patch(S.PINHOLE, 21, 7, 12, baseline=0.3)
        tb["has_lm"][:, 1:] = True
        tb["lm_xyz"][:] = tb["lm_xyz"][-1]                         # static neighbours: every flow is exactly zero
        X = tb["X0"][-1]
        for f in range(21):                                        # the candidate: a static point too, seen without noise ...
            tb["kp_xy"][f, 0] = T.project_pt(tb["model"], tb["prm"], T.se3_mul_point(tb["poses"][f].astype(F32), X))
        tb["kp_xy"][3:17, 0] += np.array([200.0, 0.0], F32)        # ... but 200 px off in fourteen middle snapshots
        return tb, 5, {0: T.E_BAD_ERROR}, None
    if name in ("track_1", "track_2", "frames_1", "frames_2"):
        tb = _patch(S.PINHOLE, 5, 3, 12)
        if name == "track_1":
            tb["has_kp"][:4, 0] = False
        elif name == "track_2":
            tb["has_kp"][1:4, 0] = False                           # the oldest and the newest snapshot: enough parallax
        elif name == "frames_1":
            tb = _take_frames(tb, [4])
        else:
            tb = _take_frames(tb, [0, 4])
        return tb, 1, {0: T.OK}, None
    if name in ("track_21_gappy", "track_21_gappy_kb8"):
        tb = _patch(S.KB8 if name.endswith("kb8") else S.PINHOLE, 21, 7, 13, baseline=0.3)
        tb["has_kp"][1::2, 0] = False                              # fr[] = 0, 2, ..., 20
        return tb, 5, {0: T.OK}, None
    if name in ("no_edges", "no_edges_kb8"):
        tb = _patch(S.KB8 if name.endswith("kb8") else S.PINHOLE, 5, 3, 3)
        tb["has_lm"][:, 1] = [True, False, False, False, False]    # A: the first snapshot only
        tb["has_lm"][:, 2] = [False, True, True, True, True]       # B: every other one
        return tb, 5, {0: T.OK}, None
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ the oracle, and what it decides on
@contextlib.contextmanager
def _spy():
    seen = {}
    real = O.lm_optimize

    def lm(G, iterations, trace=None, solver=O.solve_spd):
        seen["G"] = G
        seen["iters"] = real(G, iterations, trace, solver)
        return seen["iters"]
    O.lm_optimize = lm
    try:
        yield seen
    finally:
        O.lm_optimize = real


def neighbour_distances(tb, c):
    """the distances GetClosestMapPointsToFeature compares with 20 and 500, as the oracle computes them"""
    last = tb["n_frames"] - 1
    kp = tb["kp_xy"][last, c]
    out = []
    for j in np.where(tb["has_kp"][last] & (tb["status"] == 0))[0]:
        if j != c:
            dx, dy = np.float64(kp[0] - tb["kp_xy"][last, j, 0]), np.float64(kp[1] - tb["kp_xy"][last, j, 1])
            out.append(float(F32(np.sqrt(dx * dx + dy * dy))))
    return out


def gates_before(tb, c, min_track):
    """(name, quantity, threshold) of every gate the oracle evaluates before its LM, in its order, up to the one that stops it"""
    model, prm = tb["model"], tb["prm"]
    g = []
    for d in neighbour_distances(tb, c):
        g += [("neighbour_20", d, 20.0), ("neighbour_500", d, 500.0)]
    nb = T.closest_map_points(tb, c)
    frames = [f for f in range(tb["n_frames"]) if tb["has_kp"][f, c]]
    if not nb or len(frames) < min_track:
        return g
    P = tb["poses"].astype(F32)
    first, lastf = frames[0], frames[-1]
    kpc, kpp = tb["kp_xy"][first, c], tb["kp_xy"][lastf, c]
    cur, prev = T._normalized(T.unproject_f32(model, prm, *kpc)), T._normalized(T.unproject_f32(model, prm, *kpp))
    X = T.triangulate_mid_point(prev, cur, P[lastf], P[first])
    for Tm, kp, nm in ((P[first], kpc, "reproj1"), (P[lastf], kpp, "reproj2")):
        uv = T.project_pt(model, prm, T.se3_mul_point(Tm, X))
        ex, ey = F32(kp[0]) - uv[0], F32(kp[1]) - uv[1]
        e = float(F32(ex * ex + ey * ey))
        g.append((nm, e, 5.991))
        if e > 5.991:
            return g
    par = float(T.rays_parallax((X - T.se3_inverse(P[first])[4:]).astype(F32), (X - T.se3_inverse(P[lastf])[4:]).astype(F32)))
    g.append(("parallax", par, 0.0025 * 5.0))
    if par < 0.0025 * 5.0:
        return g
    for f in frames:
        z = [T.se3_mul_point(P[f], tb["lm_xyz"][f, j])[2] for j in nb if tb["has_lm"][f, j]]
        if not z:
            return g
        depth = F32(0)
        for v in z:
            depth = F32(depth + v)
        depth = float(F32(depth / F32(len(z))))
        g.append(("seed_depth", depth, 0.0))
        if depth < 0:
            return g
    return g


def on_threshold(gate, exact_px, rel=1e-3):
    """True when a gate quantity is closer than `rel` (relative) to its threshold.  The depth's threshold is 0: its margin is relative to
    the scene's depth.  A NaN is decided by its being a NaN.  exact_px: the case's keypoints are integers, so a neighbour distance that
    EQUALS 20 or 500 is exact and allowed."""
    name, q, th = gate
    if np.isnan(q):
        return False
    if exact_px and name.startswith("neighbour") and q == th:
        return False
    return abs(q - th) < rel * (abs(th) if th != 0 else DEPTH)


def run_oracle(tb, c, min_track):
    """dict: status, xyz, gates; past the seeds also edges (regulariser edge count), iters, trials, all_failed (no solve succeeded)"""
    trace = []
    with np.errstate(all="ignore"), _spy() as seen:
        st, xyz = T.deformable_triangulation(tb, c, tb["model"], tb["prm"], min_track, trace)
        before = gates_before(tb, c, min_track)                    # (a one-vertex track: the mid-point of a ray with itself is 0 / 0)
    r = dict(status=int(st), xyz=np.asarray(xyz, F32), gates=before, edges=None, trace=trace)
    if "G" in seen:
        G = seen["G"]
        rep, reg = G.groups
        V = rep.n
        r.update(edges=int(reg.n), iters=int(seen["iters"]), trials=len(trace), all_failed=all(not t["ok"] for t in trace))
        if reg.n:
            e = reg.residual(G, np.arange(reg.n))
            bad = int(np.sum(reg.info * np.sum(e * e, axis=1) > float(F32(7.815))))
            r["gates"].append(("bad_edge_ratio", float(F32(bad) / F32(reg.n)), 0.5))
            if st == T.E_BAD_NEIGHBOURS:
                return r
        rr = rep.residual(G, np.arange(V))
        nbad = int(np.sum(rep.info * np.sum(rr * rr, axis=1) > 5.99 * 10))
        r["gates"].append(("bad_frame_ratio", float(F32(nbad) / F32(V)), 0.5))
    return r


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(tb, cand, min_track, want {candidate: code or None}, want_nb {candidate: list} or None, exact_px, ref [run_oracle per candidate])"""
    tb, min_track, want, want_nb = _build(name)
    tb.pop("X0", None)
    cand = np.nonzero(tb["status"] == 1)[0].astype(np.int32)
    assert sorted(want) == cand.tolist() and tb["has_kp"][-1, cand].all()
    ref = [run_oracle(tb, int(c), min_track) for c in cand]
    return dict(tb=tb, cand=cand, min_track=min_track, want=want, want_nb=want_nb, exact_px=name in NB_CASES, ref=ref)
