"""Seeded synthetic problems for the NR-SLAM hot path (BASELINE.json configs).

The build's own generator: scene layout follows the recipe of SURVEY.md 8(d) -- a smooth
endoscopic-like surface, an arc of keyframe poses looking at its centroid, a low-frequency
per-keyframe deformation field, noisy observations with a few gross outliers, and a
deformation graph whose edges carry {weight, first_distance, status} exactly like
RegularizationGraph::Edge (reference modules/map/regularization_graph.h:49-59).

Everything the C-ABI consumes is produced here as flat arrays; nothing in this file depends on
the oracle.
"""
import numpy as np
from scipy.spatial import cKDTree

F32 = np.float32

PINHOLE, KB8 = 0, 1
HAMLYN_PINHOLE = np.array([766.380279, 766.380279, 304.8638076782227, 258.3343734741211, 0, 0, 0, 0], F32)
ENDOMAPPER_KB8 = np.array([358.6052, 358.7408, 367.6783, 276.3991,
                           -0.1389272, -0.001239606, 0.0009125824, -4.071615e-05], F32)

GRAPH_NEUTRAL, GRAPH_BAD = 2, 3

CONFIGS = {
    # name: (n_points, n_keyframes, seed, camera)
    "C2": (5000, 20, 1, PINHOLE),
    "C3": (10000, 50, 2, PINHOLE),
    "C4": (50000, 200, 3, PINHOLE),
    "C5": (100000, 200, 4, KB8),
}


def _project(model, prm, p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    if model == PINHOLE:
        return np.stack([prm[0] * x / z + prm[2], prm[1] * y / z + prm[3]], 1)
    r = np.sqrt(x * x + y * y)
    th = np.arctan2(r, z)
    psi = np.arctan2(y, x)
    rd = th + prm[4] * th ** 3 + prm[5] * th ** 5 + prm[6] * th ** 7 + prm[7] * th ** 9
    return np.stack([prm[0] * rd * np.cos(psi) + prm[2], prm[1] * rd * np.sin(psi) + prm[3]], 1)


def _look_at(C, target):
    z = target - C
    z /= np.linalg.norm(z)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])            # rows = camera axes in world  => p_cam = R (X - C)
    return R, -R @ C


def _R_to_quat(R):
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2
        q = np.zeros(4)
        q[i] = 0.25 * s
        q[3] = (R[k, j] - R[j, k]) / s
        q[j] = (R[j, i] + R[i, j]) / s
        q[k] = (R[k, i] + R[i, k]) / s
    if q[3] < 0:
        q = -q
    return q / np.linalg.norm(q)


def _small_rot(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def surface_points(n, rng, model):
    """Rest shape in mm."""
    if model == PINHOLE:
        x = rng.uniform(-22, 22, n)
        y = rng.uniform(-17, 17, n)
        z = 60 + 8 * np.sin(x / 15) * np.cos(y / 12)
        nrm = np.stack([-(8 / 15) * np.cos(x / 15) * np.cos(y / 12),
                        (8 / 12) * np.sin(x / 15) * np.sin(y / 12), np.ones(n)], 1)
    else:
        # colon-like tube of radius 15 mm around the optical axis, theta in ~10..80 deg
        ang = rng.uniform(0, 2 * np.pi, n)
        z = rng.uniform(3.0, 80.0, n)
        rad = 15 + 1.5 * np.sin(3 * ang) * np.cos(z / 9)
        x, y = rad * np.cos(ang), rad * np.sin(ang)
        nrm = np.stack([-np.cos(ang), -np.sin(ang), np.zeros(n)], 1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.stack([x, y, z], 1), nrm


def _weight(d, sigma):
    """InterpolationWeight (reference geometry_toolbox.cc:26-28): float argument, exp in double,
    result rounded to float (include/nrs.h nrs_graph)."""
    d = np.asarray(d, F32)
    sigma = F32(sigma)
    arg = (-(d * d) / (F32(2) * sigma * sigma)).astype(F32)
    return np.exp(arg.astype(np.float64)).astype(F32)


def build_graph(X, sigma, knn=16, stretch_th=1.1):
    """Deformation graph over points X (fp32, map units) in the flat wire form of
    RegularizationGraph (reference regularization_graph.h:49-59,79,89):
      * undirected edges e: e_i < e_j, first_distance d0, max/min distance, weight, status
      * raw CSR per point, neighbours in ascending index order (= btree_map ID order), each
        directed entry naming its undirected edge (eid).
    Candidate edges = union of k-nearest-neighbour pairs whose initial weight reaches min_weight
    (the reference starts from all pairs, map.cc:148-166; pairs below min_weight can never be
    returned by GetEdges because weights only decrease, regularization_graph.cc:113)."""
    X = np.asarray(X, F32)
    n = len(X)
    sigma = F32(sigma)
    min_w = _weight(F32(float(sigma) * 1.5), sigma)
    k = min(knn + 1, n)
    tree = cKDTree(X.astype(np.float64))
    _, nn = tree.query(X.astype(np.float64), k=k)
    src = np.repeat(np.arange(n), k - 1)
    dst = nn[:, 1:].ravel()
    a, b = np.minimum(src, dst), np.maximum(src, dst)
    keep = a != b
    pairs = np.unique(np.stack([a[keep], b[keep]], 1), axis=0)
    rel = X[pairs[:, 1]] - X[pairs[:, 0]]
    d = np.sqrt((rel[:, 0] * rel[:, 0] + rel[:, 1] * rel[:, 1] + rel[:, 2] * rel[:, 2]).astype(F32)).astype(F32)
    w = _weight(d, sigma)
    ok = w >= min_w
    pairs, d, w = pairs[ok], d[ok], w[ok]
    ne = len(pairs)
    row = np.concatenate([pairs[:, 0], pairs[:, 1]])
    col = np.concatenate([pairs[:, 1], pairs[:, 0]])
    eid = np.concatenate([np.arange(ne), np.arange(ne)])
    order = np.lexsort((col, row))
    row, col, eid = row[order], col[order], eid[order]
    rowptr = np.zeros(n + 1, np.int64)
    np.add.at(rowptr, row + 1, 1)
    rowptr = np.cumsum(rowptr).astype(np.int32)
    g = dict(n=n, rowptr=rowptr, col=col.astype(np.int32), eid=eid.astype(np.int32),
             e_ij=pairs.astype(np.int32), e_d0=d.copy(), e_w=w.copy(), e_max=d.copy(), e_min=d.copy(),
             e_status=np.full(ne, GRAPH_NEUTRAL, np.int32), min_w=float(min_w), sigma=float(sigma),
             stretch_th=float(stretch_th))
    g.update(ordered_neighbours(g))
    return g


def ordered_neighbours(g):
    """NumPy twin of GetEdges (reference regularization_graph.cc:61-87) on the flat graph: per
    point, neighbours sorted by (status asc, weight desc, index asc) and cut at the first weight
    below min_weight.  Used to build inputs; the product's version is nrs_graph_select_neighbours."""
    rowptr, col, eid = g["rowptr"], g["col"], g["eid"]
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    w = g["e_w"][eid]
    st = g["e_status"][eid]
    order = np.lexsort((col, -w.astype(np.float64), st, row))
    r2, c2, e2, w2 = row[order], col[order], eid[order], w[order]
    low = w2 < np.float32(g["min_w"])
    # cut every row at its first low-weight entry
    pos = np.arange(len(r2)) - rowptr[r2]
    first_low = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(first_low, r2[low], pos[low])
    keep = pos < first_low[r2]
    r2, c2, e2 = r2[keep], c2[keep], e2[keep]
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, r2 + 1, 1)
    return dict(o_rowptr=np.cumsum(rp).astype(np.int32), o_col=c2.astype(np.int32), o_eid=e2.astype(np.int32))


def ordered_view(g):
    """Ordered neighbour lists with per-entry weight / first_distance / status (input of
    nrs_dba_build_edges and of the oracle's dba_build)."""
    e = g["o_eid"]
    return dict(rowptr=g["o_rowptr"], col=g["o_col"], w=g["e_w"][e], d0=g["e_d0"][e], status=g["e_status"][e])


def make_scene(n_points, n_kf, seed, model=PINHOLE, dropout=0.05, outlier_frac=0.02,
               img_wh=(640, 480), knn=16):
    """Full synthetic sequence: rest shape, per-keyframe truth, observations, graph.
    Positions are in *map units* (mm * scale, scale = 3/median depth: reference
    tracking.cc:156-157)."""
    rng = np.random.default_rng(seed)
    prm = HAMLYN_PINHOLE if model == PINHOLE else ENDOMAPPER_KB8
    if model == KB8:
        img_wh = (736, 552)
    Xmm, nrm = surface_points(n_points, rng, model)
    centroid = Xmm.mean(0)
    if model == PINHOLE:
        depth0 = Xmm[:, 2]
    else:
        depth0 = Xmm[:, 2]
    scale = F32(3.0) / F32(np.median(depth0))
    sigma = F32(3.0) * F32(np.std(depth0.astype(F32))) * scale      # tracking.cc:159-160,200
    poses_R, poses_t = [], []
    phis = np.linspace(-1.0, 1.0, n_kf) if n_kf > 1 else np.array([0.0])
    for phi in phis:
        if model == PINHOLE:
            C = np.array([6.0 * phi, 2.0 * np.sin(np.pi * phi), 0.0])
            R, t = _look_at(C, centroid)
        else:
            C = np.array([1.5 * phi, 1.0 * np.sin(np.pi * phi), 2.0 * phi])
            R = _small_rot(np.array([0.03 * phi, -0.04 * phi, 0.02 * phi]))
            t = -R @ C
        poses_R.append(R)
        poses_t.append(t)
    # per-keyframe true positions (mm): low-frequency deformation along the normal
    obs = []
    Xk_true = []
    A = 1.5
    for k in range(n_kf):
        amp = A * np.sin(2 * np.pi * k / 20.0) * (0.6 + 0.4 * np.sin(Xmm[:, 0] / 11.0 + 0.3) * np.cos(Xmm[:, 1] / 9.0))
        Xk = Xmm + (amp + rng.normal(0, 0.05, n_points))[:, None] * nrm
        Xk_true.append(Xk)
        pc = Xk @ poses_R[k].T + poses_t[k]
        uv = _project(model, prm.astype(np.float64), pc)
        vis = (pc[:, 2] > 1.0) & (uv[:, 0] > 12) & (uv[:, 0] < img_wh[0] - 12) & (uv[:, 1] > 12) & (uv[:, 1] < img_wh[1] - 12)
        vis &= rng.uniform(size=n_points) > dropout
        uv = uv + rng.normal(0, 0.5, uv.shape)
        out = rng.uniform(size=n_points) < outlier_frac
        uv[out] = np.stack([rng.uniform(12, img_wh[0] - 12, out.sum()), rng.uniform(12, img_wh[1] - 12, out.sum())], 1)
        obs.append((np.where(vis)[0].astype(np.int32), uv[vis].astype(F32)))
    s = float(scale)
    X0 = (Xmm * s).astype(F32)
    graph = build_graph(X0, sigma, knn)
    return dict(model=model, prm=prm, scale=float(scale), sigma=float(sigma), X0=X0,
                Xk_true=[(x * s) for x in Xk_true], poses_R=poses_R,
                poses_t=[t * s for t in poses_t], obs=obs, graph=graph, rng=rng, img_wh=img_wh)


def make_dba_problem(name_or_n, n_kf=None, seed=None, model=PINHOLE, pose_noise=(0.002, 0.01),
                     lm_noise=0.004, **kw):
    """Flat input of nrs_dba_* for one windowed deformable BA (reference
    LocalDeformableBundleAdjustment, g2o_optimization.cc:880-1161), with the window cap lifted
    to n_kf keyframes.  Edge lists are NOT built here: the product's host builder
    (nrs_dba_build_edges) and the oracle's dba_build both derive them from (kf_points, graph)."""
    if isinstance(name_or_n, str):
        n_points, n_kf, seed, model = CONFIGS[name_or_n]
    else:
        n_points = name_or_n
    sc = make_scene(n_points, n_kf, seed, model, **kw)
    rng = sc["rng"]
    poses_q, poses_t = [], []
    for k in range(n_kf):
        dR = _small_rot(rng.normal(0, pose_noise[0], 3))
        R = dR @ sc["poses_R"][k]
        t = dR @ sc["poses_t"][k] + rng.normal(0, pose_noise[1], 3)
        q = _R_to_quat(R).astype(F32).astype(np.float64)          # boundary hands over SE3f
        poses_q.append(q)
        poses_t.append(t.astype(F32).astype(np.float64))
    kf_points = [o[0] for o in sc["obs"]]
    lm_uv = np.concatenate([o[1] for o in sc["obs"]]).astype(F32)
    lm_xyz = np.concatenate([sc["Xk_true"][k][kf_points[k]] + rng.normal(0, lm_noise, (len(kf_points[k]), 3))
                             for k in range(n_kf)]).astype(F32)
    lm_kf = np.concatenate([np.full(len(kf_points[k]), k, np.int32) for k in range(n_kf)])
    lm_pt = np.concatenate(kf_points).astype(np.int32)
    return dict(model=sc["model"], prm=sc["prm"], scale=sc["scale"], n_kf=n_kf, n_points=n_points,
                poses_q=np.array(poses_q), poses_t=np.array(poses_t), kf_points=kf_points,
                lm_xyz=lm_xyz, lm_kf=lm_kf, lm_pt=lm_pt, lm_uv=lm_uv, graph=sc["graph"],
                nbr=ordered_view(sc["graph"]), scene=sc)


def make_tracking_problem(n_points, seed, model=PINHOLE, frame=3, lost_frac=0.03, **kw):
    """One tracked frame for nrs_pose_only_solve / nrs_track_deform_solve (reference
    CameraPoseOptimization / CameraPoseAndDeformationOptimization, g2o_optimization.cc:50-557):
    previous positions X0 (= last estimate), current observations, pose seed = previous pose."""
    sc = make_scene(n_points, frame + 1, seed, model, **kw)
    rng = sc["rng"]
    idx, uv = sc["obs"][frame]
    prev = sc["Xk_true"][frame - 1] + rng.normal(0, 0.002, (n_points, 3))
    R = _small_rot(rng.normal(0, 0.003, 3)) @ sc["poses_R"][frame - 1]
    t = sc["poses_t"][frame - 1] + rng.normal(0, 0.01, 3)
    status = np.full(n_points, 3, np.int32)             # BAD unless observed
    status[idx] = 0                                     # TRACKED_WITH_3D
    lost = idx[rng.uniform(size=len(idx)) < lost_frac]
    status[lost] = 1                                    # TRACKED (no 3D this frame) -> "lost" neighbours
    uv_full = np.zeros((n_points, 2), F32)
    uv_full[idx] = uv
    return dict(model=sc["model"], prm=sc["prm"], scale=sc["scale"], n_points=n_points,
                status=status, uv=uv_full, X_prev=prev.astype(F32),
                pose_q=_R_to_quat(R).astype(F32).astype(np.float64),
                pose_t=t.astype(F32).astype(np.float64), graph=sc["graph"], scene=sc)


def make_lk_sequence(n_points=500, seed=5, wh=(640, 480), flow_px=6.0):
    """Synthetic LK pair (SURVEY.md 8d "LK"): band-limited noise texture, second frame = smooth warp
    (<= flow_px) with gain 0.8-1.2 and bias +-10; points at high-gradient locations."""
    rng = np.random.default_rng(seed)
    w, h = wh
    tex = np.zeros((h + 64, w + 64), np.float64)
    for sc, amp in ((4, 28.0), (8, 36.0), (16, 30.0), (32, 22.0)):
        gh, gw = (h + 64) // sc + 3, (w + 64) // sc + 3
        g = rng.normal(0, 1, (gh, gw))
        yy = np.arange(h + 64) / sc
        xx = np.arange(w + 64) / sc
        y0, x0 = np.floor(yy).astype(int), np.floor(xx).astype(int)
        fy, fx = (yy - y0)[:, None], (xx - x0)[None, :]
        fy, fx = fy * fy * (3 - 2 * fy), fx * fx * (3 - 2 * fx)
        tex += amp * ((g[np.ix_(y0, x0)] * (1 - fx) + g[np.ix_(y0, x0 + 1)] * fx) * (1 - fy)
                      + (g[np.ix_(y0 + 1, x0)] * (1 - fx) + g[np.ix_(y0 + 1, x0 + 1)] * fx) * fy)
    tex = 120 + tex

    def render(flow_fn, gain, bias):
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
        dx, dy = flow_fn(xs, ys)
        sx, sy = xs - dx + 32, ys - dy + 32                 # backward warp
        x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
        fx, fy = sx - x0, sy - y0
        x0 = np.clip(x0, 0, w + 62)
        y0 = np.clip(y0, 0, h + 62)
        v = (tex[y0, x0] * (1 - fx) + tex[y0, x0 + 1] * fx) * (1 - fy) + (tex[y0 + 1, x0] * (1 - fx) + tex[y0 + 1, x0 + 1] * fx) * fy
        return np.clip(np.rint(gain * v + bias), 0, 255).astype(np.uint8)

    zero = lambda xs, ys: (np.zeros_like(xs), np.zeros_like(ys))
    ax, ay = rng.uniform(0.5, 1.0) * flow_px, rng.uniform(0.5, 1.0) * flow_px
    flow = lambda xs, ys: (ax * np.sin(xs / 90.0 + 0.3) * np.cos(ys / 70.0), ay * np.cos(xs / 80.0) * np.sin(ys / 60.0 + 0.5))
    im0 = render(zero, 1.0, 0.0)
    im1 = render(flow, rng.uniform(0.8, 1.2), rng.uniform(-10, 10))
    # corners: strongest gradient-energy responses on a coarse grid, away from the border
    g = im0.astype(np.float64)
    gx = np.zeros_like(g); gy = np.zeros_like(g)
    gx[:, 1:-1] = g[:, 2:] - g[:, :-2]
    gy[1:-1, :] = g[2:, :] - g[:-2, :]
    e = gx * gx + gy * gy
    pts = []
    cell = max(8, int(np.sqrt(w * h / max(1, n_points)) * 0.9))
    for y in range(30, h - 30 - cell, cell):
        for x in range(30, w - 30 - cell, cell):
            blk = e[y:y + cell, x:x + cell]
            k = np.unravel_index(np.argmax(blk), blk.shape)
            pts.append((x + k[1] + rng.uniform(-0.4, 0.4), y + k[0] + rng.uniform(-0.4, 0.4)))
    pts = np.array(pts, F32).reshape(-1, 2)                 # (no point at all on an image too small for the 30 px margin)
    if len(pts) > n_points:
        pts = pts[rng.choice(len(pts), n_points, replace=False)]
    fx, fy = flow(pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64))
    truth = pts + np.stack([fx, fy], 1).astype(F32)
    return dict(im0=im0, im1=im1, pts=pts, truth=truth)


def _texture(h, w, rng, margin=32):
    tex = np.zeros((h + 2 * margin, w + 2 * margin), np.float64)
    for sc, amp in ((4, 28.0), (8, 36.0), (16, 30.0), (32, 22.0)):
        gh, gw = (h + 2 * margin) // sc + 3, (w + 2 * margin) // sc + 3
        g = rng.normal(0, 1, (gh, gw))
        yy = np.arange(h + 2 * margin) / sc
        xx = np.arange(w + 2 * margin) / sc
        y0, x0 = np.floor(yy).astype(int), np.floor(xx).astype(int)
        fy, fx = (yy - y0)[:, None], (xx - x0)[None, :]
        fy, fx = fy * fy * (3 - 2 * fy), fx * fx * (3 - 2 * fx)
        tex += amp * ((g[np.ix_(y0, x0)] * (1 - fx) + g[np.ix_(y0, x0 + 1)] * fx) * (1 - fy)
                      + (g[np.ix_(y0 + 1, x0)] * (1 - fx) + g[np.ix_(y0 + 1, x0 + 1)] * fx) * fy)
    return 120 + tex


def make_frame_sequence(n_points=400, n_frames=6, seed=9, model=PINHOLE, step=0.012, occluders=2, half_size=False, deform_amp=1.2):
    """A short consistent monocular sequence for the frame-loop harness: a deforming
    surface seen by a slowly moving camera.  Frame 0 is the initialised map (keyframe): 3D positions
    (truth + noise, map units), keypoints, regularisation graph; frames 1.. are images only.  Images
    are one texture warped by the dense flow that interpolates the projected point motions, so the LK
    tracker sees what the geometry says."""
    from scipy.interpolate import griddata
    rng = np.random.default_rng(seed)
    prm = HAMLYN_PINHOLE if model == PINHOLE else ENDOMAPPER_KB8
    w, h = (640, 480) if model == PINHOLE else (736, 552)
    if half_size:                                                  # the same field of view on half as many pixels (320 x 240 for the pinhole)
        prm = np.concatenate([prm[:4] * F32(0.5), prm[4:]]).astype(F32)
        w, h = w // 2, h // 2
    Xmm, nrm = surface_points(n_points, rng, model)
    centroid = Xmm.mean(0)
    scale = F32(3.0) / F32(np.median(Xmm[:, 2]))
    sigma = F32(3.0) * F32(np.std(Xmm[:, 2].astype(F32))) * scale
    s = float(scale)
    poses_R, poses_t, Xt, uvt = [], [], [], []
    for f in range(n_frames):
        phi = step * f
        if model == PINHOLE:
            R, t = _look_at(np.array([6.0 * phi, 2.0 * np.sin(np.pi * phi), 0.0]), centroid)
        else:
            R = _small_rot(np.array([0.03 * phi, -0.04 * phi, 0.02 * phi]))
            t = -R @ np.array([1.5 * phi, 1.0 * np.sin(np.pi * phi), 2.0 * phi])
        amp = deform_amp * np.sin(2 * np.pi * f / 40.0) * (0.6 + 0.4 * np.sin(Xmm[:, 0] / 11.0 + 0.3) * np.cos(Xmm[:, 1] / 9.0))
        X = Xmm + amp[:, None] * nrm
        pc = X @ R.T + t
        poses_R.append(R); poses_t.append(t * s); Xt.append(X * s)
        uvt.append(_project(model, prm.astype(np.float64), pc))
    uv0 = uvt[0]
    vis = (uv0[:, 0] > 30) & (uv0[:, 0] < w - 30) & (uv0[:, 1] > 30) & (uv0[:, 1] < h - 30)
    idx = np.where(vis)[0]
    tex = _texture(h, w, rng)
    occl = [np.clip(np.rint(_texture(46, 58, rng, 0)), 0, 255).astype(np.uint8) for _ in range(occluders)]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    images = []
    for f in range(n_frames):
        if f == 0:
            sx, sy = xs, ys
        else:
            # backward warp: displacement known at the points' positions in frame f, interpolated densely
            d = uv0[idx] - uvt[f][idx]
            pts = uvt[f][idx]
            gx = griddata(pts, d[:, 0], (xs, ys), method="linear")
            gy = griddata(pts, d[:, 1], (xs, ys), method="linear")
            nx = griddata(pts, d[:, 0], (xs, ys), method="nearest")
            ny = griddata(pts, d[:, 1], (xs, ys), method="nearest")
            gx = np.where(np.isnan(gx), nx, gx); gy = np.where(np.isnan(gy), ny, gy)
            sx, sy = xs + gx, ys + gy
        sx2, sy2 = np.clip(sx + 32, 0, w + 62.0), np.clip(sy + 32, 0, h + 62.0)
        x0, y0 = np.floor(sx2).astype(int), np.floor(sy2).astype(int)
        x0, y0 = np.minimum(x0, w + 62), np.minimum(y0, h + 62)
        fx, fy = sx2 - x0, sy2 - y0
        v = (tex[y0, x0] * (1 - fx) + tex[y0, x0 + 1] * fx) * (1 - fy) + (tex[y0 + 1, x0] * (1 - fx) + tex[y0 + 1, x0 + 1] * fx) * fy
        img = np.clip(np.rint(v), 0, 255).astype(np.uint8)
        # moving occluders (from frame 2 on): points under them fail the tracker / its SSIM gate, are
        # re-found by the point-reuse step once the patch has moved on
        for k in range(occluders if f >= 2 else 0):
            cx = int(w * (0.25 + 0.5 * k / max(1, occluders)) + 40 * (f - 2)) % w
            cy = int(h * (0.35 + 0.2 * k))
            ph, pw = 46, 58
            y1, x1 = max(0, cy - ph // 2), max(0, cx - pw // 2)
            patch = occl[k][:max(0, min(ph, h - y1)), :max(0, min(pw, w - x1))]
            img[y1:y1 + patch.shape[0], x1:x1 + patch.shape[1]] = patch
        images.append(img)
    X0 = (Xt[0][idx] + rng.normal(0, 0.002, (len(idx), 3))).astype(F32)
    graph = build_graph(X0, sigma, 16)
    return dict(model=model, prm=prm, scale=float(scale), wh=(w, h), images=images, n_points=len(idx),
                kp0=uv0[idx].astype(F32), X0=X0, graph=graph,
                pose_q=[_R_to_quat(R).astype(F32) for R in poses_R], pose_t=[t.astype(F32) for t in poses_t],
                uv_true=[u[idx].astype(F32) for u in uvt], X_true=[x[idx] for x in Xt])


def edge_checksum(e):
    """order-sensitive 64-bit checksum of a BA edge list (sp_ij, sp_d0, dm_idx, dm_w): golden files carry it so that
    a trace is only ever compared on the edge list it was computed from"""
    import zlib
    h = 0
    for key in ("sp_ij", "sp_d0", "dm_idx", "dm_w"):
        a = np.ascontiguousarray(e[key])
        a = a.astype(np.int32) if a.dtype.kind == "i" else a.astype(np.float32)
        h = (h * 1000003 + zlib.crc32(a.tobytes())) & 0xFFFFFFFFFFFF
    return int(h)


def make_temporal_buffer(n_frames=12, seed=3, model=PINHOLE, spacing=26.0, cand_frac=0.3, lm_noise=0.004, kp_noise=0.25,
                         baseline=0.35, deform_amp=0.8):
    """A flat TemporalBuffer (reference modules/map/temporal_buffer.h:43-63) for DeformableTriangulation: n_frames
    snapshots of a deforming surface seen by a translating camera.  Features sit on a jittered image grid (the
    extractor's non-maximum suppression keeps features apart; GetClosestMapPointsToFeature rejects a candidate with a
    3D neighbour closer than 20 px): (1 - cand_frac) of them are map points (landmark position in every snapshot they
    are seen in, TRACKED_WITH_3D in the last one), the rest are 2D-only candidates with tracks of varying length.
    Returns the dict nrs.triangulate_batch / oracle/triang_oracle.py read, plus `cand` (ids) and `truth` (world
    positions of the candidates in the last frame)."""
    rng = np.random.default_rng(seed)
    prm = HAMLYN_PINHOLE if model == PINHOLE else ENDOMAPPER_KB8
    w, h = (640, 480) if model == PINHOLE else (736, 552)
    gx, gy = np.meshgrid(np.arange(40, w - 40, spacing), np.arange(40, h - 40, spacing))
    uv0 = np.stack([gx.ravel(), gy.ravel()], 1) + rng.uniform(-2.0, 2.0, (gx.size, 2))
    n = len(uv0)
    # back-project the grid onto the surface z = 60 + 8 sin(x/15) cos(y/12) (two fixed-point steps are plenty)
    P = prm.astype(np.float64)
    z = np.full(n, 60.0)
    for _ in range(3):
        if model == PINHOLE:
            x, y = (uv0[:, 0] - P[2]) / P[0] * z, (uv0[:, 1] - P[3]) / P[1] * z
        else:
            th = np.hypot((uv0[:, 0] - P[2]) / P[0], (uv0[:, 1] - P[3]) / P[1])
            psi = np.arctan2((uv0[:, 1] - P[3]) / P[1], (uv0[:, 0] - P[2]) / P[0])
            x, y = z * np.tan(th) * np.cos(psi), z * np.tan(th) * np.sin(psi)
        z = 60.0 + 8.0 * np.sin(x / 15.0) * np.cos(y / 12.0)
    Xmm = np.stack([x, y, z], 1)
    nrm = np.array([0.0, 0.0, 1.0])
    scale = 3.0 / np.median(z)
    is_cand = rng.uniform(size=n) < cand_frac
    poses, has_kp, kp_xy, has_lm, lm_xyz = [], np.zeros((n_frames, n), bool), np.zeros((n_frames, n, 2), F32), np.zeros((n_frames, n), bool), np.zeros((n_frames, n, 3), F32)
    start = np.where(is_cand, rng.integers(0, n_frames - 2, n), 0)           # candidates appear at different times
    truth = np.zeros((n, 3))
    for f in range(n_frames):
        R = _small_rot(np.array([0.002 * f, -0.003 * f, 0.001 * f]))
        C = np.array([baseline * f, 0.12 * baseline * f, 0.0])              # camera centre (mm)
        t = -R @ C
        amp = deform_amp * np.sin(2 * np.pi * f / 30.0) * (0.6 + 0.4 * np.sin(Xmm[:, 0] / 11.0 + 0.3) * np.cos(Xmm[:, 1] / 9.0))
        X = Xmm + amp[:, None] * nrm
        uv = _project(model, P, X @ R.T + t) + rng.normal(0, kp_noise, (n, 2))
        q = _rot_to_quat(R)
        poses.append(np.concatenate([q, t * scale]))
        seen = (f >= start) & (uv[:, 0] > 12) & (uv[:, 0] < w - 12) & (uv[:, 1] > 12) & (uv[:, 1] < h - 12)
        has_kp[f] = seen
        kp_xy[f] = uv.astype(F32)
        has_lm[f] = seen & ~is_cand & (rng.uniform(size=n) > 0.03)          # a few map points drop out of a snapshot
        lm_xyz[f] = (X * scale + rng.normal(0, lm_noise, (n, 3))).astype(F32)
        truth = X * scale
    status = np.where(is_cand, 1, 0).astype(np.int32)                        # TRACKED (2D) / TRACKED_WITH_3D
    status[~has_kp[-1]] = 3
    cand = np.where(is_cand & has_kp[-1])[0].astype(np.int32)
    return dict(n_frames=n_frames, poses=np.array(poses, F32), has_kp=has_kp, kp_xy=kp_xy, has_lm=has_lm, lm_xyz=lm_xyz,
                status=status, cand=cand, truth=truth[cand].astype(F32), model=model, prm=prm, scale=F32(scale))


def make_mapping_buffer(n_frames=12, seed=3, model=PINHOLE, spacing=26.0, cand_frac=0.3, rad_per_pixel=None, deform_amp=0.2, **kw):
    """make_temporal_buffer for Mapping::LandmarkTriangulation (include/nrs.h nrs_map_frame): adds `deform_mag` (one
    Snapshot::deformation_magnitud per snapshot, all below the reference's rigidity threshold 0.004) and `rad_per_pixel` (default:
    1 / fx), and picks the camera baseline so that the parallax of a track of 0.7 (n_frames - 1) frames at the scene's depth (60 mm) is
    15 rad_per_pixel: the rigid leg's window [10, 20] rad_per_pixel then holds the longer tracks and rejects the short ones."""
    prm = HAMLYN_PINHOLE if model == PINHOLE else ENDOMAPPER_KB8
    rpp = float(1.0 / prm[0]) if rad_per_pixel is None else float(rad_per_pixel)
    baseline = 15.0 * rpp * 60.0 / (0.7 * (n_frames - 1))
    tb = make_temporal_buffer(n_frames, seed, model, spacing, cand_frac, baseline=baseline, deform_amp=deform_amp, **kw)
    rng = np.random.default_rng(seed + 7919)
    tb["deform_mag"] = rng.uniform(0.0005, 0.003, n_frames).astype(F32)
    tb["rad_per_pixel"] = rpp
    return tb


def _rot_to_quat(R):
    """unit quaternion (x y z w) of a rotation matrix, w >= 0"""
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def pick_nodes(points_xyz, n_nodes, start=0):
    """Farthest-point sampling of n_nodes map points (float64, ties to the lowest index): the node set of the synthetic
    embedded-deformation windows.  Returns a uint8 flag per map point."""
    X = np.asarray(points_xyz, np.float64)
    flag = np.zeros(len(X), np.uint8)
    if n_nodes >= len(X):
        flag[:] = 1
        return flag
    d = np.full(len(X), np.inf)
    cur = start
    for _ in range(n_nodes):
        flag[cur] = 1
        d = np.minimum(d, np.sum((X - X[cur]) ** 2, axis=1))
        d[flag == 1] = -1.0
        cur = int(np.argmax(d))
    return flag


def node_lists(X, sigma, flag, k=24):
    """Ordered neighbour lists for the EMBEDDED windows: per map point the k nearest NODES (itself excluded) whose weight reaches
    min_weight, by (weight desc, index asc), status NEUTRAL -- the prefix a GetEdges list of the reference's all-pairs graph
    (map.cc:148-166, regularization_graph.cc:61-87) shows once everything but the nodes is passed over; the walks of the embedded
    mode accept <= 11 of them.  Same wire form as ordered_view()."""
    X = np.asarray(X, F32)
    sigma = F32(sigma)
    nodes = np.where(np.asarray(flag) != 0)[0]
    min_w = _weight(F32(float(sigma) * 1.5), sigma)
    kk = min(k + 1, len(nodes))
    tree = cKDTree(X[nodes].astype(np.float64))
    _, nn = tree.query(X.astype(np.float64), k=kk)
    nn = nn.reshape(len(X), kk)
    rowptr = np.zeros(len(X) + 1, np.int32)
    col, w, d0 = [], [], []
    for p in range(len(X)):
        c = nodes[nn[p]]
        c = c[c != p]
        rel = X[c] - X[p]
        d = np.sqrt((rel[:, 0] * rel[:, 0] + rel[:, 1] * rel[:, 1] + rel[:, 2] * rel[:, 2]).astype(F32)).astype(F32)
        ww = _weight(d, sigma)
        keep = ww >= min_w
        c, d, ww = c[keep], d[keep], ww[keep]
        o = np.lexsort((c, -ww.astype(np.float64)))
        col.append(c[o]); w.append(ww[o]); d0.append(d[o])
        rowptr[p + 1] = rowptr[p] + len(o)
    col = np.concatenate(col).astype(np.int32)
    return dict(rowptr=rowptr, col=col, w=np.concatenate(w).astype(F32), d0=np.concatenate(d0).astype(F32), status=np.full(len(col), GRAPH_NEUTRAL, np.int32))


def embedded_problem(p, n_nodes, k=24):
    """node flags (farthest-point sampling on the rest shape) and the node lists of a window p (make_dba_problem)"""
    flag = pick_nodes(p["scene"]["X0"], n_nodes)
    return flag, node_lists(p["scene"]["X0"], p["scene"]["sigma"], flag, k)


def embedded_window(p, e):
    """Inputs of nrs_dba_*_embedded from a plain window p (make_dba_problem) and the embedded edge lists e (dba_build_embedded /
    nrs_dba_build_edges_embedded: node copies lm_obs, skinned observations sk_obs as indices into the window's observations)."""
    lo, so = e["lm_obs"], e["sk_obs"]
    return dict(lm_xyz=p["lm_xyz"][lo], lm_kf=p["lm_kf"][lo], lm_uv=p["lm_uv"][lo],
                sk_kf=p["lm_kf"][so], sk_uv=p["lm_uv"][so], sk_xyz=p["lm_xyz"][so])


def nd_block_system(n, seed=3, knn=11):
    """An SPD block system with the structure of a2's single-frame problem (input of nrs_debug_nd_solve): n points on a surface, 3 x 3
    couplings to the knn nearest neighbours, two `last` blocks (the halves of the pose) coupled to every point, block-diagonally dominant.
    Returns pos, last, pairs, Dn, Vp, bn (no dense copy: usable at 5k points)."""
    rng = np.random.default_rng(seed)
    pts = np.c_[rng.uniform(-20, 20, n), rng.uniform(-15, 15, n), 60 + rng.normal(0, 1, n)]
    _, nn = cKDTree(pts[:, :2]).query(pts[:, :2], k=min(knn + 1, n))
    a = np.repeat(np.arange(n), nn.shape[1] - 1)
    b = nn[:, 1:].ravel()
    pr = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], 1), axis=0)
    pr = pr[pr[:, 0] != pr[:, 1]]
    pp = np.array([(n + h, i) if (i + h) % 2 else (i, n + h) for i in range(n) for h in range(2)] + [(n, n + 1)], np.int64)
    pairs = np.r_[pr, pp].astype(np.int32)
    N = n + 2
    Vp = rng.normal(0, 1, (len(pairs), 3, 3)) * 0.3
    rs = np.zeros((N, 3))
    np.add.at(rs, pairs[:, 0], np.abs(Vp).sum(2))
    np.add.at(rs, pairs[:, 1], np.abs(Vp).sum(1))
    S_ = rng.normal(0, 0.2, (N, 3, 3))
    Dn = np.einsum('nij,nkj->nik', S_, S_) + np.eye(3)[None] * (rs.max(1)[:, None, None] + 0.5)
    pos = np.r_[pts, np.zeros((2, 3))]
    last = np.zeros(N, np.uint8)
    last[n:] = 1
    return pos, last, pairs, Dn, Vp, rng.normal(0, 1, (N, 3))


def make_init_pair(n=300, seed=1, model=PINHOLE, baseline=4.0, rot=(0.01, -0.02, 0.015), noise_px=0.3, outlier_frac=0.0, untracked_frac=0.0,
                   relief=10.0):
    """Two views of a RIGID surface for the monocular map initialisation (f6): the reference camera at the origin, the current one moved by
    `baseline` mm (0: a pure rotation) and turned by the rotation vector `rot`.  Returns ref_xy / cur_xy (n x 2, fp32), status (n, 1 = TRACKED;
    untracked points are interleaved and carry status 3 with their reference position as cur_xy), the true camera_transform_world (R, t with
    |t| = baseline) and the points in the reference camera's frame.  Outliers keep status TRACKED and get a uniformly random cur_xy."""
    rng = np.random.default_rng(seed)
    prm = HAMLYN_PINHOLE if model == PINHOLE else ENDOMAPPER_KB8
    if model == PINHOLE:
        x, y = rng.uniform(-20, 20, n), rng.uniform(-15, 15, n)
        z = 60 + relief * np.sin(x / 7) * np.cos(y / 6) + rng.uniform(-0.3 * relief, 0.3 * relief, n)      # (not a plane: the 8-point system needs relief)
        X = np.stack([x, y, z], 1)
    else:
        ang, z = rng.uniform(0, 2 * np.pi, n), rng.uniform(12.0, 70.0, n)
        rad = 15 + 1.5 * np.sin(3 * ang) * np.cos(z / 9)
        X = np.stack([rad * np.cos(ang), rad * np.sin(ang), z], 1)
    R = _small_rot(np.asarray(rot, np.float64))
    d = np.array([1.0, 0.25, 0.1])
    t = -baseline * d / np.linalg.norm(d)
    ref = _project(model, prm.astype(np.float64), X)
    cur = _project(model, prm.astype(np.float64), X @ R.T + t)
    ref = ref + rng.normal(0, noise_px, ref.shape)
    cur = cur + rng.normal(0, noise_px, cur.shape)
    status = np.ones(n, np.int32)
    out = rng.random(n) < outlier_frac
    lo, hi = ref.min(0), ref.max(0)
    cur[out] = rng.uniform(lo, hi, (int(out.sum()), 2))
    un = np.zeros(n, bool)
    if untracked_frac > 0:
        step = max(2, int(round(1.0 / untracked_frac)))
        un[step // 2::step] = True
        status[un] = 3
        cur[un] = ref[un]
    return dict(model=model, prm=prm.copy(), ref_xy=ref.astype(F32), cur_xy=cur.astype(F32), status=status, n_matches=int((status == 1).sum()),
                R=R, t=t, X=X, outlier=out, untracked=un)


def make_init_sequence(n_points=500, n_frames=8, seed=3, wh=(320, 240), step=0.35, rot_step=(0.0006, -0.0009, 0.0004)):
    """Rendered frames for the monocular map initialisation end to end (f6): a RIGID surface (the pinhole rest shape of surface_points)
    seen by a camera that moves `step` mm per frame sideways and turns by rot_step per frame; frame 0 is the texture of
    make_frame_sequence, the later frames are that texture warped by the dense flow interpolated from the projected point motions.
    The calibration is the Hamlyn pinhole scaled to the image size.  Returns images, the calibration and the true poses and points."""
    from scipy.interpolate import griddata
    rng = np.random.default_rng(seed)
    w, h = wh
    prm = HAMLYN_PINHOLE.copy()
    prm[:4] = prm[:4] * F32(w / 640.0)
    X, _ = surface_points(n_points, rng, PINHOLE)
    d = np.array([1.0, 0.3, 0.0])
    poses_R, poses_t, uvt = [], [], []
    for f in range(n_frames):
        R = _small_rot(np.asarray(rot_step, np.float64) * f)
        t = -R @ (step * f * d)
        poses_R.append(R); poses_t.append(t)
        uvt.append(_project(PINHOLE, prm.astype(np.float64), X @ R.T + t))
    uv0 = uvt[0]
    tex = _texture(h, w, rng)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    images = []
    for f in range(n_frames):
        if f == 0:
            sx, sy = xs, ys
        else:
            dd, pts = uv0 - uvt[f], uvt[f]
            gx = griddata(pts, dd[:, 0], (xs, ys), method="linear")
            gy = griddata(pts, dd[:, 1], (xs, ys), method="linear")
            nx = griddata(pts, dd[:, 0], (xs, ys), method="nearest")
            ny = griddata(pts, dd[:, 1], (xs, ys), method="nearest")
            gx = np.where(np.isnan(gx), nx, gx); gy = np.where(np.isnan(gy), ny, gy)
            sx, sy = xs + gx, ys + gy
        sx2, sy2 = np.clip(sx + 32, 0, w + 62.0), np.clip(sy + 32, 0, h + 62.0)
        x0, y0 = np.minimum(np.floor(sx2).astype(int), w + 62), np.minimum(np.floor(sy2).astype(int), h + 62)
        fx, fy = sx2 - x0, sy2 - y0
        v = (tex[y0, x0] * (1 - fx) + tex[y0, x0 + 1] * fx) * (1 - fy) + (tex[y0 + 1, x0] * (1 - fx) + tex[y0 + 1, x0 + 1] * fx) * fy
        images.append(np.clip(np.rint(v), 0, 255).astype(np.uint8))
    return dict(model=PINHOLE, prm=prm, wh=(w, h), images=images, R=poses_R, t=poses_t, X=X, uv_true=[u.astype(F32) for u in uvt],
                radians_per_pixel=float(1.0 / prm[0]))


# ---- f7: evaluation (include/nrs.h "f7: evaluation")
def make_stereo_pair(wh, seed, disparities=(7, 0), n_keypoints=24, row_pad=0, repeat=True):
    """A rectified pair for the stereo matchers: the left image is `_texture` (clipped to 250, so that nothing saturates by accident), the
    right image is the same texture shifted by an integer disparity per horizontal band (len(disparities) bands of equal height): the
    left pixel (x, y) of a band with disparity d is found at (x - d, y).  Keypoints sit on templates that lie inside one band; every
    second one gets a fractional part.  Planted specials, all listed in the result: one keypoint whose template holds a 255 pixel
    (saturated), one on integer coordinates in a band of disparity 0 (when there is one), one in each boundary band of
    StereoPatternMatching::computeStereo3D, and (repeat) one whose right-image patch is copied to the top-left corner of the search
    region, so that its best score is attained twice and the first row-major position, the copy, must win.
    row_pad > 0: `left_rows` / `right_rows` are h x (w + row_pad) arrays whose pad columns hold 255, for callers that pass a row stride.
    -> dict(left, right, xy, disparity (planted, -1 for boundary keypoints), kind (per keypoint: "ok", "saturated", "zero", "tie",
    "boundary"), match (expected top-left corner of the best window, -1 for rejected ones), expect_status)"""
    rng = np.random.default_rng(seed)
    w, h = wh
    dmax = int(max(disparities))
    tex = np.clip(np.rint(_texture(h, w + dmax, rng, 0)), 0, 250).astype(np.uint8)
    nb = len(disparities)
    edges = [int(round(b * h / nb)) for b in range(nb + 1)]
    left = tex[:, :w].copy()
    right = np.zeros((h, w), np.uint8)
    band_of = np.zeros(h, np.int32)
    for b, d in enumerate(disparities):
        right[edges[b]:edges[b + 1]] = tex[edges[b]:edges[b + 1], d:d + w]
        band_of[edges[b]:edges[b + 1]] = b
    cand = [(x, y) for y in range(7, h - 20) for x in range(27 + dmax, w - 20, 3)
            if band_of[y - 7] == band_of[y + 7] and y % 2 == 0]
    order = rng.permutation(len(cand))
    cand = [cand[i] for i in order]
    sat = cand[0]
    cand = [c for c in cand[1:] if max(abs(c[0] - sat[0]), abs(c[1] - sat[1])) > 15]
    xy, kind, disp = [(float(sat[0]), float(sat[1]))], ["saturated"], [int(disparities[band_of[sat[1]]])]
    left[sat[1] + 2, sat[0] - 3] = 255
    if 0 in disparities:
        z = next(c for c in cand if disparities[band_of[c[1]]] == 0)
        cand.remove(z)
        xy.append((float(z[0]), float(z[1]))); kind.append("zero"); disp.append(0)
    if repeat:
        t = next(c for c in cand if disparities[band_of[c[1]]] > 0)
        cand.remove(t)
        d = int(disparities[band_of[t[1]]])
        xy.append((float(t[0]), float(t[1]))); kind.append("tie"); disp.append(d)
        right[0:15, 0:15] = right[t[1] - 7:t[1] + 8, t[0] - 7 - d:t[0] + 8 - d]
    bounds = [(21.5, h / 2.0), (w - 19.5, h / 2.0), (w / 2.0, h - 19.5), (w / 2.0, 5.0), (-1.0, h / 2.0)]
    n_reg = max(0, n_keypoints - len(xy) - len(bounds))
    for k, c in enumerate(cand[:n_reg]):
        fr = (0.0, 0.0) if k % 2 == 0 else (float(rng.choice([0.25, 0.5, 0.75])), float(rng.choice([0.0, 0.5])))
        xy.append((c[0] + fr[0], c[1] + fr[1])); kind.append("ok"); disp.append(int(disparities[band_of[c[1]]]))
    for b in bounds:
        xy.append(b); kind.append("boundary"); disp.append(-1)
    xy = np.array(xy, F32)
    match = np.full((len(xy), 2), -1, np.int32)
    for i, k in enumerate(kind):
        if k in ("ok", "zero"):
            match[i] = (int(xy[i, 0] - 7) - disp[i], int(xy[i, 1] - 7))
        elif k == "tie":
            match[i] = (0, 0)
    # nrs_eval_status expected of each keypoint: 0 OK, 1 out of bounds, 2 saturated, 4 zero disparity (integer x in a band of disparity 0)
    expect = np.array([dict(saturated=2, boundary=1, zero=4, tie=0).get(k, 4 if (disp[i] == 0 and xy[i, 0] == int(xy[i, 0])) else 0)
                       for i, k in enumerate(kind)], np.int32)
    out = dict(wh=(w, h), left=left, right=right, xy=xy, disparity=np.array(disp, np.int32), kind=kind, match=match, expect_status=expect)
    if row_pad:
        for name, im in (("left_rows", left), ("right_rows", right)):
            full = np.full((h, w + row_pad), 255, np.uint8)
            full[:, :w] = im
            out[name] = full
    return out


def make_depth_image(sq, frame):
    """The fp32 depth image of frame `frame` of a make_frame_sequence scene: the camera-frame z of the true surface points at their true
    image positions, interpolated densely (linear inside their hull, nearest outside), in map units."""
    from scipy.interpolate import griddata
    w, h = sq["wh"]
    q = np.asarray(sq["pose_q"][frame], np.float64)
    x, y, z, s = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * s), 2 * (x * z + y * s)],
                  [2 * (x * y + z * s), 1 - 2 * (x * x + z * z), 2 * (y * z - x * s)],
                  [2 * (x * z - y * s), 2 * (y * z + x * s), 1 - 2 * (x * x + y * y)]])
    zc = (np.asarray(sq["X_true"][frame], np.float64) @ R.T + np.asarray(sq["pose_t"][frame], np.float64))[:, 2]
    uv = np.asarray(sq["uv_true"][frame], np.float64)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    lin = griddata(uv, zc, (xs, ys), method="linear")
    near = griddata(uv, zc, (xs, ys), method="nearest")
    return np.where(np.isnan(lin), near, lin).astype(F32)


# ---- f8: stereo map initialisation (include/nrs.h "f8")
def make_cluster_cases():
    """Hand-made point sets for nrs_dbscan3d: a list of dict(name, xyz [n,3] fp32, eps, min_points).  The smallest shapes at which the
    kernels can go wrong: the empty set and sets around min_points, around a wave (64) and around a compaction chunk (1024), the inclusive
    boundary, a long chain (in order and shuffled), two chains joined through a non-core point, equal sizes, noise in the majority,
    coincident points, a NaN and an infinite coordinate, min_points = 1.  Every set is clustered with noise competing and not."""
    rng = np.random.default_rng(61)
    eps, mp = 2.5, 5
    cases = []

    def add(name, xyz, eps=eps, min_points=mp):
        cases.append(dict(name=name, xyz=np.asarray(xyz, F32).reshape(-1, 3), eps=float(eps), min_points=int(min_points)))

    def blobs(n, k=3, spread=1.1, noise=0.25):
        nn = int(n * noise)
        c = rng.uniform(-14, 14, (k, 3))
        p = c[rng.integers(0, k, n - nn)] + rng.normal(0, spread, (n - nn, 3))
        p = np.concatenate([p, rng.uniform(-30, 30, (nn, 3))])
        return p[rng.permutation(n)]

    add("empty", np.zeros((0, 3)))
    add("one", [[1, 2, 3]])
    add("min_points", [[0, 0, 0], [2, 0, 0], [2.1, 0.1, 0], [2, 0.2, 0.1], [1.9, 0, 0.2]])      # 4 neighbours each: nobody is core
    # point 0 has exactly min_points neighbours (core); points 1-4 have min_points - 1 (border); point 5 has one (border)
    add("min_points+1", [[0, 0, 0], [2, 0, 0], [2.1, 0.1, 0], [2, 0.2, 0.1], [1.9, 0, 0.2], [-2.4, 0, 0]])
    for n in (63, 64, 65):
        add("blobs%d" % n, blobs(n, 2, 0.9))
    for n in (1023, 1024, 1025):
        add("blobs%d" % n, blobs(n, 5, 2.0))
    # exactly eps apart (d2 = 6.25 exactly: neighbours) and one fp32 ulp beyond (not)
    beyond = np.nextafter(F32(2.5), F32(3))
    add("boundary", [[0, 0, 0], [2.5, 0, 0], [0, 100, 0], [beyond, 100, 0]], min_points=1)
    chain = np.stack([np.arange(300) * 0.9 * eps, np.zeros(300), np.zeros(300)], 1)
    add("chain300", chain, min_points=2)
    add("chain300_shuffled", chain[rng.permutation(300)], min_points=2)
    add("chain300_reversed", chain[::-1], min_points=2)
    # min_points 3, spacing 0.45 eps: interior points have 4 neighbours.  The bridge (index 0) lies 0.9 eps beyond the end of either chain:
    # it has 2 neighbours, both core, and is not core itself -- the chains stay two clusters; chain B holds the lower indices
    s = 0.45 * eps
    a = np.stack([np.arange(20) * s, np.zeros(20), np.zeros(20)], 1)
    bridge = np.array([[19 * s + 0.9 * eps, 0, 0]])
    b = np.stack([bridge[0, 0] + 0.9 * eps + np.arange(20) * s, np.zeros(20), np.zeros(20)], 1)
    add("bridge", np.concatenate([bridge, b, a]), min_points=3)
    cube = rng.uniform(0, 1, (8, 3))
    add("equal_sizes", np.concatenate([cube + [50, 0, 0], cube]), min_points=5)
    lone = np.stack([np.arange(20) * 10.0, np.full(20, 40.0), np.zeros(20)], 1)
    add("noise_majority", np.concatenate([lone[:7], cube, lone[7:], cube[:6] + [0, -40, 0]]), min_points=5)
    add("coincident", np.tile([[3.25, -1.5, 60.0]], (10, 1)))
    p = blobs(40, 1, 0.8, 0.1)
    p[7, 1] = np.nan
    p[21, 2] = np.inf
    add("nan_inf", p)
    add("min_points_1", rng.uniform(-8, 8, (70, 3)), min_points=1)
    return cases


DB_CHUNK, DB_TRIP = 1024, 4096       # nrs_dbscan3d: points of a compaction chunk; points behind one trip of a lane-strided word loop (64 x 64)


def _star(centre):
    """a core point with six neighbours that are no neighbours of each other (2 apart along the axes, eps 2.5): with min_points 5 the
    centre is the cluster's only core point, the six are border points"""
    c = np.asarray(centre, np.float64)
    return c, c + 2.0 * np.concatenate([np.eye(3), -np.eye(3)])


def _roots(raw, core):
    """lowest core index of every cluster, by raw label (ascending, since raw labels are given in that order)"""
    r = np.full(int(raw.max()) + 1 if len(raw) else 0, len(raw), np.int64)
    idx = np.nonzero(core)[0]
    np.minimum.at(r, raw[idx], idx)
    return r


def _holds_roots_in_three_chunks(c, raw, core, nb):
    roots = _roots(raw, core)
    n = len(raw)
    assert np.all(roots < n) and np.all(np.diff(roots) > 0)
    per_chunk = np.bincount(roots // DB_CHUNK, minlength=3)
    assert len(per_chunk) == 3 and per_chunk.min() >= 20, per_chunk
    size = np.bincount(raw[raw >= 0])
    chunks_of_size = {}
    for k, s in enumerate(size):
        chunks_of_size.setdefault(int(s), set()).add(int(roots[k] // DB_CHUNK))
    assert any(len(v) > 1 for v in chunks_of_size.values())       # equal sizes, roots in different chunks: the ranking's tie-break
    assert (raw < 0).any()


def _holds_first_root_late(c, raw, core, nb):
    assert not core[:2 * DB_CHUNK].any() and core[2 * DB_CHUNK:].sum() >= 2
    assert (raw[:2 * DB_CHUNK] >= 0).any() and (raw[:2 * DB_CHUNK] < 0).any()      # border points and noise in front
    assert raw.max() >= 1


def _holds_second_trip(c, raw, core, nb):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(raw)
    assert n > DB_TRIP
    low = core & (np.arange(n) < DB_TRIP)
    g = csr_matrix(nb & low[:, None] & low[None, :])
    _, comp = connected_components(g, directed=False)              # components of the core points that the first trip alone sees
    first = [i for i in range(64) if core[i]]
    assert any(raw[i] == raw[j] and comp[i] != comp[j] for i in first for j in first), "joined only through a core point behind the trip"
    only_high = wrong_not_noise = False
    for q in np.nonzero(~core & (raw >= 0))[0]:
        cn = np.nonzero(nb[q] & core)[0]
        lo, hi = cn[cn < DB_TRIP], cn[cn >= DB_TRIP]
        if len(hi) and not len(lo):
            only_high = True
        if len(hi) and len(lo) and raw[lo].min() > raw[hi].min():
            wrong_not_noise = True
    assert only_high and wrong_not_noise


def _holds_one_chain(c, raw, core, nb):
    n = len(raw)
    assert n > DB_TRIP and np.all(raw == 0) and core.sum() == n - 2          # (the two ends have one neighbour: border points)
    assert nb[:DB_TRIP, DB_TRIP:].any()                            # neighbours on either side of the word-64 boundary


def _holds_full(c, raw, core, nb):
    n = len(raw)
    assert n > 16384 - 64 and (n + 63) // 64 == 256
    roots = _roots(raw, core)
    assert len(np.unique(roots // DB_CHUNK)) >= 8
    last = np.nonzero(core[16320:])[0] + 16320
    assert any(roots[raw[i]] < DB_CHUNK for i in last)


def make_large_cluster_cases():
    """Point sets for nrs_dbscan3d past one compaction chunk (1024 points), past one trip of the lane-strided word loops (4096 points) and
    at the limit (16384 points): the list of make_cluster_cases' dicts, each with `holds(case, raw, core, nb)`, which asserts from the
    oracle's raw labels, core flags and neighbour matrix that the set holds what it is made for.
      roots_in_three_chunks   clusters whose lowest core index lies in each of [0, 1024), [1024, 2048), [2048, n): blobs of 8 points whose
                              members all come at or after their chunk's start, and for the narrow last chunk stars (`_star`) whose centre
                              comes there; blobs of equal size in different chunks
      first_root_late         no core point before index 2048: star satellites and noise in front, the star centres and one blob behind
      second_trip4097 / 4160  around the origin + (1000, 0, 0), min_points 3: C (index >= 4096) joins A and B (indices 3 and 40); P touches
                              C alone; Q touches C and D (index 50, a cluster of its own with a higher raw label); leaves make A, B, D core
      chain4200_shuffled      one chain, min_points 2, 0.9 eps apart
      full16384 / full16321   the blob recipe shuffled; a member of the first blob point's blob is moved to the last index"""
    rng = np.random.default_rng(67)
    eps, mp = 2.5, 5
    cases = []

    def add(name, xyz, holds, eps=eps, min_points=mp):
        cases.append(dict(name=name, xyz=np.ascontiguousarray(xyz, F32).reshape(-1, 3), eps=float(eps), min_points=int(min_points), holds=holds))

    def centres(k):
        return rng.uniform(-300, 300, (k, 3))

    def blob_points(c):
        return (c[:, None, :] + rng.normal(0, 0.6, (len(c), 8, 3))).reshape(-1, 3)

    # roots_in_three_chunks: 100 blobs free, 100 blobs at index >= 1024, 30 stars with the centre at index >= 2048, 290 noise points
    n = 2100
    free = np.concatenate([blob_points(centres(100)), rng.uniform(-300, 300, (290, 3))])
    mid = blob_points(centres(100))
    stars = [_star(c) for c in centres(30)]
    late = np.array([s[0] for s in stars])
    free = np.concatenate([free] + [s[1] for s in stars])
    free, mid = free[rng.permutation(len(free))], mid[rng.permutation(len(mid))]
    n_late_mid = n - 2 * DB_CHUNK - len(late)                      # the last chunk: the star centres and this many points of `mid`
    tail = np.concatenate([late, mid[:n_late_mid]])
    middle = np.concatenate([mid[n_late_mid:], free[:DB_CHUNK - (len(mid) - n_late_mid)]])
    front = free[DB_CHUNK - (len(mid) - n_late_mid):]
    assert len(front) == DB_CHUNK and len(middle) == DB_CHUNK and len(tail) == n - 2 * DB_CHUNK
    add("roots_in_three_chunks", np.concatenate([front[rng.permutation(DB_CHUNK)], middle[rng.permutation(DB_CHUNK)], tail[rng.permutation(len(tail))]]),
        _holds_roots_in_three_chunks)

    # first_root_late: 8 star centres and a blob of 44 behind index 2047; the 48 satellites and 2000 noise points in front
    stars = [_star(c) for c in centres(8)]
    front = np.concatenate([s[1] for s in stars] + [rng.uniform(-300, 300, (2 * DB_CHUNK - 48, 3))])
    tail = np.concatenate([np.array([s[0] for s in stars]), centres(1) + rng.normal(0, 0.6, (44, 3))])
    add("first_root_late", np.concatenate([front[rng.permutation(len(front))], tail[rng.permutation(len(tail))]]), _holds_first_root_late)

    # second_trip: the planted points by name -> (index, position); everything else is blobs and noise within +-300
    for n, ic in ((DB_TRIP + 1, DB_TRIP), (DB_TRIP + 64, DB_TRIP + 63)):
        k = (n - 12) // 9
        fill = np.concatenate([blob_points(centres(k)), rng.uniform(-300, 300, (n - 12 - 8 * k, 3))])
        fill = fill[rng.permutation(len(fill))]
        planted = {3: (-2, 0, 0), 7: (-2, 2, 0), 8: (-2, -2, 0),                  # A and its leaves
                   40: (2, 0, 0), 41: (2, 2, 0), 42: (2, -2, 0),                  # B and its leaves
                   50: (0, 0, -4), 51: (0, 2, -4), 52: (0, -2, -4),               # D and its leaves
                   60: (0, 0, 2), 61: (0, 0, -2), ic: (0, 0, 0)}                  # P, Q and C
        xyz = np.zeros((n, 3))
        rest = np.array([i for i in range(n) if i not in planted])
        xyz[rest] = fill
        for i, p in planted.items():
            xyz[i] = np.array(p, np.float64) + (1000.0, 0.0, 0.0)
        add("second_trip%d" % n, xyz, _holds_second_trip, min_points=3)

    chain = np.stack([np.arange(4200) * 0.9 * eps, np.zeros(4200), np.zeros(4200)], 1)
    add("chain4200_shuffled", chain[rng.permutation(4200)], _holds_one_chain, min_points=2)

    for n in (16384, 16384 - 63):
        k = int(n * 0.9) // 8
        member = np.concatenate([np.repeat(np.arange(k), 8), np.full(n - 8 * k, -1)])
        xyz = np.concatenate([blob_points(centres(k)), rng.uniform(-300, 300, (n - 8 * k, 3))])
        order = rng.permutation(n)
        xyz, member = xyz[order], member[order]
        first = int(np.nonzero(member >= 0)[0][0])                 # (index 0 or just behind it)
        other = int(np.nonzero(member == member[first])[0][1])
        xyz[[other, n - 1]] = xyz[[n - 1, other]]
        add("full%d" % n, xyz, _holds_full)
    return cases


def make_stereo_init_sequence(n_points=500, n_frames=3, seed=3, wh=(320, 240), step=0.35, rot_step=(0.0006, -0.0009, 0.0004), bf=2400.0):
    """make_init_sequence's surface, texture and warp (the same random stream, so the same left images) plus a RIGHT view of frame 0: the
    same warp for a camera displaced by the baseline along +x only, so the pair is rectified -- a point at depth z that the left image shows
    at (u, v) is found at (u - bf / z, v).  bf (baseline times focal length, in mm px) puts the surface's 52-68 mm at disparities of
    about 35-46 px: one disparity step is about 1.5 mm of depth.  Returned with the scene: bf, the z gate around the surface's range
    (z_min, z_max) and eps -- the extractor leaves a few hundred keypoints on 50 x 38 mm of surface, about 0.15 per square mm, so the
    reference's 2.5 mm radius (Hamlyn images hold several times as many) would find no core point; eps = 6 mm holds about 15."""
    from scipy.interpolate import griddata
    sq = make_init_sequence(n_points, n_frames, seed, wh, step, rot_step)
    rng = np.random.default_rng(seed)                              # the stream of make_init_sequence: surface, then texture
    w, h = wh
    X, _ = surface_points(n_points, rng, PINHOLE)
    tex = _texture(h, w, rng)
    uv0 = _project(PINHOLE, sq["prm"].astype(np.float64), X)
    disp = float(bf) / X[:, 2]
    uvr = uv0 - np.stack([disp, np.zeros(len(X))], 1)              # the right camera sees the point `disp` pixels to the left
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    gx = griddata(uvr, disp, (xs, ys), method="linear")
    nx = griddata(uvr, disp, (xs, ys), method="nearest")
    gx = np.where(np.isnan(gx), nx, gx)
    sx2, sy2 = np.clip(xs + gx + 32, 0, w + 62.0), np.clip(ys + 32, 0, h + 62.0)
    x0, y0 = np.minimum(np.floor(sx2).astype(int), w + 62), np.minimum(np.floor(sy2).astype(int), h + 62)
    fx, fy = sx2 - x0, sy2 - y0
    v = (tex[y0, x0] * (1 - fx) + tex[y0, x0 + 1] * fx) * (1 - fy) + (tex[y0 + 1, x0] * (1 - fx) + tex[y0 + 1, x0 + 1] * fx) * fy
    sq.update(right=np.clip(np.rint(v), 0, 255).astype(np.uint8), bf=float(bf), z_min=45.0, z_max=75.0, eps=6.0, min_points=5,
              disparity_at=lambda xy: griddata(uv0, disp, np.asarray(xy, np.float64), method="linear"))
    return sq
