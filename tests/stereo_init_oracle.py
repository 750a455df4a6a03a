"""NumPy oracle of the stereo map initialisation (include/nrs.h "f8"), taking nothing from the library:

  dbscan3d      Dbscan3D (modules/utilities/dbscan.cc:61-104).  mlpack is not in the tree, so the clustering is the project's definition
                (DESIGN.md 4 "Stereo map initialisation"), written here as the TEXTBOOK SEQUENTIAL algorithm: points are visited in index
                order, every unvisited core point starts a cluster that is expanded with a queue, a border point is kept by the first
                cluster that reaches it.  The device is specified by the fixed-point formulation (connected components of the core points,
                a border point takes the lowest raw label among its core neighbours); `dbscan3d_fixed_point` restates that one by brute
                force, and tests/test_stereo_init_oracle_cpu.py holds the two to each other.
  init_stereo   Tracking::StereoMapInitialization (modules/tracking/tracking.cc:216-263) over eval_oracle.stereo_match_pattern

d2 is formed on float64 copies of the fp32 coordinates as (dx*dx + dy*dy) + dz*dz, element-wise (no BLAS, no np.linalg.norm)."""
from collections import deque

import numpy as np

import eval_oracle as EO

F32 = np.float32
SELECTED, MATCHER_REJECTED, OUTSIDE_GATE, OTHER_CLUSTER = 0, 1, 2, 3


def neighbours(xyz, eps):
    """n x n bool: j != i and d2(i, j) <= eps * eps (inclusive); a non-finite d2 is no neighbour pair"""
    p = np.asarray(xyz, F32).reshape(-1, 3).astype(np.float64)
    n = len(p)
    nb = np.zeros((n, n), bool)
    eps2 = np.float64(eps) * np.float64(eps)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            dx, dy, dz = p[:, 0] - p[i, 0], p[:, 1] - p[i, 1], p[:, 2] - p[i, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            nb[i] = np.isfinite(d2) & (d2 <= eps2)
            nb[i, i] = False
    return nb


def rank_labels(raw, noise_competes):
    """dbscan.cc:80-101: classes by raw label, size descending, ties by ascending raw key; noise (-1) is a class when it competes,
    else keeps -1.  -> (label, counts = clusters, noise points, size of label 0)"""
    raw = np.asarray(raw, np.int32)
    sizes = {}
    for r in raw:
        if r >= 0 or noise_competes:
            sizes[int(r)] = sizes.get(int(r), 0) + 1
    order = sorted(sizes, key=lambda k: (-sizes[k], k))
    rank = {k: i for i, k in enumerate(order)}
    label = np.array([rank.get(int(r), -1) for r in raw], np.int32).reshape(-1)
    n_clusters = len({int(r) for r in raw if r >= 0})
    counts = np.array([n_clusters, int((raw < 0).sum()), sizes[order[0]] if order else 0], np.int32)
    return label, counts


def dbscan3d_raw(xyz, eps=2.5, min_points=5, nb=None):
    """-> (raw_label, core flags).  The sequential algorithm: OrderedPointSelection, a queue per cluster.  nb: `neighbours(xyz, eps)` when
    the caller holds it already (the large cases, whose properties are asserted on the same matrix)"""
    if nb is None:
        nb = neighbours(xyz, eps)
    n = len(nb)
    core = nb.sum(1) >= min_points
    raw = np.full(n, -1, np.int32)
    visited = np.zeros(n, bool)
    next_label = 0
    for i in range(n):
        if visited[i] or not core[i]:
            continue
        visited[i] = True
        raw[i] = next_label
        queue = deque([i])
        while queue:
            a = queue.popleft()
            for j in np.nonzero(nb[a])[0]:
                if raw[j] < 0:                                     # first cluster to reach it keeps it
                    raw[j] = next_label
                if core[j] and not visited[j]:
                    visited[j] = True
                    queue.append(int(j))
        next_label += 1
    return raw, core


def dbscan3d(xyz, eps=2.5, min_points=5, noise_competes=True):
    """-> (raw_label, label, counts): dbscan3d_raw and the reference's ranking"""
    raw, _ = dbscan3d_raw(xyz, eps, min_points)
    label, counts = rank_labels(raw, noise_competes)
    return raw, label, counts


def dbscan3d_fixed_point(xyz, eps=2.5, min_points=5, noise_competes=True):
    """The definition the device is written to, by brute force: components of the core points by repeated closure of the minimum label,
    raw labels in ascending order of a component's lowest core index, a border point takes the lowest raw label among its core neighbours"""
    nb = neighbours(xyz, eps)
    n = len(nb)
    core = nb.sum(1) >= min_points
    lab = np.where(core, np.arange(n), n)
    while True:
        new = lab.copy()
        for i in np.nonzero(core)[0]:
            m = nb[i] & core
            if m.any():
                new[i] = min(lab[i], lab[m].min())
        if np.array_equal(new, lab):
            break
        lab = new
    roots = sorted({int(v) for v in lab[core]})
    rid = {r: k for k, r in enumerate(roots)}
    raw = np.full(n, -1, np.int32)
    for i in range(n):
        if core[i]:
            raw[i] = rid[int(lab[i])]
        else:
            m = nb[i] & core
            if m.any():
                raw[i] = min(rid[int(v)] for v in lab[m])
    label, counts = rank_labels(raw, noise_competes)
    return raw, label, counts


def init_stereo(prm, left, right, xy, bf=3886.37, z_min=35.5, z_max=70.5, eps=2.5, min_points=5, noise_competes=1):
    """-> the dict of nrs.Context.init_stereo"""
    xy = np.asarray(xy, F32).reshape(-1, 2)
    n = len(xy)
    xyz, st, _, _ = EO.stereo_match_pattern(prm, F32(bf), left, right, xy)
    z = xyz[:, 2]
    with np.errstate(invalid="ignore"):
        gate = (st == EO.OK) & (z > F32(z_min)) & (z < F32(z_max))           # float against float; a NaN fails
    gidx = np.nonzero(gate)[0]                                               # keypoint order: the reference's push_back order
    raw_g, lab_g, counts = dbscan3d(xyz[gidx], eps, min_points, bool(noise_competes))
    code = np.where(st != EO.OK, MATCHER_REJECTED, OUTSIDE_GATE).astype(np.int32)
    raw, label = np.full(n, -2, np.int32), np.full(n, -2, np.int32)
    raw[gidx], label[gidx] = raw_g, lab_g
    code[gidx] = np.where(lab_g == 0, SELECTED, OTHER_CLUSTER)
    sel = gidx[lab_g == 0].astype(np.int32)
    sel_xyz = xyz[sel]
    median = F32(np.nan)
    if len(sel):
        k = len(sel) // 2
        median = F32(np.sort(sel_xyz[:, 2])[k])                              # nth_element at n / 2 (:247-248)
    return dict(verdict=0 if len(gidx) else 1, n_matched=int((st == EO.OK).sum()), n_gated=len(gidx), n_clusters=int(counts[0]),
                n_noise=int(counts[1]), n_selected=len(sel), median_depth=median, xyz=xyz, match_status=st.astype(np.int32), code=code,
                raw_label=raw, label=label, selected=sel, selected_xyz=sel_xyz)
