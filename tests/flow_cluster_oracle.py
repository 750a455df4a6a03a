"""NumPy oracle of the flow-track clustering (include/nrs.h "f6": nrs_dbscan_nd, nrs_flow_tracks_cluster), taking nothing from the library:

  flows                MonocularMapInitializer::FeatureTracksClustering's flow builder (monocular_map_initializer.cc:191-211): one fp32
                       subtraction per coordinate and step
  neighbours_nd        j != i and d2(i, j) <= eps * eps, d2 the fp64 sum over the coordinates in ascending order, written as a SEPARATE multiply
                       and add per coordinate (element-wise; no BLAS, no np.sum, no np.linalg.norm), the first product starting the sum.
                       order="tree" sums the same products pairwise instead: the cases use it to show that a pair's verdict depends on the order
  dbscan_nd            DbscanND (modules/utilities/dbscan.cc:106-131) under the project's definition (DESIGN.md 4 "Flow-track clustering"):
                       the textbook SEQUENTIAL algorithm of stereo_init_oracle.dbscan3d_raw on that relation; no ranking
  flow_tracks_cluster  the two together with eps = double(float(0.1 * dim)) and min_points = 10"""
import numpy as np

import stereo_init_oracle as SO

F32 = np.float32
MIN_POINTS = 10


def flows(tracks_xy):
    """[n, L, 2] fp32 keypoints -> [n, 2 (L - 1)] fp32: coordinate 2(t-1) is x_t - x_(t-1), 2(t-1)+1 is y_t - y_(t-1), each one fp32 subtraction"""
    t = np.asarray(tracks_xy, F32)
    n, L = t.shape[0], t.shape[1]
    out = np.zeros((n, 2 * (L - 1)), F32)
    for s in range(1, L):
        out[:, 2 * (s - 1)] = t[:, s, 0] - t[:, s - 1, 0]           # fp32 - fp32 -> fp32
        out[:, 2 * (s - 1) + 1] = t[:, s, 1] - t[:, s - 1, 1]
    return out


def d2_row(p, i, order="sequential"):
    """d2(i, j) for every j, on the float64 copy p of the fp32 coordinates"""
    dim = p.shape[1]
    prods = []
    for k in range(dim):
        d = p[:, k] - p[i, k]
        prods.append(d * d)                                          # the product, rounded
    if order == "sequential":
        acc = prods[0]
        for k in range(1, dim):
            acc = acc + prods[k]                                     # then the add, rounded
        return acc
    assert order == "tree"
    while len(prods) > 1:
        nxt = [prods[a] + prods[a + 1] for a in range(0, len(prods) - 1, 2)]
        if len(prods) % 2:
            nxt.append(prods[-1])
        prods = nxt
    return prods[0]


def neighbours_nd(data, eps, order="sequential"):
    """n x n bool: j != i and d2(i, j) <= eps * eps (inclusive); a non-finite d2 is no neighbour pair"""
    p = np.asarray(data, F32).astype(np.float64)
    assert p.ndim == 2 and p.shape[1] >= 1
    n = len(p)
    nb = np.zeros((n, n), bool)
    eps2 = np.float64(eps) * np.float64(eps)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            d2 = d2_row(p, i, order)
            nb[i] = np.isfinite(d2) & (d2 <= eps2)
            nb[i, i] = False
    return nb


def labels_from(nb, min_points):
    """-> (label, counts = clusters, noise points, core flags): the sequential pass over a neighbour matrix; the raw label is the label"""
    raw, core = SO.dbscan3d_raw(None, min_points=min_points, nb=nb)
    counts = np.array([len({int(r) for r in raw if r >= 0}), int((raw < 0).sum())], np.int32)
    return raw.astype(np.int32), counts, core


def dbscan_nd(data, eps, min_points=MIN_POINTS, order="sequential"):
    """-> (label [n], counts (clusters, noise points))"""
    data = np.asarray(data, F32)
    if len(data) == 0:
        return np.zeros(0, np.int32), np.zeros(2, np.int32)
    label, counts, _ = labels_from(neighbours_nd(data, eps, order), min_points)
    return label, counts


def flow_eps(dim):
    """the reference's `float eps = 0.1 * dim`, widened again"""
    return float(F32(0.1 * float(dim)))


def flow_tracks_cluster(tracks_xy):
    """-> (label [n], counts, flows [n, 2 (L - 1)])"""
    fl = flows(tracks_xy)
    label, counts = dbscan_nd(fl, flow_eps(fl.shape[1]), MIN_POINTS)
    return label, counts, fl
