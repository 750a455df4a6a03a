"""Inputs of the flow-track clustering tests (tests/test_flow_cluster_cases_cpu.py, tests/test_gpu_flow_cluster.py): every case is built
once, with the oracle's result, and handed out read-only.  A point case is dict(name, data [n, dim] fp32, eps, min_points, label, counts);
a track case dict(name, tracks [n, L, 2] fp32, label, counts, flows).  What a case is made for is asserted on the CPU by `holds(case)`
from the oracle alone, so a pass on the device cannot be vacuous."""
import functools

import numpy as np

import flow_cluster_oracle as FO

F32 = np.float32
EDGE_N = (1, 63, 64, 65, 130, 200)        # around an adjacency word = an LDS tile (64) and no multiple of any tile
EDGE_DIM = (1, 2, 3, 7, 60, 64)
TILE = 64


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _solved(name, data, eps, min_points, **more):
    data = np.ascontiguousarray(data, F32)
    nb = FO.neighbours_nd(data, eps)
    label, counts, core = FO.labels_from(nb, min_points)
    return _freeze(dict(name=name, data=data, eps=float(eps), min_points=int(min_points), label=label, counts=counts, core=core, nb=nb, **more))


def _blobs(rng, n, dim, k, noise):
    """k blobs 10 apart along coordinate 0 (jitter within 0.4 / sqrt(dim) per coordinate: any two points of a blob are within 0.8) and
    `noise` lone points 100 apart from everything"""
    m = n - noise
    c = np.zeros((k, dim))
    c[:, 0] = 10.0 * np.arange(k)
    p = c[np.arange(m) % k] + rng.uniform(-0.4, 0.4, (m, dim)) / np.sqrt(dim)
    lone = np.zeros((noise, dim))
    lone[:, 0] = -100.0 * (1 + np.arange(noise))
    p = np.concatenate([p, lone])
    return p[rng.permutation(n)]


@functools.lru_cache(maxsize=None)
def edge_case(n, dim):
    rng = np.random.default_rng(1000 * n + dim)
    noise = 0 if n == 1 else max(1, n // 10)
    return _solved("edge_n%d_dim%d" % (n, dim), _blobs(rng, n, dim, 3, noise) if n > 1 else np.full((1, dim), 2.5), 1.0, 4)


def edge_holds(c):
    n = len(c["data"])
    if n == 1:
        assert c["label"].tolist() == [-1] and c["counts"].tolist() == [0, 1]
    else:
        assert c["counts"].tolist() == [3, max(1, n // 10)] and c["core"].sum() == n - c["counts"][1]
        if n >= 2 * TILE:                                          # a cluster's members lie in more than one word / tile
            assert all(len(set(np.nonzero(c["label"] == k)[0] // TILE)) >= 2 for k in range(3))


@functools.lru_cache(maxsize=None)
def structure_case():
    """dim 5, everything on coordinate 0, eps 1, min_points 4.  Cluster B (indices 1, 7..10; label 0 through index 1) and cluster A (indices
    2..6; label 1), five points each within 0.65: four neighbours, all core.  Point 0 at x = 1 is 0.95 from A's 0.05 (index 6) and from B's
    1.95 (index 7) and further than 1 from everything else: two neighbours, not core, a border point of BOTH clusters whose lowest-index
    core neighbour is in the cluster with the HIGHER label.  Index 11 is noise."""
    x = [1.0, 2.6, -0.6, -0.5, -0.4, -0.3, 0.05, 1.95, 2.3, 2.4, 2.5, 50.0]
    data = np.zeros((len(x), 5), F32)
    data[:, 0] = x
    return _solved("structure", data, 1.0, 4)


def structure_holds(c):
    lab, nb, core = c["label"], c["nb"], c["core"]
    assert c["counts"].tolist() == [2, 1] and lab[11] == -1
    assert lab[[1, 7, 8, 9, 10]].tolist() == [0] * 5 and lab[2:7].tolist() == [1] * 5 and core[1:11].all()
    assert not core[0] and np.nonzero(nb[0])[0].tolist() == [6, 7] and (lab[6], lab[7]) == (1, 0)
    assert lab[0] == 0                                             # the lowest label wins, not the lowest-index neighbour's


def _tie_points(outwards):
    """dim 10 (eps = 0.1 * 10 = 1 exactly).  Rows come in pairs (2 i, 2 i + 1), pairs 100 apart on coordinate 9: the second row differs from
    the first by 0.5 in four coordinates (pairs 0..2) or by 1.0 in one (pairs 3..5), so d2 == eps^2 == 1 exactly.  outwards: one of those
    coordinates lies one fp32 ulp further out"""
    rows = []
    for i in range(6):
        a = np.zeros(10, F32)
        a[9] = 100.0 * i
        a[:9] = [3.0, -1.5, 0.25, 8.0, 0.0, -4.0, 2.0, 1.0, -0.75]
        b = a.copy()
        if i < 3:
            ks = [(i + s) % 9 for s in (0, 2, 4, 6)]
            for k in ks:
                b[k] = a[k] + F32(0.5)
        else:
            ks = [i]
            b[i] = a[i] - F32(1.0)
        if outwards:
            k = ks[-1]
            b[k] = np.nextafter(b[k], F32(np.inf) if b[k] > a[k] else F32(-np.inf))       # away from a[k]
        rows += [a, b]
    return np.array(rows, F32)


@functools.lru_cache(maxsize=None)
def tie_case(outwards):
    assert FO.flow_eps(10) == 1.0
    return _solved("near_ties" if outwards else "exact_ties", _tie_points(outwards), FO.flow_eps(10), 1)


def tie_holds(exact, near):
    """the exact pairs are neighbours (inclusive boundary) and each is a cluster of two; one ulp outwards flips every one of them to noise"""
    for i in range(6):
        assert exact["nb"][2 * i, 2 * i + 1] and exact["nb"][2 * i + 1, 2 * i]
        assert not near["nb"][2 * i, 2 * i + 1] and not near["nb"][2 * i + 1, 2 * i]
    assert exact["nb"].sum() == 12 and near["nb"].sum() == 0
    assert exact["label"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5] and exact["counts"].tolist() == [6, 0]
    assert near["label"].tolist() == [-1] * 12 and near["counts"].tolist() == [0, 12]


ORDER_SEED, ORDER_DIM, ORDER_PAIRS = 7, 60, 10


@functools.lru_cache(maxsize=None)
def order_case():
    """dim 60, eps = 0.1 * 60 = 6, min_points 2.  Triples (a, b, h): h is 1 from a and more than sqrt(37) from b; b is made so that d2(a, b)
    equals eps^2 = 36 to far below one fp64 unit in the last place of 36 in EXACT arithmetic -- 58 random coordinates that leave a gap of
    about 2e-5, one coordinate (a 0, b t1) whose square fills the gap up to t1's fp32 rounding, one more (a 0, b t2) that fills that
    remainder -- so the rounding of the 59 adds alone decides on which side of 36 the sum falls.  A seeded search keeps the first ORDER_PAIRS
    triples where the ascending sequential sum and the pairwise (tree) sum fall on DIFFERENT sides.  With the pair a neighbour pair a has
    two neighbours and is core, (a, b, h) is a cluster; without it all three are noise."""
    import math
    rng = np.random.default_rng(ORDER_SEED)
    eps = FO.flow_eps(ORDER_DIM)
    assert eps == 6.0
    eps2 = eps * eps
    rows, pairs, tried = [], [], 0
    while len(pairs) < ORDER_PAIRS:
        tried += 1
        assert tried < 4000
        a = rng.uniform(-4, 4, ORDER_DIM).astype(F32)
        k1, k2 = 1 + rng.choice(ORDER_DIM - 1, 2, replace=False)
        delta = rng.standard_normal(ORDER_DIM)
        delta[[k1, k2]] = 0.0
        delta *= math.sqrt((eps2 - 2e-5) / float(np.sum(delta * delta)))
        a[[k1, k2]] = 0.0
        b = (a.astype(np.float64) + delta).astype(F32)
        b[[k1, k2]] = 0.0

        def exact_gap():
            d = b.astype(np.float64) - a.astype(np.float64)
            return eps2 - math.fsum([float(v) * float(v) for v in d])      # (each product of two 24-bit differences is exact in fp64 up to its 53 bits)

        g = exact_gap()
        if not 1e-7 < g < 1e-4:
            continue
        t1 = F32(math.sqrt(g))
        if float(t1) * float(t1) > g:
            t1 = np.nextafter(t1, F32(0))
        b[k1] = t1
        g2 = exact_gap()
        if not 0.0 <= g2 < 1e-9:
            continue
        b[k2] = F32(math.sqrt(g2))
        p = np.stack([a, b]).astype(np.float64)
        seq, tree = FO.d2_row(p, 0, "sequential")[1], FO.d2_row(p, 0, "tree")[1]
        if (seq <= eps2) == (tree <= eps2):
            continue
        h = a.copy()
        h[0] = a[0] - F32(1.0 if b[0] >= a[0] else -1.0)
        pairs.append((len(rows), len(rows) + 1, bool(seq <= eps2)))
        rows += [a, b, h]
    c = _solved("order_sensitive", np.array(rows, F32), eps, 2, pairs=tuple(pairs))
    c["label_tree"], c["counts_tree"] = FO.dbscan_nd(c["data"], eps, 2, order="tree")
    return _freeze(c)


def order_holds(c):
    nb_tree = FO.neighbours_nd(c["data"], c["eps"], "tree")
    diff = np.argwhere(c["nb"] != nb_tree)
    want = sorted([(i, j) for i, j, _ in c["pairs"]] + [(j, i) for i, j, _ in c["pairs"]])
    assert sorted(map(tuple, diff.tolist())) == want and len(c["pairs"]) >= 8     # the two orders part on these pairs and nowhere else
    assert len({s for _, _, s in c["pairs"]}) == 2                               # ... in both directions
    changed = 0
    for i, j, seq_in in c["pairs"]:
        assert c["nb"][i, j] == seq_in and nb_tree[i, j] != seq_in
        trio = [i, j, j + 1]
        assert (c["label"][trio] >= 0).all() == seq_in and (c["label"][trio] == -1).all() != seq_in
        changed += int(not np.array_equal(c["label"][trio] >= 0, c["label_tree"][trio] >= 0))
    assert changed >= 1 and changed == len(c["pairs"])             # decided the other way, every one of them changes its labels


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    rng = np.random.default_rng(11)
    p = _blobs(rng, 30, 4, 1, 2).astype(F32)
    p[5] = p[4]; p[5, 2] = np.nan                                  # copies of cluster points, one coordinate spoilt
    p[17] = p[16]; p[17, 0] = np.inf
    return _solved("nonfinite", p, 1.0, 3, bad=(5, 17))


def nonfinite_holds(c):
    for i in c["bad"]:
        assert not c["nb"][i].any() and not c["nb"][:, i].any() and c["label"][i] == -1
    assert c["counts"][0] == 1 and c["counts"][1] >= 2 and (c["label"] == 0).sum() >= 20


@functools.lru_cache(maxsize=None)
def chunk_case():
    """n = 1100 at dim 20 (two queries per wave): five blobs and 30 lone points in the first 1030 indices, a sixth blob alone in the last 70,
    so its lowest core index lies past one compaction chunk (1024)"""
    rng = np.random.default_rng(12)
    head = _blobs(rng, 1030, 20, 5, 30)
    tail = _blobs(rng, 70, 20, 1, 0)
    tail[:, 1] += 40.0
    return _solved("chunk1100", np.concatenate([head, tail]), 1.0, 4)


def chunk_holds(c):
    lab = c["label"]
    assert len(lab) == 1100 and c["counts"].tolist() == [6, 30]
    last = np.nonzero(lab == 5)[0]
    assert len(last) == 70 and last.min() >= 1030 and c["core"][last].all()     # the sixth root is found in the second chunk
    assert np.nonzero(c["core"])[0][lab[c["core"]] == 5].min() > 1024


@functools.lru_cache(maxsize=None)
def wide_case():
    """n = 4100 at dim 4: past 4096 points a wave carries four queries"""
    rng = np.random.default_rng(13)
    return _solved("wide4100", _blobs(rng, 4100, 4, 7, 100), 1.0, 4)


def wide_holds(c):
    assert len(c["data"]) > 4096 and c["counts"].tolist() == [7, 100]


@functools.lru_cache(maxsize=None)
def big60_case():
    """1100 x 60: the longest flow vectors of a 31-image track at a size past one compaction chunk"""
    return _solved("big1100x60", _blobs(np.random.default_rng(14), 1100, 60, 4, 40), 1.0, 4)


@functools.lru_cache(maxsize=None)
def tiny_case():
    """5 x 2, for a call that follows a large one in the same buffer: four points within 0.15 of each other and one far away"""
    return _solved("tiny5x2", [[0, 0], [0.1, 0], [0, 0.1], [5, 5], [0.1, 0.1]], 0.5, 3)


def big_then_tiny_holds(big, tiny):
    assert big["data"].shape == (1100, 60) and big["counts"].tolist() == [4, 40]
    assert tiny["data"].shape == (5, 2) and tiny["label"].tolist() == [0, 0, 0, -1, 0] and tiny["counts"].tolist() == [1, 1]


POINT_CASES = ("structure", "exact_ties", "near_ties", "order_sensitive", "nonfinite", "chunk1100", "wide4100", "big1100x60", "tiny5x2")


def point_case(name):
    return {"structure": structure_case, "exact_ties": lambda: tie_case(False), "near_ties": lambda: tie_case(True), "order_sensitive": order_case,
            "nonfinite": nonfinite_case, "chunk1100": chunk_case, "wide4100": wide_case, "big1100x60": big60_case, "tiny5x2": tiny_case}[name]()


def for_device(c):
    """(data, eps, min_points) without the oracle's side"""
    return c["data"], c["eps"], c["min_points"]


# ---- flow tracks
@functools.lru_cache(maxsize=None)
def track_case(length, quantised=True):
    """150 tracks of `length` keypoints in a 640 x 480 image: two motions of 60 tracks each (steps (0.8, 0.1) and (-0.5, 0.6) px, jitter within
    0.05 px) and 30 tracks that wander by up to 3 px a step.  quantised: keypoints on multiples of 1 / 1024 px.  Not quantised: the tracks
    start within a pixel of the corner instead, where consecutive keypoints differ by more than a factor of two -- the only place where an fp32
    subtraction of two fp32 keypoints rounds at all (closer than that it is exact)"""
    rng = np.random.default_rng(20 + length)
    n = 150
    step = np.zeros((n, length - 1, 2))
    step[:60] = (0.8, 0.1)
    step[60:120] = (-0.5, 0.6)
    step[:120] += rng.uniform(-0.05, 0.05, (120, length - 1, 2))
    step[120:] = rng.uniform(-3, 3, (30, length - 1, 2))
    start = rng.uniform([100, 100], [540, 380], (n, 2)) if quantised else rng.uniform(0.1, 0.6, (n, 2))
    xy = np.concatenate([start[:, None, :], start[:, None, :] + np.cumsum(step, 1)], 1)
    if quantised:
        xy = np.rint(xy * 1024.0) / 1024.0
    order = rng.permutation(n)
    tracks = np.ascontiguousarray(xy[order], F32)
    label, counts, fl = FO.flow_tracks_cluster(tracks)
    return _freeze(dict(name="tracks_L%d%s" % (length, "" if quantised else "_raw"), tracks=tracks, label=label, counts=counts, flows=fl,
                        group=np.where(order < 60, 0, np.where(order < 120, 1, 2))))


def track_holds(c):
    t, lab, g = c["tracks"], c["label"], c["group"]
    L = t.shape[1]
    assert c["flows"].shape == (150, 2 * (L - 1)) and c["flows"].dtype == F32
    assert c["counts"][0] == 2 and len(set(lab[g == 0])) == 1 and len(set(lab[g == 1])) == 1 and lab[g == 0][0] != lab[g == 1][0]
    assert (lab[g == 2] == -1).sum() >= 25 and (lab[g < 2] >= 0).all()
    if c["name"].endswith("_raw"):                                  # unquantised keypoints: the fp32 subtraction rounds, the fp64 one does not
        t64 = t.astype(np.float64)
        assert (c["flows"][:, 0::2].astype(np.float64) != t64[:, 1:, 0] - t64[:, :-1, 0]).any()
    else:
        assert np.array_equal(t * F32(1024), np.rint(t * F32(1024)))
