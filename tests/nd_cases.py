"""Designed block systems for the direct solver (nr-slam_amd/csrc/nrs_nd_kernels.hpp k_nd_level / k_nd_tile / k_nd_back on the plan of
nrs_nd_plan.hpp), shared by tests/test_nd_cases_cpu.py (vets them without a GPU) and tests/test_gpu_nd_cases.py (holds the device to them).

A case is (pos, last, pairs, Dn, Vp, bn, lam) -- the arguments of nrs_debug_nd_solve and of the host reference CPU.nd_solve -- with its
dense matrix A (lam included), a high-precision reference solution xref (dense fp64 solve + two steps of iterative refinement, residual in
np.longdouble; None for an indefinite case), a sentence on what it is for, and CLAIMS: the front shapes it says it reaches, which
test_nd_cases_cpu.py proves through the plan taps CPU.nd_plan_fronts / CPU.nd_plan_nodes.  get(name) builds a case once; treat it as
read-only (the arrays are write-protected).

The targets come from the kernels' constants: 16-column steps, ND_S16 = 96, ND_TB = 48 (the right-hand side is row b of the boundary: at
b = 48 and b = 96 it sits alone in a row block of its own), ND_SMAXN = ND_LEAFN = 32 nodes.

SHAPE cases (values as in test_nd_cpu.block_system: strictly diagonally dominant, lam = 0.37)
  s<k>          a complete graph on k nodes: ONE front with s = 3 k, b = 0      s = 3, 15, 18, 48, 51, 93, 96
  b<3m>         a complete graph on 32 nodes (one leaf, s = 96) coupled to m nodes flagged `last`: a leaf with b = 3 m
                b = 3, 45, 48, 51, 96, 99, 150 (four row blocks: workgroups with I > J), and b1056 (23 row blocks: 277 workgroups in
                the leaf's level, more than an MI355X has CUs, so the level runs as two launches and k_nd_tile makes the tiles)
  s51b48        17 + 16 nodes: the own block ends inside a 16-column step AND the right-hand side row is alone in its row block
  grid          40 x 10 grid, stretched across its rows so that the dissection cuts ALONG them: 40-node separators, each split into a
                chain of two fronts; several levels
  gridpose      the grid with two `last` nodes coupled to every point (a2's pose); gridpose_nolast: the same problem with last=None
  path          200 nodes in a line: one-node separators, a deep tree
  star          a hub that is NOT flagged `last` with 120 spokes
  isolated      a 60-node neighbour graph with ten nodes that nothing couples to
  n1, n2        one node without pairs; two coupled nodes
  No b target is left out.

NUMERIC cases, each on `grid` (several levels) and on `b150` (one front with four row blocks)
  *_lam0        lam = 0
  *_ill         NOT diagonally dominant: diagonal blocks are sums of R^T R over the node's couplings (a graph Laplacian with 3 x 3 weights)
                plus a ridge of 1e-9 of the largest diagonal entry, lam of the same size: condition number 1e8 .. 1e12
  *_dn40, *_up40  Dn, Vp, bn and lam scaled by 2^-40 / 2^+40: the exact solution is unchanged
  *_unit_leaf, *_unit_root   the right-hand side is a unit vector in an unknown of a leaf / of the root

INDEFINITE cases: a twin with one defect, placed through CPU.nd_plan_nodes; smallest eigenvalue below -1e-3 of the largest
  b150_neg_c0 / _c16 / _c80   a diagonal block of the leaf (s = 96, four row blocks: ten (I, J) workgroups) negated, at an own column in 0..15, >= 16, >= 80
  grid_neg_mid                ... of a separator front at a middle level
  b150_neg_root, grid_neg_root   ... of the root front (in b150: a `last` node, the pose)
  b150_late, grid_late        every diagonal block is positive definite, but one coupling block between a leaf node and a node of an
                              ancestor outweighs them: the pivot turns negative only once the leaf's Schur complement is in the ancestor
  isolated_zero               an exactly zero 3 x 3 block on an isolated node, lam = 0 (twin: isolated_lam0); exempt from the margin

HOST: eta_host and fwd_host of the host reference per definite case, MEASURED by test_nd_cases_cpu.py (which also checks this table, so it
cannot go stale; `PYTHONPATH=oracle python tests/nd_cases.py` prints it).  eta = |b - A x|inf / (|A|inf |x|inf + |b|inf) with the residual in np.longdouble,
fwd = |x - xref|inf / |xref|inf.  The device bounds of test_gpu_nd_cases.py are built from these, never from a device result."""
import functools
from collections import namedtuple

import numpy as np

import nrs_cpu as CPU

Case = namedtuple("Case", "name pos last pairs Dn Vp bn lam A xref what kind twin claims defect")
LAM = 0.37
EPS = float(np.finfo(np.float64).eps)


# ---------------------------------------------------------------------------------------------------------------- pieces
def dense(n, pairs, Dn, Vp, lam):
    A = np.zeros((3 * n, 3 * n))
    for (a, b), V in zip(pairs, Vp):
        A[3 * a:3 * a + 3, 3 * b:3 * b + 3] += V
        A[3 * b:3 * b + 3, 3 * a:3 * a + 3] += V.T
    for i in range(n):
        A[3 * i:3 * i + 3, 3 * i:3 * i + 3] += Dn[i]
    return A + lam * np.eye(3 * n)


def reference(A, b):
    """dense fp64 solve, then two steps of iterative refinement with the residual in np.longdouble"""
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    x = np.linalg.solve(A, b).astype(np.longdouble)
    for _ in range(2):
        r = bl - Al @ x
        x = x + np.linalg.solve(A, r.astype(np.float64)).astype(np.longdouble)
    return x


def errors(A, b, x, xref):
    """(normwise backward error of x, residual in np.longdouble; forward error against xref)"""
    xl = np.asarray(x, np.float64).ravel().astype(np.longdouble)
    r = b.ravel().astype(np.longdouble) - A.astype(np.longdouble) @ xl
    eta = np.abs(r).max() / (np.abs(A).sum(1).max() * np.abs(xl).max() + np.abs(b).max())
    fwd = np.abs(xl - xref).max() / np.abs(xref).max()
    return float(eta), float(fwd)


def _orient(pairs):
    """either node may come first in a pair"""
    pairs = np.array(sorted(set((min(a, b), max(a, b)) for a, b in pairs)), np.int32).reshape(-1, 2)
    flip = (np.arange(len(pairs)) * 7 + 3) % 5 < 2
    pairs[flip] = pairs[flip][:, ::-1]
    return pairs


def _dominant_values(n, pairs, seed):
    """as test_nd_cpu.block_system: every diagonal block is S S^T + (largest absolute row sum of its rows + 0.5) I"""
    rng = np.random.default_rng(seed)
    Vp = rng.normal(0, 1, (len(pairs), 3, 3)) * 0.3
    rowsum = np.abs(dense(n, pairs, np.zeros((n, 3, 3)), Vp, 0.0)).sum(1)
    Dn = np.zeros((n, 3, 3))
    for i in range(n):
        S = rng.normal(0, 0.2, (3, 3))
        Dn[i] = S @ S.T + np.eye(3) * (rowsum[3 * i:3 * i + 3].max() + 0.5)
    return Dn, Vp, rng.normal(0, 1, (n, 3))


def _laplacian_values(n, pairs, seed):
    """A = sum over the couplings (a, b) of B^T B, B = [R at a, -R at b]: every diagonal block is the sum of R^T R over the node's
    couplings, the coupling block is -R^T R -- positive SEMI-definite (constant vectors are in the null space), not diagonally dominant;
    plus a ridge of 1e-9 of the largest diagonal entry.  Returns the values and that ridge (the case's lam is the same size)."""
    rng = np.random.default_rng(seed)
    R = rng.normal(0, 1, (len(pairs), 3, 3))
    G = np.einsum("pki,pkj->pij", R, R)
    Dn = np.zeros((n, 3, 3))
    for (a, b), g in zip(pairs, G):
        Dn[a] += g
        Dn[b] += g
    ridge = 1e-9 * max(Dn[i][j, j] for i in range(n) for j in range(3))
    Dn += ridge * np.eye(3)
    return Dn, -G, rng.normal(0, 1, (n, 3)), ridge


# ---------------------------------------------------------------------------------------------------------------- geometries
def _cluster_tail(k, m):
    """a complete graph on k nodes; m `last` nodes, each coupled to two of the cluster's nodes and to the next `last` node"""
    n = k + m
    ang = 2 * np.pi * np.arange(k) / max(k, 1)
    pos = np.r_[np.c_[10 * np.cos(ang), 8 * np.sin(ang), 60 + 0.1 * np.arange(k)], np.zeros((m, 3))]
    pairs = [(i, j) for i in range(k) for j in range(i + 1, k)]
    for j in range(m):
        pairs += [(k + j, j % k)]
        if (7 * j + 3) % k != j % k:
            pairs += [(k + j, (7 * j + 3) % k)]
        if j + 1 < m:
            pairs += [(k + j, k + j + 1)]
    last = np.zeros(n, np.uint8)
    last[k:] = 1
    return pos, last, _orient(pairs)


GRID_W, GRID_H = 40, 10


def _grid(pose):
    """40 x 10 points, neighbours along the rows, the columns and one diagonal; the rows lie 20 apart, so the longest axis is across them"""
    idx = lambda x, y: y * GRID_W + x
    pos = np.array([(x, 20.0 * y, 60 + 0.01 * ((x * 7 + y * 3) % 11)) for y in range(GRID_H) for x in range(GRID_W)], float)
    pairs = []
    for y in range(GRID_H):
        for x in range(GRID_W):
            if x + 1 < GRID_W:
                pairs.append((idx(x, y), idx(x + 1, y)))
            if y + 1 < GRID_H:
                pairs.append((idx(x, y), idx(x, y + 1)))
            if x + 1 < GRID_W and y + 1 < GRID_H:
                pairs.append((idx(x, y), idx(x + 1, y + 1)))
    n = GRID_W * GRID_H
    if pose:
        pairs += [(n + h, i) for i in range(n) for h in range(2)] + [(n, n + 1)]
        pos = np.r_[pos, np.zeros((2, 3))]
    last = np.zeros(len(pos), np.uint8)
    last[n:] = 1
    return pos, last, _orient(pairs)


def _path(n=200):
    pos = np.c_[np.arange(n) * 1.0, np.zeros(n), np.full(n, 60.0)]
    return pos, np.zeros(n, np.uint8), _orient([(i, i + 1) for i in range(n - 1)])


def _star(spokes=120):
    ang = 2 * np.pi * np.arange(spokes) / spokes
    pos = np.r_[[[0.0, 0.0, 60.0]], np.c_[20 * np.cos(ang), 15 * np.sin(ang), np.full(spokes, 60.0)]]
    return pos, np.zeros(spokes + 1, np.uint8), _orient([(0, 1 + i) for i in range(spokes)])


ISOLATED_NODES = tuple(range(3, 70, 7))                             # ten of the seventy


def _isolated():
    rng = np.random.default_rng(77)
    n = 70
    pts = np.c_[rng.uniform(-20, 20, n), rng.uniform(-15, 15, n), 60 + rng.normal(0, 1, n)]
    live = [i for i in range(n) if i not in ISOLATED_NODES]
    pairs = []
    for i in live:
        d = np.linalg.norm(pts[live, :2] - pts[i, :2], axis=1)
        pairs += [(i, live[j]) for j in np.argsort(d)[1:5]]
    return pts, np.zeros(n, np.uint8), _orient(pairs)


# ---------------------------------------------------------------------------------------------------------------- the table of cases
S_CASES = {"s%d" % (3 * k): k for k in (1, 5, 6, 16, 17, 31, 32)}
B_CASES = {"b%d" % (3 * m): m for m in (1, 15, 16, 17, 32, 33, 50, 352)}
NUMERIC_BASES = ("grid", "b150")
NUMERIC_KINDS = ("lam0", "ill", "dn40", "up40", "unit_leaf", "unit_root")

SHAPE_NAMES = tuple(S_CASES) + ("b0",) + tuple(B_CASES) + ("s51b48", "grid", "gridpose", "gridpose_nolast", "path", "star", "isolated", "n1", "n2")
NUMERIC_NAMES = tuple("%s_%s" % (b, k) for b in NUMERIC_BASES for k in NUMERIC_KINDS) + ("isolated_lam0",)
DEFINITE_NAMES = SHAPE_NAMES + NUMERIC_NAMES
INDEFINITE_NAMES = ("b150_neg_c0", "b150_neg_c16", "b150_neg_c80", "grid_neg_mid", "b150_neg_root", "grid_neg_root", "b150_late", "grid_late", "isolated_zero")
# the shape cases that run under every launch-form switch: s = 96, b = 48, b >= 147 (b1056: a crowded level as well), the separator chain
LAUNCH_FORM_NAMES = ("s96", "b48", "b150", "b1056", "grid")


def _geometry(name):
    """(pos, last, pairs, seed, what, claims) of a shape case"""
    if name in S_CASES:
        k = S_CASES[name]
        pos, last, pairs = _cluster_tail(k, 0)
        return pos, last, pairs, 100 + k, "one front whose own block has %d unknowns" % (3 * k), dict(fronts=1, sb=[(3 * k, 0)])
    if name == "b0":
        pos, last, pairs = _cluster_tail(32, 0)
        return pos, last, pairs, 199, "a root: no boundary, the right-hand side row alone", dict(fronts=1, sb=[(96, 0)])
    if name in B_CASES:
        m = B_CASES[name]
        pos, last, pairs = _cluster_tail(32, m)
        nR = (3 * m + 1 + 47) // 48
        return pos, last, pairs, 200 + m, "a 96-unknown leaf with a boundary of %d unknowns (%d row blocks)" % (3 * m, nR), dict(sb=[(96, 3 * m)], wg=nR * (nR + 1) // 2 + 1)
    if name == "s51b48":
        pos, last, pairs = _cluster_tail(17, 16)
        return pos, last, pairs, 251, "own block ends inside a 16-column step, right-hand side row alone in its row block", dict(sb=[(51, 48)])
    if name in ("grid", "gridpose", "gridpose_nolast"):
        pos, last, pairs = _grid(name != "grid")
        what = {"grid": "40-node separators split into chains of fronts, several levels",
                "gridpose": "the grid with a2's pose: two `last` nodes coupled to every point",
                "gridpose_nolast": "the same problem with last=None: the pose nodes are dissected like any other"}[name]
        claims = dict(levels_min=4, chain=True) if name != "gridpose_nolast" else dict(levels_min=3)
        return pos, (None if name == "gridpose_nolast" else last), pairs, 300, what, claims
    if name == "path":
        pos, last, pairs = _path()
        return pos, last, pairs, 310, "a path: one-node separators, a deep tree, tiny fronts", dict(levels_min=4, one_node_separator=True)
    if name == "star":
        pos, last, pairs = _star()
        return pos, last, pairs, 320, "a star whose hub is not flagged `last`", dict(levels_min=2)
    if name == "isolated":
        pos, last, pairs = _isolated()
        return pos, last, pairs, 330, "isolated nodes among connected ones", dict()
    if name == "n1":
        return np.array([[0.0, 0.0, 60.0]]), np.zeros(1, np.uint8), np.zeros((0, 2), np.int32), 340, "one node, no pairs", dict(fronts=1, sb=[(3, 0)])
    if name == "n2":
        return np.array([[0.0, 0.0, 60.0], [1.0, 0.0, 60.0]]), np.zeros(2, np.uint8), np.array([[1, 0]], np.int32), 341, "two coupled nodes", dict(fronts=1, sb=[(6, 0)])
    raise KeyError(name)


def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


def _make(name, pos, last, pairs, Dn, Vp, bn, lam, what, kind, twin, claims, defect=None):
    A = dense(len(pos), pairs, Dn, Vp, lam)
    xref = reference(A, bn.ravel()) if kind == "definite" else None
    _freeze(pos, last, pairs, Dn, Vp, bn, A, xref)
    return Case(name, pos, last, pairs, Dn, Vp, bn, lam, A, xref, what, kind, twin, claims, defect)


def _fronts_nodes(pos, last, pairs):
    return CPU.nd_plan_fronts(pos, last, pairs), CPU.nd_plan_nodes(pos, last, pairs)


def _pick_node(pos, last, pairs, where):
    """a node by its place in the plan: `where` = dict(level=, s=, col_min=, root=, mid=)"""
    fr, nd = _fronts_nodes(pos, last, pairs)
    top = fr[:, 0].max()
    for u in range(len(pos)):
        f, col = nd[u]
        lvl, par, s, b, wg = fr[f]
        if where.get("root") and par >= 0:
            continue
        if where.get("mid") and not (0 < lvl < top and par >= 0):
            continue
        if "level" in where and lvl != where["level"]:
            continue
        if "s" in where and s != where["s"]:
            continue
        if wg < where.get("wg_min", 0):
            continue
        if not (where.get("col_min", 0) <= col <= where.get("col_max", 10 ** 9)):
            continue
        return u
    raise AssertionError("no node at %r" % (where,))


@functools.lru_cache(maxsize=None)
def get(name):
    if name in SHAPE_NAMES:
        pos, last, pairs, seed, what, claims = _geometry(name)
        Dn, Vp, bn = _dominant_values(len(pos), pairs, seed)
        return _make(name, pos, last, pairs, Dn, Vp, bn, LAM, what, "definite", None, claims)
    if name == "isolated_lam0":
        c = get("isolated")
        return _make(name, c.pos, c.last, c.pairs, c.Dn, c.Vp, c.bn, 0.0, "isolated nodes, lam = 0 (twin of isolated_zero)", "definite", None, dict())
    if name in NUMERIC_NAMES:
        base, kind = name.split("_", 1)
        c = get(base)
        pos, last, pairs, Dn, Vp, bn, lam = c.pos, c.last, c.pairs, c.Dn, c.Vp, c.bn, c.lam
        claims = dict(c.claims)
        if kind == "lam0":
            lam, what = 0.0, "lam = 0"
        elif kind == "ill":
            Dn, Vp, bn, lam = _laplacian_values(len(pos), pairs, 400 + len(pos))
            what = "not diagonally dominant, condition number 1e8 .. 1e12"
            claims["cond"] = (1e8, 1e12)
        elif kind in ("dn40", "up40"):
            f = 2.0 ** (-40 if kind == "dn40" else 40)
            Dn, Vp, bn, lam, what = Dn * f, Vp * f, bn * f, lam * f, "the whole system scaled by 2^%s40" % ("-" if kind == "dn40" else "+")
            claims["same_solution_as"] = base
        else:
            u = _pick_node(pos, last, pairs, dict(level=0) if kind == "unit_leaf" else dict(root=True))
            bn = np.zeros_like(bn)
            bn[u, 1] = 1.0
            what = "right-hand side: a unit vector in an unknown of %s" % ("a leaf" if kind == "unit_leaf" else "the root")
            claims["rhs_node"] = (u, "leaf" if kind == "unit_leaf" else "root")
        return _make(name, pos, last, pairs, Dn, Vp, bn, lam, "%s: %s" % (base, what), "definite", None, claims)
    if name in INDEFINITE_NAMES:
        if name == "isolated_zero":
            c = get("isolated_lam0")
            u = ISOLATED_NODES[4]
            Dn = c.Dn.copy()
            Dn[u] = 0.0
            return _make(name, c.pos, c.last, c.pairs, Dn, c.Vp, c.bn, 0.0, "an exactly zero block on an isolated node, lam = 0", "zero", "isolated_lam0", dict(), dict(node=u))
        base, kind = name.split("_", 1)
        c = get(base)
        Dn, Vp = c.Dn.copy(), c.Vp.copy()
        if kind == "late":
            fr, nd = _fronts_nodes(c.pos, c.last, c.pairs)
            q = next(q for q, (a, b) in enumerate(c.pairs) if nd[a][0] != nd[b][0] and 0 in (fr[nd[a][0]][0], fr[nd[b][0]][0]))
            Vp[q] = 4.0 * max(Dn[i][j, j] for i in range(len(Dn)) for j in range(3)) * np.eye(3)
            return _make(name, c.pos, c.last, c.pairs, Dn, Vp, c.bn, c.lam, "%s: a coupling block outweighs the positive definite diagonal blocks" % base, "indefinite", base,
                         dict(), dict(pair=q))
        where = {"neg_c0": dict(level=0, s=96, col_min=0, col_max=15), "neg_c16": dict(level=0, s=96, col_min=16, col_max=79), "neg_c80": dict(level=0, s=96, col_min=80),
                 "neg_mid": dict(mid=True), "neg_root": dict(root=True)}[kind]
        if base == "b150" and kind != "neg_root":
            where["wg_min"] = 4                                    # (three row-block workgroups and the inverse one, at least)
        u = _pick_node(c.pos, c.last, c.pairs, where)
        Dn[u] = -Dn[u]
        return _make(name, c.pos, c.last, c.pairs, Dn, Vp, c.bn, c.lam, "%s: a negated diagonal block at %r" % (base, where), "indefinite", base, dict(), dict(node=u, where=where))
    raise KeyError(name)


def args(c):
    """the arguments of CPU.nd_solve / ctx.debug_nd_solve"""
    return c.pos, c.last, c.pairs, c.Dn, c.Vp, c.bn, c.lam


def measure_host(name):
    """(eta_host, fwd_host, stats) of the host reference on a definite case"""
    c = get(name)
    ok, x, st = CPU.nd_solve(*args(c))
    assert ok, name
    eta, fwd = errors(c.A, c.bn, x, c.xref)
    return eta, fwd, st


# name: (eta_host, fwd_host) -- measured by test_nd_cases_cpu.py, which fails if an entry is off by more than a factor of two
HOST = {
    "s3": (1.047e-16, 2.407e-16),
    "s15": (1.336e-16, 4.007e-16),
    "s18": (9.873e-17, 3.505e-16),
    "s48": (1.080e-16, 3.740e-16),
    "s51": (1.469e-16, 4.298e-16),
    "s93": (3.155e-16, 1.020e-15),
    "s96": (1.955e-16, 6.441e-16),
    "b0": (2.438e-16, 7.860e-16),
    "b3": (1.405e-16, 3.866e-16),
    "b45": (6.593e-17, 4.582e-16),
    "b48": (5.835e-17, 2.412e-16),
    "b51": (8.981e-17, 9.486e-16),
    "b96": (1.333e-16, 2.120e-15),
    "b99": (6.218e-17, 8.886e-16),
    "b150": (6.373e-17, 9.308e-16),
    "b1056": (1.182e-16, 2.501e-15),
    "s51b48": (6.702e-17, 6.432e-16),
    "grid": (3.349e-16, 1.105e-15),
    "gridpose": (1.093e-17, 7.807e-16),
    "gridpose_nolast": (1.092e-17, 7.807e-16),
    "path": (7.137e-17, 2.704e-16),
    "star": (9.104e-18, 3.094e-16),
    "isolated": (4.330e-17, 1.901e-16),
    "n1": (8.145e-17, 1.756e-16),
    "n2": (7.711e-17, 2.339e-16),
    "grid_lam0": (2.269e-16, 8.022e-16),
    "grid_ill": (2.410e-16, 2.957e-09),
    "grid_dn40": (3.349e-16, 1.105e-15),
    "grid_up40": (3.349e-16, 1.105e-15),
    "grid_unit_leaf": (5.521e-17, 3.423e-16),
    "grid_unit_root": (2.277e-17, 7.221e-17),
    "b150_lam0": (6.497e-17, 1.055e-15),
    "b150_ill": (2.664e-16, 7.249e-09),
    "b150_dn40": (6.373e-17, 9.308e-16),
    "b150_up40": (6.373e-17, 9.308e-16),
    "b150_unit_leaf": (8.583e-17, 2.750e-16),
    "b150_unit_root": (1.707e-17, 2.675e-16),
    "isolated_lam0": (1.767e-17, 2.080e-16),
}


if __name__ == "__main__":
    for nm in DEFINITE_NAMES:
        e, f, _ = measure_host(nm)
        print('    "%s": (%.3e, %.3e),' % (nm, e, f))
