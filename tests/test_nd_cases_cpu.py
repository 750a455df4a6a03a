"""The designed systems of tests/nd_cases.py, vetted without a GPU: the plan of every case is sound (nrs_cpu_nd_plan_check), its front table
(CPU.nd_plan_fronts / nd_plan_nodes: taps of the product's nrs_nd_plan.hpp) shows every shape the case claims, the host reference
(oracle/nd_host.cpp through CPU.nd_solve) agrees with the high-precision reference, reports every indefinite case and no definite one, and
the eigenvalue / condition-number conditions of the cases hold.  It also MEASURES the two figures tests/test_gpu_nd_cases.py builds its
bounds from -- eta_host and fwd_host, see nd_cases.HOST -- prints them with the shapes reached (pytest -s), and holds the table to them."""
import numpy as np
import pytest

import nrs_cpu as CPU
import nd_cases as K


def _eig(c):
    w = np.linalg.eigvalsh(c.A)
    return float(w[0]), float(w[-1])


def test_the_shape_targets_are_all_reached():
    """every own-block and boundary size the kernels' constants single out is the (s, b) of some front of some shape case"""
    s_seen, b_seen = set(), set()
    for name in K.SHAPE_NAMES:
        c = K.get(name)
        fr = CPU.nd_plan_fronts(c.pos, c.last, c.pairs)
        s_seen |= set(fr[:, 2].tolist())
        b_seen |= set(fr[:, 3].tolist())
    assert {3, 15, 18, 48, 51, 93, 96} <= s_seen
    assert {0, 3, 45, 48, 51, 96, 99} <= b_seen and max(b_seen) >= 147


@pytest.mark.parametrize("name", K.DEFINITE_NAMES)
def test_definite_case(name):
    c = K.get(name)
    assert c.kind == "definite" and np.isfinite(c.A).all() and np.isfinite(c.bn).all()
    assert CPU.nd_plan_check(c.pos, c.last, c.pairs) == 0
    fr = CPU.nd_plan_fronts(c.pos, c.last, c.pairs)
    nd = CPU.nd_plan_nodes(c.pos, c.last, c.pairs)
    level, parent, s, b, wg = fr.T
    assert (nd[:, 0] >= 0).all() and s.sum() == 3 * len(c.pos)
    # ---- the shapes the case claims
    cl = c.claims
    if "fronts" in cl:
        assert len(fr) == cl["fronts"]
    for sb in cl.get("sb", ()):
        assert sb in set(zip(s.tolist(), b.tolist())), (sb, fr.tolist())
    if "wg" in cl:                                                 # the claimed front's workgroups: every (I >= J) pair of row blocks and the inverse one
        f = [i for i in range(len(fr)) if (s[i], b[i]) == cl["sb"][0]][0]
        assert wg[f] == cl["wg"] and (b[f] < 147 or wg[f] >= 11)   # (from four row blocks on there are workgroups with I > J > 0)
    assert level.max() + 1 >= cl.get("levels_min", 1)
    if cl.get("chain"):                                            # a separator too long for one front: a front with ONE child, and more than 96 unknowns between them
        assert any(parent[f] >= 0 and (parent == parent[f]).sum() == 1 and s[f] + s[parent[f]] > 96 for f in range(len(fr)))
    if cl.get("one_node_separator"):
        assert any(s[f] == 3 and level[f] > 0 for f in range(len(fr)))
    if name == "star":                                             # the hub is dissected like any node: it ends up in a separator, above the spokes
        assert level[nd[0][0]] > 0
    if name == "isolated":
        assert all(not (c.pairs == u).any() for u in K.ISOLATED_NODES)
    if "rhs_node" in cl:
        u, where = cl["rhs_node"]
        assert np.count_nonzero(c.bn) == 1 and c.bn[u, 1] == 1.0
        assert level[nd[u][0]] == 0 if where == "leaf" else parent[nd[u][0]] < 0
        assert level.max() > 0
    if name.startswith("grid_"):
        assert level.max() >= 4                                    # the numeric cases run on a system of several levels ...
    if name.startswith("b150_"):
        assert wg.max() >= 11                                      # ... and on one whose front has four row blocks
    # ---- conditioning
    lo, hi = _eig(c)
    if "cond" in cl:
        cond = np.linalg.cond(c.A)
        assert cl["cond"][0] < cond < cl["cond"][1], cond
        dominant = np.abs(np.diag(c.A)) > np.abs(c.A).sum(1) - np.abs(np.diag(c.A))
        assert not dominant.any()                                  # no row is diagonally dominant
        assert c.lam == pytest.approx(1e-9 * np.diag(c.A - c.lam * np.eye(len(c.A))).max(), rel=1e-6)
    else:
        assert lo > 1e-3 * hi, (lo, hi)
    if "same_solution_as" in cl:
        assert np.array_equal(c.xref, K.get(cl["same_solution_as"]).xref) or np.allclose(np.asarray(c.xref, float), np.asarray(K.get(cl["same_solution_as"]).xref, float), rtol=1e-15, atol=0)
    # ---- the host reference against the high-precision reference; the two figures of the table
    eta, fwd, st = K.measure_host(name)
    assert st["fronts"] == len(fr) and st["max_s"] == s.max() and st["max_b"] == b.max() and st["workgroups"] == wg.sum()
    cond_inf = np.linalg.cond(c.A, np.inf)
    print("\n%-16s %s | fronts %d levels %d, (s, b): %s | cond_inf %.2e eta_host %.3e fwd_host %.3e" % (
        name, c.what, len(fr), level.max() + 1, sorted(set(zip(s.tolist(), b.tolist())))[-6:], cond_inf, eta, fwd))
    assert eta <= 16 * K.EPS                                       # backward stable
    assert fwd <= 2 * cond_inf * eta + 4 * K.EPS                   # |dx| / |x| <= cond (|r| / (|A| |x|)), and eta's denominator is at most twice |A| |x|
    te, tf = K.HOST[name]
    for measured, table in ((eta, te), (fwd, tf)):
        assert table / 2 <= measured <= 2 * table, "nd_cases.HOST[%r] is stale: measured (%.3e, %.3e)" % (name, eta, fwd)


@pytest.mark.parametrize("name", K.INDEFINITE_NAMES)
def test_indefinite_case(name):
    c = K.get(name)
    twin = K.get(c.twin)
    assert twin.kind == "definite" and np.isfinite(c.A).all()
    assert CPU.nd_plan_check(c.pos, c.last, c.pairs) == 0
    for a, b in zip(K.args(c)[:3] + (c.bn, c.lam), K.args(twin)[:3] + (twin.bn, twin.lam)):       # the same system ...
        assert np.array_equal(a, b)
    fr = CPU.nd_plan_fronts(c.pos, c.last, c.pairs)
    nd = CPU.nd_plan_nodes(c.pos, c.last, c.pairs)
    level, parent, s, b, wg = fr.T
    lo, hi = _eig(c)
    if c.kind == "zero":
        u = c.defect["node"]
        assert c.lam == 0.0 and not c.Dn[u].any() and not (c.pairs == u).any() and not c.A[3 * u:3 * u + 3].any()
        assert np.count_nonzero((c.Dn != twin.Dn).any((1, 2))) == 1
    else:
        assert lo < -1e-3 * hi, (lo, hi)                           # ... indefinite with a margin
        if "pair" in c.defect:                                     # late: only the coupling differs, every diagonal block is positive definite on its own,
            q = c.defect["pair"]                                   # and so is everything eliminated before the front that owns the pair's later node
            assert np.array_equal(c.Dn, twin.Dn) and np.count_nonzero((c.Vp != twin.Vp).any((1, 2))) == 1 and (c.Vp[q] != twin.Vp[q]).any()
            assert all(np.linalg.eigvalsh(D + c.lam * np.eye(3))[0] > 0 for D in c.Dn)
            fa, fb = nd[c.pairs[q][0]][0], nd[c.pairs[q][1]][0]
            lo_f, hi_f = (fa, fb) if level[fa] < level[fb] else (fb, fa)
            assert level[lo_f] == 0 and level[hi_f] > 0
            late = set()
            f = hi_f
            while f >= 0:
                late.add(f)
                f = parent[f]
            assert lo_f not in late
            early = np.array([u for u in range(len(c.pos)) if nd[u][0] not in late])
            rows = (3 * early[:, None] + np.arange(3)).ravel()
            assert np.linalg.eigvalsh(c.A[np.ix_(rows, rows)])[0] > 0
        else:
            u = c.defect["node"]
            assert np.array_equal(c.Vp, twin.Vp) and np.array_equal(c.Dn[u], -twin.Dn[u]) and np.count_nonzero((c.Dn != twin.Dn).any((1, 2))) == 1
            f, col = nd[u]
            w = c.defect["where"]
            if w.get("root"):
                assert parent[f] < 0 and level[f] == level.max() > 0
                if c.twin == "b150":
                    assert c.last[u]                               # the pose
            if w.get("mid"):
                assert 0 < level[f] < level.max() and parent[f] >= 0 and (parent == f).any()
            if "level" in w:
                assert level[f] == w["level"] and s[f] == w["s"] and w["col_min"] <= col <= w.get("col_max", 95)
            if "wg_min" in w:
                assert wg[f] >= 4 and b[f] + 1 > 2 * 48            # at least three row blocks
    ok, x, st = CPU.nd_solve(*K.args(c))
    okt, xt, stt = CPU.nd_solve(*K.args(twin))
    print("\n%-16s %s | eigenvalues %.3e .. %.3e | host: ok %s, twin %s ok %s" % (name, c.what, lo, hi, ok, c.twin, okt))
    assert not ok and okt and st == stt
