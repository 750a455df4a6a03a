"""The direct solver's device kernels (nr-slam_amd/csrc/nrs_nd_kernels.hpp k_nd_level / k_nd_tile / k_nd_back, through the C ABI tap
nrs_debug_nd_solve) on the designed systems of tests/nd_cases.py, against a dense high-precision solve and the host reference of the same
plan (oracle/nd_host.cpp).  Stands for LinearSolverEigen::solve (third_party/g2o/g2o/solvers/eigen/linear_solver_eigen.h:92-136).

Bounds (conditions, not measurements of the device): the normwise backward error |b - A x|inf / (|A|inf |x|inf + |b|inf), residual in
np.longdouble, is at most max(8 eta_host, 64 eps), and the forward error against the refined reference at most max(8 fwd_host, 1e-11) --
the device sums in another order (four-deep matrix-core accumulation, tiles) and forms its pivots by reciprocal square root, both backward
stable with constants of a few units; a lost tile, a wrong lane map or a missed right-hand-side row lands orders of magnitude above.
eta_host / fwd_host are the host reference's figures in nd_cases.HOST, which tests/test_nd_cases_cpu.py measures and holds the table to.
Every test prints the device's figures next to their bounds (pytest -s)."""
import numpy as np
import pytest

import nrs
import nrs_cpu as CPU
import nd_cases as K

pytestmark = pytest.mark.gpu


def _bounds(name):
    eta_host, fwd_host = K.HOST[name]
    return max(8 * eta_host, 64 * K.EPS), max(8 * fwd_host, 1e-11)


def _check(c, x, tag=""):
    eta, fwd = K.errors(c.A, c.bn, x, c.xref)
    eta_max, fwd_max = _bounds(c.name)
    print("\n%-16s %-26s backward %.3e (<= %.3e)  forward %.3e (<= %.3e)" % (c.name, tag, eta, eta_max, fwd, fwd_max))
    assert eta <= eta_max, (c.name, tag, eta, eta_max)
    assert fwd <= fwd_max, (c.name, tag, fwd, fwd_max)


@pytest.mark.parametrize("name", K.DEFINITE_NAMES)
def test_definite_case(ctx, name):
    c = K.get(name)
    ok, x, st, _ = ctx.debug_nd_solve(*K.args(c))
    okh, xh, sth = CPU.nd_solve(*K.args(c))
    assert ok and okh and st == sth
    _check(c, x)
    ok2, x2, _, _ = ctx.debug_nd_solve(*K.args(c))
    assert ok2 and np.array_equal(x, x2)                           # fixed summation order: the same bits


@pytest.mark.parametrize("name", K.INDEFINITE_NAMES)
def test_indefinite_case_is_reported_and_leaves_nothing_behind(ctx, name):
    c = K.get(name)
    twin = K.get(c.twin)
    ok0, x0, _, _ = ctx.debug_nd_solve(*K.args(twin))
    assert ok0
    ok, x, st, _ = ctx.debug_nd_solve(*K.args(c))
    print("\n%-16s %s: ok %s" % (name, c.what, ok))
    assert not ok                                                  # linear_solver_eigen.h:124-136: reported, not hidden
    # (the panel by 16-column steps is the third place that factorises a diagonal block; the flag is raised per workgroup, whatever its width or launch)
    for sw in ({"NRS_ND_STEP32": "0"}, {"NRS_ND_THREADS": "256"}, {"NRS_ND_CHAIN": "1"}):
        for k, v in sw.items():
            nrs.debug_set(k, v)
        try:
            okf, _, _, _ = ctx.debug_nd_solve(*K.args(c))
        finally:
            nrs.debug_clear()
        assert not okf, sw
    ok1, x1, _, _ = ctx.debug_nd_solve(*K.args(twin))               # the definite twin right afterwards, on the same context
    assert ok1 and np.array_equal(x0, x1)
    _check(twin, x1, "after " + name)


# the launch forms the solver has (nrs_switches.hpp "direct solver"; tests/test_gpu_nd.py promises the same bits for every one of them):
# the top of the tree chained in one launch or a launch per level, 256-thread workgroups, the panel by 16-column steps, the back pass
# handing over by flags, crowded levels in one launch instead of two
LAUNCH_FORMS = (
    {"NRS_ND_CHAIN": "1"},
    {"NRS_ND_CHAIN": "1", "NRS_ND_LEVELS": "1"},
    {"NRS_ND_LEVELS": "1"},
    {"NRS_ND_THREADS": "256"},
    {"NRS_ND_THREADS": "256", "NRS_ND_STEP32": "0"},
    {"NRS_ND_STEP32": "0"},
    {"NRS_ND_BACK_FLAGS": "1"},
    {"NRS_ND_NO_SPLIT": "1"},
    {"NRS_ND_NO_SPLIT": "1", "NRS_ND_THREADS": "256"},
)


@pytest.mark.parametrize("name", K.LAUNCH_FORM_NAMES)
def test_every_launch_form(ctx, name):
    c = K.get(name)
    nrs.debug_clear()
    ok, x, st, _ = ctx.debug_nd_solve(*K.args(c))
    assert ok
    _check(c, x, "default")
    for sw in LAUNCH_FORMS:
        for k, v in sw.items():
            nrs.debug_set(k, v)
        try:
            ok2, x2, st2, _ = ctx.debug_nd_solve(*K.args(c))
        finally:
            nrs.debug_clear()
        assert ok2 and st2 == st, sw
        _check(c, x2, " ".join("%s=%s" % (k[4:], v) for k, v in sw.items()))
        assert np.array_equal(x, x2), sw
