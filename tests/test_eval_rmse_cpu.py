"""nrs_eval_rmse (include/nrs.h "f7: evaluation"; host code, no device) against tests/eval_oracle.py bit for bit: rmse, scale, counts and
the inlier mask, for the aligned and the unaligned form, with and without precomputed_depth."""
import numpy as np
import pytest

import eval_oracle as E

F32 = np.float32
FORMS = [(a, p) for a in (True, False) for p in (False, True)]


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


def _same(dev, ora):
    rmse, scale, counts, inl, rc = dev
    o_rmse, o_scale, o_counts, o_inl = ora
    assert counts == tuple(o_counts)
    assert np.array_equal(_bits(rmse), _bits(o_rmse)) and np.array_equal(_bits(scale), _bits(o_scale)), (rmse, o_rmse, scale, o_scale)
    assert np.array_equal(inl, o_inl)
    assert (rc == 0) == bool(np.isfinite(o_rmse))
    if rc != 0:
        assert rc == -1 and np.isnan(rmse) and np.isnan(scale)


def _depths(n, seed, k=1.7, noise=0.01, drop=0.15):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(2.0, 6.0, n).astype(F32)
    est = (gt / F32(k) + rng.normal(0, noise, n).astype(F32)).astype(F32)
    ok = rng.uniform(0, 1, n) > drop
    if n <= 3:
        ok[:] = True
    return est, gt, ok


@pytest.mark.parametrize("n", [1, 2, 3, 10, 11, 257])
@pytest.mark.parametrize("align,pre", FORMS)
def test_rmse_matches_the_oracle_bit_for_bit(lib_built, n, align, pre):
    """n = 1: (int)(1 * 0.9f) = 0 inliers, the error return; 2 and 3: the smallest sizes with a result; 10 / 11: where (int)(n * 0.9f)
    steps; 257: a size with a tail"""
    est, gt, ok = _depths(n, 100 + n)
    ora = E.eval_rmse(est, gt, ok, align, pre)
    _same(lib_built.eval_rmse(est, gt, ok, align, pre), ora)
    if n == 1:
        assert np.isnan(ora[0]) and ora[2] == (1, 1, 0)
    else:
        assert np.isfinite(ora[0]) and ora[2][2] >= 1


@pytest.mark.parametrize("align,pre", FORMS)
def test_no_valid_point_and_empty_input_are_errors(lib_built, align, pre):
    est, gt, _ = _depths(5, 3)
    for e, g, ok in ((est, gt, np.zeros(5, bool)), (est[:0], gt[:0], np.zeros(0, bool))):
        _same(lib_built.eval_rmse(e, g, ok, align, pre), E.eval_rmse(e, g, ok, align, pre))
        assert lib_built.eval_rmse(e, g, ok, align, pre)[4] == -1


@pytest.mark.parametrize("align,pre", FORMS)
def test_exact_ties_at_the_inlier_threshold(lib_built, align, pre):
    """more values at the threshold than n_inliers holds: the first n_inliers in index order are taken (aligned form); in the unaligned
    form nothing is strictly below the threshold and the missing residuals count as 0"""
    n = 20
    est = np.full(n, 2.0, F32)
    gt = np.full(n, 2.5, F32)
    ok = np.ones(n, bool)
    ora = E.eval_rmse(est, gt, ok, align, pre)
    dev = lib_built.eval_rmse(est, gt, ok, align, pre)
    _same(dev, ora)
    n_inl = ora[2][2]
    assert n_inl == (19 if (align and pre) else 18)
    if align:                                                     # twenty equal residuals: the first n_inliers are the inliers
        assert dev[3][:n_inl].all() and not dev[3][n_inl:].any()
        assert dev[1] == F32(1.25) and dev[0] == 0
    else:
        assert dev[3].sum() == 0 and dev[0] == 0
    gt[3], gt[11] = 2.25, 2.25                                    # two values apart, eighteen equal ones
    _same(lib_built.eval_rmse(est, gt, ok, align, pre), E.eval_rmse(est, gt, ok, align, pre))


@pytest.mark.parametrize("align,pre", FORMS)
def test_gross_outliers_are_dropped_by_the_iqr_gate(lib_built, align, pre):
    est, gt, ok = _depths(120, 8, k=1.0, noise=0.003, drop=0.0)
    bad = np.arange(0, 120, 17)
    gt[bad] += F32(40)
    ora = E.eval_rmse(est, gt, ok, align, pre)
    dev = lib_built.eval_rmse(est, gt, ok, align, pre)
    _same(dev, ora)
    if align and pre:                                             # precomputed_depth bypasses the gate
        assert dev[2][1] == 120
    else:
        # (the gate also takes the few largest of the Gaussian errors)
        assert 100 < dev[2][1] <= 120 - len(bad) and not dev[3][bad].any() and dev[0] < 0.02


def test_a_known_scale_is_recovered(lib_built):
    est, gt, ok = _depths(257, 21, k=1.7, noise=0.002)
    for pre in (False, True):
        rmse, scale, counts, inl, rc = lib_built.eval_rmse(est, gt, ok, True, pre)
        assert rc == 0 and abs(float(scale) - 1.7) < 5e-3 and float(rmse) < 0.01
        _same((rmse, scale, counts, inl, rc), E.eval_rmse(est, gt, ok, True, pre))
    rmse, scale, _, _, rc = lib_built.eval_rmse(est, gt, ok, False, False)
    assert rc == 0 and scale == 1 and float(rmse) > 0.5           # unaligned: the scale error is the residual
