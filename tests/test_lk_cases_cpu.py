"""CPU: the Lucas-Kanade case table (tests/lk_cases.py) on the two CPU restatements of the tracker, oracle/lk_oracle.py (NumPy) and
oracle/nrs_cpu_lk.hpp (C++, behind nrs_cpu.LucasKanadeCpp): no case raises, every builder's own non-emptiness assertions hold, the two
agree exactly, and the two rules DESIGN.md 4 "Lucas-Kanade tracker" defines hold on both -- a tracker configured with more levels than
the tracked image's pyramid has is the tracker configured with exactly that many, and a position that is not finite or does not fit an
int is outside the image."""
import numpy as np
import pytest

import lk_cases as LC
import nrs_cpu as CPU


@pytest.fixture(scope="module")
def cpu_lib():
    CPU.build()
    return CPU.load()


def _run_cpp(c, lib, **cfg):
    k = dict(c["cfg"], **cfg)
    lk = CPU.LucasKanadeCpp(21, k["max_level"], k["max_iters"], k["epsilon"], k["min_eig"], lib=lib)
    try:
        lk.set_reference(c["im0"], c["pts"])
        t = lk.templates()
        return t, lk.track(c["im1"], c["guess"], c["status"], c["initial_flow"], c["min_ssim"])
    finally:
        lk.close()


def _same_result(a, b):
    assert np.array_equal(a[0], b[0], equal_nan=True)                               # xy, NaN positions included
    assert np.array_equal(a[1], b[1]) and a[2] == b[2]                              # status, n_good
    assert np.array_equal(a[3], b[3], equal_nan=True)                               # SSIM (NaN where the gate was not reached)


@pytest.mark.parametrize("name", LC.NAMES)
def test_case_builds_and_the_oracle_returns(name):
    """the builder's own assertions (its case is not empty) and an oracle that returns instead of raising; unusable points come back
    with the guess's bits and their input status"""
    c = LC.case(name)
    t, (xy, st, good, ssim) = LC.oracle(name)
    assert 15 <= len(c["pts"]) <= 40
    un = ~np.isin(c["status"], LC.USABLE)
    assert np.array_equal(st[un], c["status"][un]) and np.array_equal(xy[un].view(np.uint32), c["guess"][un].view(np.uint32))
    assert good == int(((st == c["status"]) & ~un).sum())                           # n_good = the usable points that stay usable
    assert np.all(t["mean"][t["valid"] == 0] == -1)


def test_table_reaches_every_status_code():
    LC.vet_table()


def test_ssim_gate_decides_only_non_finite_positions():
    """the checked statement of how far the SSIM gate's position test can be reached (tests/lk_cases.py vet_ssim_gate_reach)"""
    LC.vet_ssim_gate_reach()


@pytest.mark.parametrize("name", LC.UNMASKED)
def test_numpy_and_cpp_agree_exactly(cpu_lib, name):
    c = LC.case(name)
    t, r = LC.oracle(name)
    tc, rc = _run_cpp(c, cpu_lib)
    for k in ("valid", "mean", "gray", "grad"):                                     # templates and means at every level
        assert np.array_equal(t[k], tc[k]), k
    _same_result(r, rc)


@pytest.mark.parametrize("name", LC.SHORT)
def test_short_pyramid_is_the_tracker_of_its_top_level(cpu_lib, name):
    """on a pyramid of k levels, max_level >= k returns bit for bit what max_level = k - 1 returns (both restatements)"""
    c = LC.case(name)
    h, w = c["im0"].shape
    k = LC.n_levels(w, h, c["cfg"]["max_level"])
    assert k <= c["cfg"]["max_level"]
    _, r = LC.oracle(name)
    _, r_top = LC.run_oracle(c, max_level=k - 1)
    _same_result(r, r_top)
    _same_result(_run_cpp(c, cpu_lib)[1], _run_cpp(c, cpu_lib, max_level=k - 1)[1])
    _, r_more = LC.run_oracle(c, max_level=k)                                       # (and one level more than it has, below the default)
    _same_result(r, r_more)


def test_short_pyramid_finds_the_flow():
    """161 x 123 with the default five-level configuration (3 levels built): the median error of the status-0 points against the
    synthetic flow is under the 0.5 px bar of tests/test_gpu_klt.py, and all 15 points track"""
    c = LC.case("short_161x123")
    _, (xy, st, good, _) = LC.oracle("short_161x123")
    assert good == len(st) == 15 and np.all(st == 0)
    err = np.linalg.norm(xy[st == 0] - c["truth"][st == 0], axis=1)
    print("median error %.4f px over %d points" % (np.median(err), len(err)))
    assert np.median(err) < 0.5
