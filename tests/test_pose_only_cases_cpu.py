"""CPU: the a1 case table (tests/pose_only_cases.py) on the two CPU restatements of CameraPoseOptimization, oracle/nrs_oracle.py (NumPy)
and oracle/nrs_cpu_track.hpp (C++, behind nrs_cpu.pose_only_solve): what tests/test_gpu_pose_only_forms.py relies on when it holds the
device to the NumPy oracle.  The two agree on every case (identical inlier masks, traces to the noise floor, pose to a1's bar from 6
points on), no case has a point in the gate band (at most 2 on the hand-over pair), and the control-flow cases do what they are named
after.  Below 6 points the two oracles' pose disagreement is MEASURED and printed: the constants in pose_only_cases.py come from it."""
import numpy as np
import pytest

import nrs_cpu as CPU
import pose_only_cases as PC


@pytest.fixture(scope="module")
def cpu_lib():
    CPU.build()
    return CPU.load()


@pytest.fixture(scope="module")
def cpp(cpu_lib):
    cache = {}

    def run(name):
        if name not in cache:
            c = PC.case(name)
            cache[name] = CPU.pose_only_solve(c["model"], c["prm"], c["uv"], c["X"], c["pose_q"], c["pose_t"], cpu_lib)
        return cache[name]
    return run


def test_sizes_are_exact():
    for n in PC.LADDER_PINHOLE + PC.HANDOVER + PC.NARROW_PINHOLE:
        c = PC.case("pin_%d" % n)
        assert c["uv"].shape == (n, 2) and c["X"].shape == (n, 3) and c["uv"].dtype == c["X"].dtype == np.float32
    for n in PC.LADDER_KB8 + PC.NARROW_KB8:
        assert PC.n_points("kb8_%d" % n) == n
    big = PC.case("pin_%d" % PC.HANDOVER[1])                                        # slices of ONE problem
    assert np.array_equal(PC.case("pin_513")["uv"], big["uv"][:513]) and np.array_equal(PC.case("pin_7169")["X"], big["X"][:7169])
    assert set(PC.NARROW) <= set(PC.NAMES) and len(set(PC.NAMES)) == len(PC.NAMES)


@pytest.mark.parametrize("name", PC.NAMES)
def test_numpy_and_cpp_agree(cpp, name):
    o = PC.oracle(name)
    q, t, inl, tr, _ = cpp(name)
    n = PC.n_points(name)
    assert np.all(np.isfinite(o["q"])) and np.all(np.isfinite(o["t"])) and np.all(np.isfinite(q)) and np.all(np.isfinite(t))
    assert np.array_equal(inl, o["inl"])
    compared = PC.compare_traces(tr, name)
    dq, dt = np.abs(q - o["q"]).max(), np.abs(t - o["t"]).max()
    print("%s: n %d, trials per round %s, compared %d%s, iterations %d, inliers %d, band %d, |dq| %.2e, |dt| %.2e" % (
        name, n, [len(r) for r in o["rounds"]], compared, " (to the end)" if o["to_the_end"] else "", o["iterations"], o["inl"].sum(),
        o["n_band"], dq, dt))
    assert compared >= 1 and len(o["rounds"][0]) >= 1
    if n >= 6:
        assert dq <= PC.TOL_Q and dt <= PC.TOL_T
    else:
        # the GPU bar of this size: 10 x the oracles' own disagreement, floored at a1's bar, and no looser than that
        tq, tt = PC.tolerance(name)
        assert 10 * dq <= tq and 10 * dt <= tt
        assert tq == PC.TOL_Q or tq <= 30 * dq
        assert tt == PC.TOL_T or tt <= 30 * dt
    if o["to_the_end"]:
        assert len(tr) == len(o["trace"])
        assert sum(len({(y["round"], y["iter"]) for y in tr if y["round"] == r}) for r in range(3)) == o["iterations"]


@pytest.mark.parametrize("name", PC.NAMES)
def test_gate_band(name):
    """no point's chi2 within 1e-6 (relative) of the 5.99 gate, at any of the three classifications; at most 2 above 12000 points"""
    o = PC.oracle(name)
    assert o["n_band"] <= PC.GATE_BAND_MAX
    if PC.n_points(name) <= 12000:
        assert o["n_band"] == 0


def test_far_seed_rejects_three_in_a_row():
    """an iteration of round 0 with at least 3 consecutive rejected trials, among the trials that are compared with the device"""
    o = PC.oracle("far_seed")
    assert PC.n_points("far_seed") == 600
    assert PC.rejection_run(PC.compared_prefix(o["rounds"][0])) >= 3
    assert all(len(r) > 0 for r in o["rounds"])


def test_all_outliers_leaves_two_empty_rounds():
    o = PC.oracle("all_outliers_after_round0")
    assert len(o["rounds"][0]) > 0 and o["empty_rounds"] == [1, 2] and o["rounds"][1] == [] and o["rounds"][2] == []
    assert not o["inl"].any()


def test_behind_camera(cpp):
    c = PC.case("behind_camera")
    z = PC.depth_at_seed(c)
    assert len(z) == 300 and (z < 0).sum() == PC.N_BEHIND and not (z == 0).any() and np.abs(z).min() > 1e-3
    o = PC.oracle("behind_camera")
    assert np.all(np.isfinite(o["q"])) and np.all(np.isfinite(o["t"]))
    assert all(np.isfinite([y["chi"], y["chi_new"], y["lam"], y["rho"]]).all() for y in o["trace"])
    assert not o["inl"][z < 0].any() and o["inl"].sum() > 250                       # the mirrored points end as outliers, the rest fit
