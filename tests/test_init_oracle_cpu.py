"""CPU: the monocular map initialisation (include/nrs.h f6) -- the new entry points are declared, listed and exported; the NumPy restatement
(tests/init_oracle.py) recovers a known motion; every case of tests/init_cases.py stays inside the bands the GPU test excuses, and the two
measured tolerances recorded there are the ones this file measures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import init_cases as IC
import init_oracle as IO
import nrs_synth as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["nrs_init_options_init", "nrs_init_essential"]


def test_new_symbols_are_declared_listed_and_exported(lib_built):
    nrs = lib_built
    lib = nrs.load_library()
    hdr = open(os.path.join(ROOT, "include", "nrs.h")).read()
    declared = set(re.findall(r"\b(nrs_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in nrs.SYMBOLS and hasattr(lib, name), name
    assert "} nrs_init_options;" in hdr and "} nrs_init_result;" in hdr
    # the records the binding hands over have the header's layout
    assert C.sizeof(nrs.InitOptions) == 40 and nrs.InitOptions.seed.offset == 32
    assert C.sizeof(nrs.InitResult) == 184 and nrs.InitResult.counters.offset == 24 and nrs.InitResult.E.offset == 56
    assert nrs.InitResult.pose_qt.offset == 92 and nrs.InitResult.inlier.offset == 120 and nrs.InitResult.centres.offset == 176
    opt = nrs.InitOptions()
    lib.nrs_init_options_init(C.byref(opt))                  # host code only: no device needed
    assert (opt.struct_size, opt.n_hypotheses, opt.min_triangulated, opt.compact_indexing, opt.seed) == (40, 0, 100, 0, 4)
    assert (opt.epipolar_threshold, opt.max_low_parallax) == (np.float32(0.005), np.float32(0.25))


def test_compute_max_tries_is_16():
    assert IO.compute_max_tries() == 16


def test_hash_is_splitmix64():
    # splitmix64's first outputs for the state 0 are its published test vector; seed + (k + 1) * golden is that generator's state sequence
    assert [IO.init_hash(0, k) for k in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


@pytest.mark.parametrize("model", [S.PINHOLE, S.KB8])
def test_oracle_recovers_a_noise_free_motion(model):
    p = S.make_init_pair(n=300, seed=21, model=model, noise_px=0.0)
    o = IO.initialize(p["model"], p["prm"], p["ref_xy"], p["cur_xy"], p["status"], p["n_matches"], radians_per_pixel=IC.RPP[model])
    assert o["verdict"] == 0 and o["score"] == 300 and o["counters"][1] == 300
    x, y, z, w = o["pose_q"].astype(np.float64)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    assert np.max(np.abs(R - p["R"])) < 2e-4                 # fp32 keypoints (1e-5 px) over a 4 mm baseline at 60 mm
    t_true = p["t"] / np.linalg.norm(p["t"])
    assert abs(np.linalg.norm(o["pose_t"]) - 1) < 1e-6 and np.max(np.abs(o["pose_t"] - t_true)) < 2e-3
    # the map comes out at unit baseline: true points / |t|
    m = o["code"] == 0
    assert np.max(np.abs(o["xyz"][m] - p["X"][m] / np.linalg.norm(p["t"])) / np.linalg.norm(p["X"][m] / np.linalg.norm(p["t"]), axis=1)[:, None]) < 5e-3


def test_cases_say_what_the_gpu_test_needs():
    assert IC.oracle("outlier30", 16)["verdict"] != 0 and IC.oracle("outlier30", 1024)["verdict"] == 0
    assert IC.oracle("rotation", 16)["verdict"] in (2, 3)
    a, b = IC.oracle("untracked", 16, 0), IC.oracle("untracked", 16, 1)
    assert not np.array_equal(a["code"], b["code"]) and not np.array_equal(a["counters"], b["counters"])
    # the exact best_hypothesis comparison of the GPU test runs on these: their winning margin exceeds twice the largest excusable count
    for name in ("pinhole300", "kb8_300", "untracked"):
        p, o = IC.case(name), IC.oracle(name, 16)
        _, rr, cr = IC.rays(name)
        excusable = max(int(np.sum(np.abs(IO.score(E, rr, cr, p["n_matches"], np.float32(0.005))[1] - float(np.float32(0.005))) < IC.SCORE_BAND))
                        for E in o["hyp_E"])
        top = np.sort(o["hyp_score"])[::-1]
        assert int(top[0] - top[1]) > 2 * excusable, name
    for nc in IC.SAMPLER_COMPACT:
        p = IC.sampler_case(nc)
        assert int((p["status"] == 1).sum()) == nc
    lab, _, smp = IO.sampler(IC.sampler_case(8)["ref_xy"][IC.sampler_case(8)["status"] == 1], 16, 4)
    assert sorted(lab) == list(range(8)) and all(sorted(lab[s]) == list(range(8)) for s in smp)      # 8 points: every cluster one member


def test_two_fp64_methods_set_the_hypothesis_tolerance():
    worst = 0.0
    for name in IC.HYP_CASES:
        _, rr, cr = IC.rays(name)
        for s in IC.samples(name, 256)[2]:
            a = IO.compute_E(rr[s], cr[s])
            b = IO.align_sign(IO.compute_E_eigh(rr[s], cr[s]), a)
            worst = max(worst, float(np.max(np.abs(a.astype(np.float64) - b))))
    print("largest disagreement of the two fp64 methods: %.3g (recorded %.3g, tolerance %.3g)" % (worst, IC.HYP_E_MEASURED, IC.HYP_E_TOL))
    assert worst <= IC.HYP_E_MEASURED


@pytest.mark.parametrize("name,n_hyp", [("pinhole300", 16), ("kb8_300", 16), ("untracked", 16), ("outlier30", 1024), ("rotation", 16), ("whole4000", 1024)])
def test_cases_stay_inside_the_bands(name, n_hyp):
    p, o = IC.case(name), IC.oracle(name, n_hyp)
    _, rr, cr = IC.rays(name)
    near = total = 0
    for E in o["hyp_E"]:
        err = IO.score(E, rr, cr, p["n_matches"], np.float32(0.005))[1]
        near += int(np.sum(np.abs(err - float(np.float32(0.005))) < IC.SCORE_BAND))
        total += len(err)
    print("%s: %d of %d (hypothesis, point) pairs within %.0e rad of the threshold" % (name, near, total, IC.SCORE_BAND))
    assert near <= IC.SCORE_CAP * total
    visited = np.isfinite(o["margins"])
    close = int(np.sum(o["margins"][visited] < IC.GATE_BAND))
    print("%s: %d of %d visited points within %.0e of a gate" % (name, close, int(visited.sum()), IC.GATE_BAND))
    assert close <= IC.GATE_CAP * max(int(visited.sum()), 1)


def test_fp32_against_fp64_mid_point_sets_the_xyz_tolerance():
    worst = 0.0
    for name, nh in (("pinhole300", 16), ("kb8_300", 16), ("untracked", 16), ("outlier30", 1024), ("whole4000", 1024)):
        p, o = IC.case(name), IC.oracle(name, nh)
        for kp in np.where(o["code"] == 0)[0]:
            x64 = IO.triangulate64(p["ref_xy"][kp], p["cur_xy"][kp], p["model"], p["prm"], o["pose_q"], o["pose_t"])
            worst = max(worst, float(np.linalg.norm(o["xyz"][kp] - x64) / np.linalg.norm(x64)))
    print("largest relative fp32 / fp64 mid-point difference: %.3g (recorded %.3g, tolerance %.3g)" % (worst, IC.XYZ_MEASURED, IC.XYZ_RTOL))
    assert worst <= IC.XYZ_MEASURED
