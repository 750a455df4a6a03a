"""Cases of the monocular map initialisation tests (tests/test_init_oracle_cpu.py, tests/test_gpu_init.py): built once, shared, never changed.

Bands and tolerances (the CPU test asserts that the cases stay inside them, so the GPU test cannot excuse more than it says):
  SCORE_BAND   2e-6 rad: a (hypothesis, point) pair whose fp64 error lies this close to the threshold may flip; one fp32 ulp at pi/2
               (1.2e-7) plus a few ulp of the dot product, slope 1, rounded up.  At most 1 % of the pairs of a case
  GATE_BAND    1e-5 relative: a point this close to a gate of ReconstructPoints may change its code.  At most 1 % of the points of a case
  HYP_E_TOL    max(4 fp32 ulp of 1, 10 x the largest disagreement of the oracle's two fp64 methods over all hypotheses of HYP_CASES);
               measured 2.1e-7 (eigh on A^T A against the SVD, after both are rounded to fp32; the noisy pure rotation sets it), so 10 x that =
               2.1e-6 decides
  XYZ_RTOL     4 x the largest relative difference between the oracle's fp32 mid-point and the same in fp64 over the triangulated points
               of the cases; measured 1.2e-6, so 4.8e-6
  POSE_TOL     4 fp32 ulp of 1 per rotation entry and per component of the unit translation"""
import functools

import numpy as np

import init_oracle as IO
import nrs_synth as S

F32 = np.float32
ULP1 = float(np.finfo(F32).eps)
SCORE_BAND, SCORE_CAP = 2e-6, 0.01
GATE_BAND, GATE_CAP = 1e-5, 0.01
HYP_E_MEASURED = 2.1e-7
HYP_E_TOL = max(4 * ULP1, 10 * HYP_E_MEASURED)
XYZ_MEASURED = 1.2e-6
XYZ_RTOL = 4 * XYZ_MEASURED
POSE_TOL = 4 * ULP1
RPP = {S.PINHOLE: F32(1.0 / 766.380279), S.KB8: F32(1.0 / 358.6052)}          # radians per pixel: 1 / fx (tracking.cc:65)

SPECS = {
    "pinhole300": dict(n=300, seed=1, model=S.PINHOLE),
    "kb8_300": dict(n=300, seed=2, model=S.KB8),
    "untracked": dict(n=333, seed=3, model=S.PINHOLE, untracked_frac=0.1),
    "outlier30": dict(n=300, seed=4, model=S.PINHOLE, outlier_frac=0.3),
    "rotation": dict(n=300, seed=5, model=S.PINHOLE, baseline=0.0),
    "whole4000": dict(n=4000, seed=6, model=S.PINHOLE, outlier_frac=0.1, untracked_frac=0.05),
}
HYP_CASES = ("pinhole300", "kb8_300", "outlier30", "rotation")
SAMPLER_COMPACT = (8, 9, 137, 300)


@functools.lru_cache(maxsize=None)
def case(name):
    p = S.make_init_pair(**SPECS[name])
    p["rpp"] = RPP[p["model"]]
    return p


@functools.lru_cache(maxsize=None)
def sampler_case(n_compact):
    """n_compact TRACKED keypoints with 10 % untracked ones interleaved"""
    n = n_compact + n_compact // 9 + 1
    p = S.make_init_pair(n=n, seed=10 + n_compact, model=S.PINHOLE, untracked_frac=0.1)
    extra = int((p["status"] == 1).sum()) - n_compact             # trim from the end to the exact compact count
    idx = np.where(p["status"] == 1)[0]
    if extra > 0:
        p["status"][idx[-extra:]] = 3
    assert int((p["status"] == 1).sum()) == n_compact and int((p["status"] != 1).sum()) >= 1
    p["n_matches"] = n_compact
    p["rpp"] = RPP[p["model"]]
    return p


@functools.lru_cache(maxsize=None)
def rays(name):
    p = case(name)
    return IO.compact_unproject(p["model"], p["prm"], p["ref_xy"], p["cur_xy"], p["status"])


@functools.lru_cache(maxsize=None)
def samples(name, n_hyp, seed=4):
    p = case(name)
    cmap = rays(name)[0]
    return IO.sampler(p["ref_xy"][cmap], n_hyp, seed)


@functools.lru_cache(maxsize=None)
def oracle(name, n_hyp, compact_indexing=0):
    p = case(name)
    return IO.initialize(p["model"], p["prm"], p["ref_xy"], p["cur_xy"], p["status"], p["n_matches"], n_hypotheses=n_hyp,
                         radians_per_pixel=p["rpp"], compact_indexing=compact_indexing)


# ---- end to end (tests/test_gpu_init_loop.py): the device's hyp_E may differ from the oracle's by HYP_E_TOL, and everything behind it follows.
#   POSE_E2E_TOL  R and t come from the SVD of an E whose singular values (1, 1, 0) are a gap of 1 apart: a perturbation dE turns the singular
#                 vectors by at most 2 |dE|_F <= 6 HYP_E_TOL, and R = U W V^T collects two such turns: 12 HYP_E_TOL per entry
#   XYZ_E2E_RTOL  a mid-point moves by the pose error over the parallax angle, relative to its depth; accepted points have a parallax of at
#                 least 5 radians_per_pixel (the gate), 1 / 76.6 rad for the 320-wide calibration of make_init_sequence: POSE_E2E_TOL x 76.6,
#                 plus XYZ_RTOL.  The scale (3 / median depth) and sigma (a deviation of depths, times scale) inherit that relative bound
LOOP_KLT = dict(win=21, max_level=3, max_iters=10, epsilon=1e-4, min_eig=1e-4)   # (a 320 x 240 pyramid has 4 levels with a 21-pixel window)
POSE_E2E_TOL = 12 * HYP_E_TOL
XYZ_E2E_RTOL = POSE_E2E_TOL * 76.6 + XYZ_RTOL


@functools.lru_cache(maxsize=None)
def init_sequence():
    sq = S.make_init_sequence(n_points=500, n_frames=8, seed=3)
    mask = np.zeros((240, 320), np.uint8)
    mask[20:-20, 20:-20] = 255                                 # BorderFilter-like: the tracker's window stays inside the image
    sq["mask"] = mask
    return sq
