"""GPU parity of the kernel variants the engine's launchers choose among (csrc/nrs_engine_launch.hpp): every lane count of the sliced-ELL
layout (NRS_SELL_T = 1, 2, 4, 8, 16) on the fused, two-kernel, temporal-difference and gather paths, the lanes = 2 lineariser / operator
forms of large plain windows (compact headers, re-formed factors, non-temporal streams) and the embedded window's merged operator launch.
The defaults reach lanes 2 and 8 only; the other arms are pinned here.

Tolerances are those of tests/test_gpu_dba.py and, between two forms of the same arithmetic, of its dform test."""
import numpy as np
import pytest

import embedded_oracle as E
import embedded_window_cases as W
import nrs
import nrs_oracle as O
import nrs_synth as S

pytestmark = pytest.mark.gpu

LANES = [1, 2, 4, 8, 16]
PATHS = {"fused": {}, "two-kernel": {"NRS_NO_FUSED": "1"}, "dform": {"NRS_NO_FUSED": "1", "NRS_DFORM": "1"}, "gather": {"NRS_NO_LDS": "1"}}
_cache = {}


def _switches(env):
    for k, v in env.items():
        nrs.debug_set(k, v)


def _clear(env):
    for k in env:
        nrs.debug_set(k, None)


def _window(n, k, seed, model):
    """problem, edges, camera, poses; built once per module, shared and left unchanged"""
    key = ("window", n, k, seed, model)
    if key not in _cache:
        p = S.make_dba_problem(n, k, seed, model)
        e = nrs.dba_build_edges(p["kf_points"], p["nbr"])
        _cache[key] = (p, e, nrs.make_camera(p["model"], p["prm"]), np.concatenate([p["poses_q"], p["poses_t"]], 1))
    return _cache[key]


def _small_oracle(model):
    key = ("oracle", model)
    if key not in _cache:
        p, e, cam, qt = _window(500, 5, 34, model)
        otr = []
        oq, ot, opts, nit = O.dba_solve(p["model"], p["prm"], p["poses_q"], p["poses_t"], p["lm_xyz"], p["lm_kf"], p["lm_uv"],
                                        e["sp_ij"], e["sp_d0"], e["dm_idx"], e["dm_w"], p["scale"], 5, otr)
        _cache[key] = (oq, ot, opts, nit, otr)
    return _cache[key]


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("model,lanes", [(S.PINHOLE, t) for t in LANES] + [(S.KB8, 2), (S.KB8, 8)])
def test_every_lane_count_on_every_path_matches_the_oracle(ctx, model, lanes, path):
    """500 points x 5 keyframes (the window of test_two_kernel_path_with_temporal_difference_dampers, same assertions): k_pcg_fused<T>,
    k_spmv_f<T, dform> + k_reg / k_lin_plain<T>, k_spmv<T> + k_reg<T, ., false>"""
    p, e, cam, qt = _window(500, 5, 34, model)
    oq, ot, opts, nit, otr = _small_oracle(model)
    env = dict(PATHS[path], NRS_SELL_T=str(lanes))
    try:
        _switches(env)
        tr = nrs.Trace()
        pq, xyz = ctx.dba_solve(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"], 5, tr)
    finally:
        _clear(env)
    assert tr.iterations == nit and [t["accepted"] for t in tr.trials] == [t["accepted"] for t in otr]
    for a, o in zip(tr.trials, otr):
        assert abs(a["lam"] - o["lam"]) <= 1e-6 * o["lam"] and abs(a["chi"] - o["chi"]) <= 1e-6 * o["chi"]
        if not a["early"]:
            assert abs(a["chi_new"] - o["chi_new"]) <= 1e-6 * o["chi_new"]
    assert np.allclose(pq[:, :4], oq, atol=1e-6, rtol=0) and np.allclose(pq[:, 4:], ot, atol=1e-5, rtol=0)
    assert np.allclose(xyz, opts, atol=1e-4, rtol=0)


def _large_run(model, env):
    """5000 x 8 (the window of test_compact_damper_headers_change_nothing: two-kernel path, lanes = 2, compact headers), fresh context"""
    key = ("large", model, tuple(sorted(env.items())))
    if key not in _cache:
        p, e, cam, qt = _window(5000, 8, 21, model)
        try:
            _switches(env)
            c = nrs.Context()
            c.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"])
            h = c.dba_pack_hash()
            tr = nrs.Trace(64)
            c.dba_optimize(4, tr)
            pq, xyz = c.dba_download()
            c.close()
        finally:
            _clear(env)
        _cache[key] = (h, tr.trials, pq, xyz)
    return _cache[key]


@pytest.mark.parametrize("case", ["NRS_RC=0", "NRS_RC=1", "NRS_RC=2", "NRS_RC=3", "NRS_NT=1", "NRS_NO_H4=1"])
@pytest.mark.parametrize("model", [S.PINHOLE, S.KB8])
def test_lanes_2_operator_and_lineariser_variants(model, case):
    """k_lin_plain<2, 4, CAM, true, 0, H4, RCS, RCD, ., NT> / k_spmv_f<2, false, TPC, H4, RCS, RCD, NT> against the 8-byte-header run
    (NRS_NO_H4=1: the TPC form).  NRS_RC=0 and NRS_NT=1 are an encoding and a load hint: the same bits.  NRS_RC=1..3 re-form the
    spring / damper factors in the operator instead of storing them: the same arithmetic grouped differently, held at what the
    dform test holds its two forms to."""
    name, value = case.split("=")
    h8, t8, q8, x8 = _large_run(model, {"NRS_NO_H4": "1"})
    h, t, q, x = _large_run(model, {name: value} if name != "NRS_NO_H4" else {})      # (the baseline itself: against the default run)
    assert h[20] != h8[20], "the variant must run on compact headers (the flag is part of the scalar checksum)"
    if case in ("NRS_RC=0", "NRS_NT=1", "NRS_NO_H4=1"):
        tup = lambda tt: [(a["accepted"], a["early"], a["inner"], a["lam"], a["chi"], a["chi_new"]) for a in tt]
        assert tup(t) == tup(t8)
        assert np.array_equal(q, q8) and np.array_equal(x, x8)
    else:
        assert [a["accepted"] for a in t] == [a["accepted"] for a in t8]
        assert np.allclose(q, q8, atol=1e-9, rtol=0) and np.allclose(x, x8, atol=1e-7, rtol=0)
        # (the outputs cannot show that the switch was taken: the re-formed factors are the stored ones to the last bit on this window.
        # Dev::rc is set from NRS_RC wherever compact headers are on -- engine_compact_headers -- which the checksum above shows.)


@pytest.mark.parametrize("lanes", LANES)
def test_embedded_window_operator_at_every_lane_count(ctx_emb_pcg, lanes):
    """k_spmv_f_skin<T>: the smallest window of tests/embedded_window_cases.py on the block-Jacobi PCG, held to the oracle as
    tests/test_gpu_embedded_ba.py test_solve_matches_oracle holds it"""
    n, k, m, seed, model, kw = W.CASES[0]
    key = ("embedded", seed)
    if key not in _cache:
        p, flag, nb = W.window(W.CASES[0], "nodes")
        e = nrs.dba_build_edges_embedded(p["kf_points"], flag, nb)
        w = S.embedded_window(p, e)
        otr = []
        ora = E.dba_solve_embedded(p["model"], p["prm"], p["poses_q"], p["poses_t"], w["lm_xyz"], w["lm_kf"], w["lm_uv"], e["sp_ij"], e["sp_d0"],
                                   e["dm_idx"], e["dm_w"], w["sk_kf"], w["sk_uv"], w["sk_xyz"], e["sk_node"], e["sk_omega"], p["scale"], 5, otr)
        _cache[key] = (p, e, w, ora, otr)
    p, e, w, (oq, ot, opts, osk, nit), otr = _cache[key]
    assert len(e["sk_obs"]) > 0.7 * len(p["lm_kf"])
    cam = nrs.make_camera(p["model"], p["prm"])
    qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
    env = {"NRS_SELL_T": str(lanes)}
    try:
        _switches(env)
        tr = nrs.Trace()
        pq, xyz, sk = ctx_emb_pcg.dba_solve_embedded(cam, qt, w, e, p["scale"], 5, tr)
    finally:
        _clear(env)
    assert tr.iterations == nit
    assert [t["accepted"] for t in tr.trials] == [t["accepted"] for t in otr]
    for a, b in zip(tr.trials, otr):
        assert (a["iter"], a["trial"]) == (b["iter"], b["trial"])
        assert abs(a["lam"] - b["lam"]) <= 1e-6 * b["lam"]
        assert abs(a["chi"] - b["chi"]) <= 1e-6 * b["chi"]
        if a["early"]:
            assert not a["accepted"] and not b["accepted"] and b["rho"] < -0.02
        else:
            assert abs(a["chi_new"] - b["chi_new"]) <= 1e-6 * b["chi_new"]
    assert np.allclose(pq[:, :4], oq, atol=1e-6, rtol=0)
    assert np.allclose(pq[:, 4:], ot, atol=1e-5, rtol=0)
    assert np.allclose(xyz, opts, atol=1e-4, rtol=0)
    assert np.allclose(sk, osk, atol=1e-4, rtol=0)
    assert sum(t["inner"] for t in tr.trials if not t["early"]) > 20 * len(tr.trials)
