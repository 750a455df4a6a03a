"""GPU: nrs_dba_solve_window_rg (include/nrs.h) -- LocalDeformableBundleAdjustment served by the device-resident all-pairs graph --
against the same window on the device's own FULL lists (nrs_rgraph_get_edges at capacity - 1 -> nrs_dba_build_edges / nrs_dba_solve_window)
and against the oracle (DenseGraph.get_edges -> dba_build -> dba_solve).  Inputs: tests/window_rg_cases.py."""
import os
import sys

import numpy as np
import pytest

import nrs
import nrs_oracle as O
import window_rg_cases as W

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_window_rg_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu


def _device_graph(ctx, c):
    """nrs_rgraph_create at capacity n, all-pairs add_edges at the start positions, one update at the perturbed ones"""
    ids = np.arange(c["n"], dtype=np.int32)
    rg = nrs.RGraph(ctx, c["n"], c["sigma"], W.STRETCH_TH)
    rg.add_edges(c["X0"], ids, ids)
    rg.update(c["X1"], ids)
    return rg


def _full_lists(rg, n):
    cnt, col, w, d0, st = rg.get_edges(np.arange(n, dtype=np.int32), n - 1)
    assert cnt.max() <= n - 1
    rowptr = np.zeros(n + 1, np.int32)
    rowptr[1:] = np.cumsum(cnt)
    keep = np.arange(n - 1)[None, :] < cnt[:, None]
    return dict(rowptr=rowptr, col=col[keep], w=w[keep], d0=d0[keep], status=st[keep])


def _qt(p):
    return np.concatenate([p["poses_q"], p["poses_t"]], 1)


def _same_edges(a, b):
    return all(np.array_equal(np.asarray(a[k]).reshape(-1), np.asarray(b[k]).reshape(-1)) and np.asarray(a[k]).dtype == np.asarray(b[k]).dtype
               for k in ("sp_ij", "sp_d0", "dm_idx", "dm_w"))


def _trace_bits(tr):
    return [(t["iter"], t["trial"], t["accepted"], t["ok"], t["inner"], t["lam"], t["chi"], t["chi_new"], t["rho"]) for t in tr.trials]


def _check(ctx, name, first_cap):
    c = W.case(name)
    p, n = c["p"], c["n"]
    cam = nrs.make_camera(p["model"], p["prm"])
    rg = _device_graph(ctx, c)
    try:
        full = _full_lists(rg, n)
        # the device's full lists are the oracle's (the graph itself is tests/test_gpu_rgraph.py's subject; here it pins the input)
        for k in ("rowptr", "col", "status"):
            assert np.array_equal(full[k], c["nbr"][k]), k
        tr = nrs.Trace()
        pq, xyz = ctx.dba_solve_window_rg(cam, _qt(p), p["kf_points"], p["lm_xyz"], p["lm_uv"], rg, p["scale"], 5, tr, first_cap)
        edges, stats = ctx.dba_window_edges(), ctx.dba_window_rg_stats()
        assert edges is not None
        # ---- the edge lists: index for index, bit for bit
        host = nrs.dba_build_edges(p["kf_points"], full)
        assert _same_edges(edges, host)
        eo = O.dba_build(p["kf_points"], c["nbr"]["rowptr"], c["nbr"]["col"], c["nbr"]["w"], c["nbr"]["d0"], c["nbr"]["status"])
        assert np.array_equal(edges["sp_ij"], eo["sp_ij"]) and np.array_equal(edges["dm_idx"], eo["dm_idx"])
        assert np.array_equal(edges["sp_d0"], eo["sp_d0"]) and np.array_equal(edges["dm_w"], eo["dm_w"])
        assert len(edges["sp_d0"]) > 0 and len(edges["dm_w"]) > 0
        # ---- the solve: the bits of nrs_dba_solve_window on the full lists
        tr2 = nrs.Trace()
        pq2, xyz2 = ctx.dba_solve_window(cam, _qt(p), p["kf_points"], p["lm_xyz"], p["lm_uv"], full, p["scale"], 5, tr2)
        assert np.array_equal(pq, pq2) and np.array_equal(xyz, xyz2)
        assert _trace_bits(tr) == _trace_bits(tr2) and len(tr.trials) >= 5
        return c, pq, xyz, tr, edges, stats
    finally:
        rg.close()


@pytest.mark.parametrize("name", list(W.CASES))
def test_window_on_the_resident_graph_is_the_window_on_its_full_lists(ctx, name):
    c, pq, xyz, tr, edges, stats = _check(ctx, name, 0)
    p = c["p"]
    assert stats["n_points"] == len(np.unique(np.concatenate(p["kf_points"])))
    cap, rounds = W.final_cap(c, 64, c["n"])                      # the documented default first prefix
    assert stats["cap"] == cap and stats["rounds"] == rounds and stats["ran_off_first"] == W.walks_that_run_off(c, 64)[0]
    # ---- nrs_oracle.dba_solve at the tolerances of tests/test_gpu_dba.py: run here on the small window, read from the golden on the two
    # larger ones (minutes of dense solves: tests/golden/make_window_rg_golden.py), which must be the golden of THIS problem
    if name in G.GOLDEN_CASES:
        z = np.load(G.path(name))
        assert str(z["checksum"]) == G.problem_checksum(p, edges)
        oq, ot, opts, accepted = z["q"], z["t"], z["pts"], [bool(a) for a in z["accepted"]]
    else:
        otr = []
        oq, ot, opts, _ = O.dba_solve(p["model"], p["prm"], p["poses_q"], p["poses_t"], p["lm_xyz"], p["lm_kf"], p["lm_uv"], edges["sp_ij"], edges["sp_d0"],
                                      edges["dm_idx"], edges["dm_w"], p["scale"], 5, otr)
        accepted = [t["accepted"] for t in otr]
    assert [t["accepted"] for t in tr.trials] == accepted
    assert np.allclose(pq[:, :4], oq, atol=1e-6, rtol=0) and np.allclose(pq[:, 4:], ot, atol=1e-5, rtol=0)
    assert np.allclose(xyz, opts.astype(np.float32), atol=1e-4, rtol=0)


@pytest.mark.parametrize("name", ["120x3", "900x6_kb8"])
def test_a_short_first_prefix_is_retried_until_no_walk_runs_off(ctx, name):
    c = W.case(name)
    ran, total = W.walks_that_run_off(c, 8)
    assert 0 < ran < total                                         # walks that run off at 8 entries, and walks that do not
    cap, rounds = W.final_cap(c, 8, c["n"])
    assert cap < c["n"] - 1 and rounds >= 2                        # ... and the window is served by prefixes, not by the whole lists
    _, _, _, _, _, stats = _check(ctx, name, 8)                    # lists and result equal the full-list run
    assert stats["rounds"] >= 2 and stats["rounds"] == rounds and stats["cap"] == cap
    assert stats["ran_off_first"] == ran


def test_a_walk_that_runs_off_at_the_limit_is_refused(ctx):
    c = W.case("120x3")
    assert W.walks_that_run_off(c, 16)[0] > 0
    p = c["p"]
    rg = _device_graph(ctx, c)
    try:
        nrs.debug_set("NRS_RG_MAX_CAP", 16)
        with pytest.raises(nrs.NrsError) as e:
            ctx.dba_solve_window_rg(nrs.make_camera(p["model"], p["prm"]), _qt(p), p["kf_points"], p["lm_xyz"], p["lm_uv"], rg, p["scale"], 5, None, 8)
        assert e.value.code == -1 and "ran off" in str(e.value) and "limit of 16" in str(e.value)
        with pytest.raises(nrs.NrsError) as e2:                    # no window is left behind
            ctx.dba_window_rg_stats()
        assert e2.value.code == -5
        nrs.debug_set("NRS_RG_MAX_CAP", None)
        ctx.dba_solve_window_rg(nrs.make_camera(p["model"], p["prm"]), _qt(p), p["kf_points"], p["lm_xyz"], p["lm_uv"], rg, p["scale"], 5, None, 8)
        assert ctx.dba_window_rg_stats()["cap"] == 64
    finally:
        nrs.debug_set("NRS_RG_MAX_CAP", None)
        rg.close()


def test_refusals(ctx):
    c = W.case("120x3")
    p = c["p"]
    cam = nrs.make_camera(p["model"], p["prm"])
    rg = _device_graph(ctx, c)
    try:
        pts = [k.copy() for k in p["kf_points"]]
        pts[1][3] = c["n"]                                         # an index beyond the graph's capacity
        with pytest.raises(nrs.NrsError) as e:
            ctx.dba_solve_window_rg(cam, _qt(p), pts, p["lm_xyz"], p["lm_uv"], rg, p["scale"])
        assert e.value.code == -1 and "beyond the graph" in str(e.value)
    finally:
        rg.close()
    # a communicator on the context (a world of one): sharded forms of the call do not exist
    grp = nrs.LocalGroup(1)
    c2 = nrs.Context()
    try:
        c2.comm_init_local(grp, 0)
        rg2 = _device_graph(c2, c)
        try:
            with pytest.raises(nrs.NrsError) as e:
                c2.dba_solve_window_rg(cam, _qt(p), p["kf_points"], p["lm_xyz"], p["lm_uv"], rg2, p["scale"])
            assert e.value.code == -1 and "communicator" in str(e.value)
        finally:
            rg2.close()
    finally:
        c2.close()
        grp.close()
