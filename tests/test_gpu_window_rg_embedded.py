"""GPU: nrs_dba_solve_window_rg_embedded (include/nrs.h) -- the embedded BA window served by the device-resident all-pairs graph --
against the same window on the device's own FULL lists (nrs_rgraph_get_edges at capacity - 1 -> nrs_dba_build_edges_embedded /
nrs_dba_solve_window_embedded), against the oracle's lists (embedded_oracle.dba_build_embedded) and against the C++ restatement of
embedded_oracle.dba_solve_embedded at the tolerances of tests/test_gpu_embedded_ba.py.  Inputs: tests/window_rg_embedded_cases.py."""
import numpy as np
import pytest

import embedded_oracle as E
import nrs
import nrs_cpu as CPU
import nrs_synth as S
import window_rg_embedded_cases as WE
from test_gpu_window_rg import _device_graph, _full_lists, _qt, _trace_bits

pytestmark = pytest.mark.gpu

LISTS = ("lm_obs", "sp_ij", "sp_d0", "dm_idx", "dm_w", "sk_obs", "sk_node", "sk_omega")
_ref = {}


def _reference(ctx, c, rg):
    """per case, computed once and shared (left unchanged): the device graph's full lists, the host lists on them, the oracle's lists and
    nrs_dba_solve_window_embedded on the full lists"""
    if c["name"] not in _ref:
        p, n, nb = c["p"], c["n"], c["nbr"]
        full = _full_lists(rg, n)
        for k in ("rowptr", "col", "status"):                      # the graph itself is tests/test_gpu_rgraph.py's subject; here it pins the input
            assert np.array_equal(full[k], nb[k]), k
        host = nrs.dba_build_edges_embedded(p["kf_points"], c["flag"], full)
        ora = E.dba_build_embedded(p["kf_points"], c["flag"], nb["rowptr"], nb["col"], nb["w"], nb["d0"], nb["status"])
        tr = nrs.Trace()
        pq, xyz = ctx.dba_solve_window_embedded(nrs.make_camera(p["model"], p["prm"]), _qt(p), p["kf_points"], p["lm_xyz"], p["lm_uv"], c["flag"], full,
                                                p["scale"], 5, tr)
        _ref[c["name"]] = dict(host=host, ora=ora, pq=pq, xyz=xyz, trace=_trace_bits(tr))
    return _ref[c["name"]]


def _solve(ctx, c, rg, first_cap, flag=None, trace=None):
    p = c["p"]
    return ctx.dba_solve_window_rg_embedded(nrs.make_camera(p["model"], p["prm"]), _qt(p), p["kf_points"], p["lm_xyz"], p["lm_uv"], rg,
                                            c["flag"] if flag is None else flag, p["scale"], 5, trace, first_cap)


@pytest.mark.parametrize("first_cap", [0, 8])
@pytest.mark.parametrize("name", WE.CASES)
def test_lists_and_solve_are_those_of_the_full_lists(ctx, name, first_cap):
    c = WE.case(name)
    rg = _device_graph(ctx, c)
    try:
        ref = _reference(ctx, c, rg)
        tr = nrs.Trace()
        pq, xyz = _solve(ctx, c, rg, first_cap, trace=tr)
        dev, stats = ctx.dba_window_edges_embedded(), ctx.dba_window_rg_stats()
    finally:
        rg.close()
    # ---- the lists: index for index, bit for bit, sk_omega included
    assert dev["on_device"] == 1
    for key in LISTS:
        assert dev[key].dtype == ref["host"][key].dtype and np.array_equal(dev[key], ref["host"][key]), key
        assert np.array_equal(dev[key], ref["ora"][key]), key
    assert len(dev["sp_d0"]) > 0 and len(dev["dm_w"]) > 0 and len(dev["sk_obs"]) > 0
    # ---- the statistics: the CPU restatement's
    first = first_cap if first_cap > 0 else 64                     # the documented default first prefix
    cap, rounds = WE.final_cap(c, first, c["n"])
    assert stats["n_points"] == len(np.unique(np.concatenate(c["p"]["kf_points"])))
    assert stats["cap"] == cap and stats["rounds"] == rounds and rounds >= 2
    assert stats["ran_off_first"] == WE.walks_that_run_off(c, first)[0] > 0
    # ---- the solve: the bits of nrs_dba_solve_window_embedded on the full lists
    assert np.array_equal(pq, ref["pq"]) and np.array_equal(xyz, ref["xyz"])
    assert _trace_bits(tr) == ref["trace"] and len(tr.trials) >= 5
    moved = np.zeros(len(xyz), bool)
    moved[dev["lm_obs"]] = True
    moved[dev["sk_obs"]] = True
    assert (~moved).any() and np.array_equal(xyz[~moved], c["p"]["lm_xyz"][~moved])       # observations bound to nothing stay


@pytest.mark.parametrize("name", WE.CASES)
def test_solve_matches_the_oracle(ctx, name):
    """the C++ twin of embedded_oracle.dba_solve_embedded (tests/test_oracle_cpp_cpu.py holds it to the oracle) on the device-built lists,
    with the comparisons of tests/test_gpu_embedded_ba.py test_solve_matches_oracle"""
    c = WE.case(name)
    p = c["p"]
    rg = _device_graph(ctx, c)
    try:
        tr = nrs.Trace()
        pq, xyz = _solve(ctx, c, rg, 0, trace=tr)
        e = ctx.dba_window_edges_embedded()
    finally:
        rg.close()
    w = S.embedded_window(p, e)
    oq, ot, opts, osk, otr, _ = CPU.dba_solve_embedded(p["model"], p["prm"], p["poses_q"], p["poses_t"], w["lm_xyz"], w["lm_kf"], w["lm_uv"], e["sp_ij"], e["sp_d0"],
                                                       e["dm_idx"], e["dm_w"], w["sk_kf"], w["sk_uv"], w["sk_xyz"], e["sk_node"], e["sk_omega"], p["scale"], 5)
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
    assert np.allclose(xyz[e["lm_obs"]], opts, atol=1e-4, rtol=0)
    assert np.allclose(xyz[e["sk_obs"]], osk, atol=1e-4, rtol=0)


@pytest.mark.parametrize("name", WE.CASES)
def test_every_point_a_node_is_the_plain_window_on_the_graph(ctx, name):
    c = WE.case(name)
    p = c["p"]
    rg = _device_graph(ctx, c)
    try:
        tr0 = nrs.Trace()
        pq0, xyz0 = ctx.dba_solve_window_rg(nrs.make_camera(p["model"], p["prm"]), _qt(p), p["kf_points"], p["lm_xyz"], p["lm_uv"], rg, p["scale"], 5, tr0)
        plain, stats0 = ctx.dba_window_edges(), ctx.dba_window_rg_stats()
        tr = nrs.Trace()
        pq, xyz = _solve(ctx, c, rg, 0, flag=np.ones(c["n"], np.uint8), trace=tr)
        e, stats = ctx.dba_window_edges_embedded(), ctx.dba_window_rg_stats()
    finally:
        rg.close()
    assert e["on_device"] == 1 and len(e["sk_obs"]) == 0 and np.array_equal(e["lm_obs"], np.arange(len(p["lm_xyz"])))
    for key in ("sp_ij", "sp_d0", "dm_idx", "dm_w"):
        assert np.array_equal(e[key], plain[key]), key
    assert stats == stats0
    assert len(tr.trials) >= 5 and _trace_bits(tr) == _trace_bits(tr0)
    assert np.array_equal(pq, pq0) and np.array_equal(xyz, xyz0)


def _taps_are_gone(ctx):
    for tap in (ctx.dba_window_edges_embedded, ctx.dba_window_rg_stats):
        with pytest.raises(nrs.NrsError) as e:
            tap()
        assert e.value.code == -5                                  # NRS_ERR_STATE


def test_a_walk_that_runs_off_at_the_limit_is_refused(ctx):
    c = WE.case(WE.SMALL)
    assert WE.walks_that_run_off(c, 16)[0] > 0
    rg = _device_graph(ctx, c)
    try:
        _solve(ctx, c, rg, 8)                                       # a window is resident ...
        assert ctx.dba_window_rg_stats()["rounds"] >= 2
        nrs.debug_set("NRS_RG_MAX_CAP", 16)
        with pytest.raises(nrs.NrsError) as e:
            _solve(ctx, c, rg, 8)
        assert e.value.code == -1 and "ran off" in str(e.value) and "limit of 16" in str(e.value) and "nrs_dba_solve_window_rg_embedded" in str(e.value)
        _taps_are_gone(ctx)                                         # ... and is gone after the refused call
        nrs.debug_set("NRS_RG_MAX_CAP", None)
        _solve(ctx, c, rg, 8)
        assert ctx.dba_window_rg_stats()["cap"] == WE.final_cap(c, 8, c["n"])[0] and ctx.dba_window_edges_embedded()["on_device"] == 1
    finally:
        nrs.debug_set("NRS_RG_MAX_CAP", None)
        rg.close()


def test_refusals(ctx):
    c = WE.case(WE.SMALL)
    p = c["p"]
    cam = nrs.make_camera(p["model"], p["prm"])
    rg = _device_graph(ctx, c)

    def refused(what, kf_points=p["kf_points"], flag=c["flag"], graph=rg, on=ctx):
        _solve(ctx, c, rg, 0)                                       # a window is resident ...
        with pytest.raises(nrs.NrsError) as e:
            on.dba_solve_window_rg_embedded(cam, _qt(p), kf_points, p["lm_xyz"], p["lm_uv"], graph, flag, p["scale"], 5)
        assert e.value.code == -1 and what in str(e.value), str(e.value)
        if on is ctx:
            _taps_are_gone(ctx)                                     # ... and is gone after the refused call

    other = nrs.Context()
    try:
        refused("bad argument", flag=None)                          # null is_node
        pts = [k.copy() for k in p["kf_points"]]
        pts[1][3] = c["n"]                                          # an index beyond the graph's capacity
        refused("beyond the graph", kf_points=pts)
        pts = [k.copy() for k in p["kf_points"]]                    # a node twice in a keyframe: the same number of observations
        node_here = pts[1][c["flag"][pts[1]] != 0]
        assert len(node_here) >= 2
        pts[1][np.where(pts[1] == node_here[1])[0][0]] = node_here[0]
        refused("listed twice", kf_points=pts)
        nrs.debug_set("NRS_RG_MAX_CAP", 16)                         # ... refused before any GetEdges round: not as the run-off at the limit
        with pytest.raises(nrs.NrsError) as e:
            ctx.dba_solve_window_rg_embedded(cam, _qt(p), pts, p["lm_xyz"], p["lm_uv"], rg, c["flag"], p["scale"], 5, None, 8)
        nrs.debug_set("NRS_RG_MAX_CAP", None)
        assert e.value.code == -1 and "listed twice" in str(e.value)
        empty = [np.zeros(0, np.int32) for _ in p["kf_points"]]     # argument checks name the call
        with pytest.raises(nrs.NrsError) as e:
            ctx.dba_solve_window_rg_embedded(cam, _qt(p), empty, p["lm_xyz"][:0], p["lm_uv"][:0], rg, c["flag"], p["scale"], 5)
        assert e.value.code == -1 and "nrs_dba_solve_window_rg_embedded: empty window" in str(e.value)
        rg_other = _device_graph(other, c)                          # a graph of another context
        try:
            refused("another context", graph=rg_other)
        finally:
            rg_other.close()
    finally:
        other.close()
        rg.close()
    # a communicator on the context (a world of one)
    grp = nrs.LocalGroup(1)
    c2 = nrs.Context()
    try:
        c2.comm_init_local(grp, 0)
        rg2 = _device_graph(c2, c)
        try:
            with pytest.raises(nrs.NrsError) as e:
                c2.dba_solve_window_rg_embedded(cam, _qt(p), p["kf_points"], p["lm_xyz"], p["lm_uv"], rg2, c["flag"], p["scale"], 5)
            assert e.value.code == -1 and "communicator" in str(e.value)
        finally:
            rg2.close()
    finally:
        c2.close()
        grp.close()
