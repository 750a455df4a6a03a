"""GPU parity of a2 (nrs_track_deform_solve, _rg, _embedded) on frames that are a permuted, partial view of the map: frame slot, map id,
index among the optimised points, vertex and GetEdges row are five different numbers (tests/track_frame_cases.py; the other a2 tests
pass f_map = arange(n)).  Scene A drives the device walk (nrs_rgraph.hip k_rg_walk) through several 64-entry chunks per list, growing
prefixes and the host fallback; scene B the stage-2 retry (prefix of 32, ran off, longer prefixes, second GetEdges on the updated
graph).  tests/test_track_frame_cases_cpu.py proves on the oracle's side that the scenes reach those branches.

Every comparison is library against oracle, at the bars of the dense-graph tests (tests/test_gpu_rgraph.py): statuses, lost list, dense
edge status rows exact; pose 1e-6 / 1e-5; positions 1e-4; max / min distance rows 2e-4; LM traces to the noise floor -- and library runs
that must build the same problem are equal to the bit."""
import numpy as np
import pytest

import nrs
import nrs_oracle as O
import rgraph_oracle as RG
import track_frame_cases as T
from conftest import compare_lm_traces

pytestmark = pytest.mark.gpu

BITS = ("pose_q", "pose_t", "f_pos", "f_status", "map_pos")


def _device_graph(ctx, sc, good):
    """the scene's graph with its history on the device; the UpdateVertex returns are the oracle's"""
    n = len(sc["tp"]["X_prev"])
    ids = np.arange(n, dtype=np.int32)
    g = nrs.RGraph(ctx, n, sc["sigma"], sc["stretch_th"])
    g.add_edges(sc["tp"]["X_prev"], ids, ids)
    for (pos, upd), ref in zip(sc["updates"], good):
        assert np.array_equal(g.update(pos, upd), ref)
    return g


def _solve_rg(ctx, sc, good, cap, probe=None):
    tp, fr = sc["tp"], sc["frame"]
    cam = nrs.make_camera(tp["model"], tp["prm"])
    g = _device_graph(ctx, sc, good)
    tr = nrs.Trace(1024)
    r = ctx.track_deform_solve_rg(cam, g, tp["X_prev"], fr["f_map"], fr["f_status"], fr["f_uv"], fr["f_pos"], tp["pose_q"], tp["pose_t"],
                                  tp["scale"], tr, cap)
    rows = g.rows(probe) if probe is not None else None
    g.close()
    return r, tr.trials, rows


def _held_to_the_oracle(r, trials, rows, o, otr, D_after, probe):
    assert np.allclose(r["pose_q"], o["pose_q"], atol=1e-6, rtol=0) and np.allclose(r["pose_t"], o["pose_t"], atol=1e-5, rtol=0)
    assert np.array_equal(r["f_status"], o["f_status"]) and r["lost"] == o["lost"] and len(o["lost"]) > 0
    assert np.allclose(r["f_pos"], o["f_pos"], atol=1e-4, rtol=0) and np.allclose(r["map_pos"], o["map_pos"], atol=1e-4, rtol=0)
    depth = compare_lm_traces(trials, otr, len(otr))
    print("LM trials compared with the oracle's:", depth)
    assert depth >= 6
    mx, mn, d0, st = rows
    assert np.array_equal(st, D_after.st[probe])                    # the graph after OPT:457-474, all N - 1 connections of a point
    ex = D_after.st[probe] != RG.NONE
    assert np.allclose(mx[ex], D_after.maxd[probe][ex], atol=2e-4, rtol=0) and np.allclose(mn[ex], D_after.mind[probe][ex], atol=2e-4, rtol=0)


def _same_bits(a, b):
    for k in BITS:
        assert np.array_equal(a[k], b[k]), k
    assert a["lost"] == b["lost"] and a["median"] == b["median"]


def _probe(sc, extra):
    """rows to compare: optimised points (frame order: not ascending), points outside the frame, the scene's special ones"""
    opt = T.optimised_ids(sc["frame"])
    n = len(sc["tp"]["X_prev"])
    return np.unique(np.concatenate([opt[:12], np.arange(0, n, n // 12), np.asarray(extra, np.int64)])).astype(np.int32)


def test_scene_a_sparse_permuted_frame_on_the_dense_graph(ctx):
    """prefixes of 16 (every long walk runs off; the prefixes grow 16 -> 64 -> 256 -> 1024) and whole lists: each held to the oracle, both
    equal to the bit; so are the host walk over the downloaded lists and the host fallback after two device passes"""
    sc, before, good, o, otr = T.dense_oracle_run("A")
    n = len(sc["tp"]["X_prev"])
    probe = _probe(sc, list(sc["special"]) + [sc["hole_pt"]])
    runs = []
    for cap in (16, n):
        r, trials, rows = _solve_rg(ctx, sc, good, cap, probe=probe)
        _held_to_the_oracle(r, trials, rows, o, otr, o["graph"], probe)
        runs.append((r, trials))
    _same_bits(runs[0][0], runs[1][0])
    key = [(t["lam"], t["chi"], t["chi_new"], t["accepted"]) for t in runs[0][1]]
    for switch in ("NRS_HOST_WALK", "1"), ("NRS_WALK_MAX_PASSES", "2"):
        nrs.debug_set(*switch)
        r, trials, _ = _solve_rg(ctx, sc, good, 64)
        nrs.debug_set(switch[0], None)
        _same_bits(r, runs[0][0])
        assert [(t["lam"], t["chi"], t["chi_new"], t["accepted"]) for t in trials] == key


def test_scene_a_embedded(ctx):
    """the same frame in embedded mode: f_node per frame slot (under the permutation not the per-map-id array), the `skip` bytes of
    GetEdges per map id, is_node per optimised point -- against oracle/embedded_oracle.py; device walk and host walk equal to the bit"""
    import copy
    import embedded_oracle as E
    sc, before, good, _, _ = T.dense_oracle_run("A")
    tp, fr = sc["tp"], sc["frame"]
    n = len(tp["X_prev"])
    cam = nrs.make_camera(tp["model"], tp["prm"])
    eligible = np.zeros(n, np.uint8)
    eligible[T.optimised_ids(fr)] = 1
    node = T.node_flags(fr, ctx.skin_select_nodes(tp["X_prev"], 40, eligible))
    D = copy.deepcopy(before)
    otr = []
    o = E.track_deform_solve_embedded(tp["model"], tp["prm"], D, tp["X_prev"], fr["f_map"], fr["f_status"], fr["f_uv"], fr["f_pos"], node,
                                      tp["pose_q"], tp["pose_t"], tp["scale"], otr)
    assert o["n_nodes"] == 40 and o["n_skinned"] > (len(T.optimised_ids(fr)) - 40) // 2 and len(o["lost"]) > 0
    probe = _probe(sc, list(sc["special"]))
    out = []
    for host in (False, True):
        nrs.debug_set("NRS_HOST_WALK", "1" if host else None)
        g = _device_graph(ctx, sc, good)
        tr = nrs.Trace(1024)
        r = ctx.track_deform_solve_embedded(cam, g, tp["X_prev"], fr["f_map"], fr["f_status"], fr["f_uv"], fr["f_pos"], node, tp["pose_q"], tp["pose_t"],
                                            tp["scale"], tr, 64)
        st = g.rows(probe)[3]
        g.close()
        out.append((r, tr.trials, st))
    nrs.debug_set("NRS_HOST_WALK", None)
    r, trials, st = out[0]
    assert np.allclose(r["pose_q"], o["pose_q"], atol=1e-6, rtol=0) and np.allclose(r["pose_t"], o["pose_t"], atol=1e-5, rtol=0)
    assert np.array_equal(r["f_status"], o["f_status"]) and r["lost"] == o["lost"]
    assert np.allclose(r["f_pos"], o["f_pos"], atol=1e-4, rtol=0) and np.allclose(r["map_pos"], o["map_pos"], atol=1e-4, rtol=0)
    assert abs(r["median"] - o["median"]) < 1e-5
    depth = compare_lm_traces(trials, otr, len(otr))
    print("LM trials compared with the oracle's:", depth)
    assert depth >= 6
    assert np.array_equal(st, D.st[probe])
    _same_bits(out[0][0], out[1][0])
    assert [(t["lam"], t["chi"], t["chi_new"], t["accepted"]) for t in out[0][1]] == [(t["lam"], t["chi"], t["chi_new"], t["accepted"]) for t in out[1][1]]
    assert np.array_equal(out[0][2], out[1][2])


@pytest.mark.parametrize("solver", ["direct", "pcg"])
def test_flat_graph_permuted_partial_frame(ctx_direct, ctx_pcg, solver):
    """nrs_track_deform_solve at the full bar of test_track_deform_matches_oracle (tests/test_gpu_track.py) on the frame both CPU
    restatements agree on"""
    tp, fr = T.flat_case()
    ctx = ctx_direct if solver == "direct" else ctx_pcg
    cam = nrs.make_camera(tp["model"], tp["prm"])
    tr = nrs.Trace(1024)
    r = ctx.track_deform_solve(cam, tp["graph"], tp["X_prev"], fr["f_map"], fr["f_status"], fr["f_uv"], fr["f_pos"], tp["pose_q"], tp["pose_t"],
                               tp["scale"], tr)
    otr = []
    o = O.track_deform_solve(tp["model"], tp["prm"], tp["graph"], tp["X_prev"], fr["f_map"], fr["f_status"], fr["f_uv"], fr["f_pos"], tp["pose_q"],
                             tp["pose_t"], tp["scale"], otr)
    assert all(t["inner"] == 1 for t in tr.trials) == (solver == "direct")
    assert np.allclose(r["pose_q"], o["pose_q"], atol=1e-6, rtol=0)
    assert np.allclose(r["pose_t"], o["pose_t"], atol=1e-5, rtol=0)
    assert np.array_equal(r["f_status"], o["f_status"])
    assert r["lost"] == o["lost"] and len(r["lost"]) > 0
    assert np.allclose(r["f_pos"], o["f_pos"], atol=1e-4, rtol=0)
    assert np.allclose(r["map_pos"], o["map_pos"], atol=1e-4, rtol=0)
    assert abs(r["median"] - o["median"]) < 1e-5
    assert np.array_equal(r["graph"]["e_status"], o["graph"]["e_status"])
    assert np.allclose(r["graph"]["e_w"], o["graph"]["e_w"], atol=1e-5)
    depth = compare_lm_traces(tr.trials, otr, 3)
    print("LM trials compared with the oracle's:", depth)
    assert depth >= 9


def test_scene_b_stage_2_retry(ctx):
    """whole lists in stage 1 (cap_per_point = n: no retry there), so that stage 2's own prefix of 32 is what cuts the lost point's list:
    held to the oracle; prefixes of 8 give the same bits"""
    sc, before, good, o, otr = T.dense_oracle_run("B")
    n = len(sc["tp"]["X_prev"])
    probe = _probe(sc, [sc["retry_pt"]] + list(sc["cluster"][:6]))
    r, trials, rows = _solve_rg(ctx, sc, good, n, probe=probe)
    _held_to_the_oracle(r, trials, rows, o, otr, o["graph"], probe)
    assert sc["retry_pt"] in r["lost"] and max(t["round"] for t in trials) == 2
    r8, trials8, _ = _solve_rg(ctx, sc, good, 8)
    _same_bits(r, r8)
    assert [(t["lam"], t["chi"], t["chi_new"], t["accepted"]) for t in trials] == [(t["lam"], t["chi"], t["chi_new"], t["accepted"]) for t in trials8]


def test_bad_frames_are_reported_and_the_context_stays_usable(ctx):
    sc, before, good, o, otr = T.dense_oracle_run("B")
    tp, fr = sc["tp"], sc["frame"]
    n = len(tp["X_prev"])
    cam = nrs.make_camera(tp["model"], tp["prm"])
    g = _device_graph(ctx, sc, good)
    args = (tp["pose_q"], tp["pose_t"], tp["scale"])
    far = fr["f_map"].copy()
    far[np.where(far >= 0)[0][5]] = n                                 # one entry >= n_points
    ones = np.ones(len(far), np.uint8)
    for call in (lambda: ctx.track_deform_solve_rg(cam, g, tp["X_prev"], far, fr["f_status"], fr["f_uv"], fr["f_pos"], *args, None, 64),
                 lambda: ctx.track_deform_solve_embedded(cam, g, tp["X_prev"], far, fr["f_status"], fr["f_uv"], fr["f_pos"], ones, *args, None, 64)):
        with pytest.raises(nrs.NrsError) as e:
            call()
        assert e.value.code == -1, e.value                          # NRS_ERR_INVALID
    node = (fr["f_status"] != O.TRACKED_WITH_3D).astype(np.uint8)   # nodes marked, but on no optimised point
    with pytest.raises(nrs.NrsError) as e:
        ctx.track_deform_solve_embedded(cam, g, tp["X_prev"], fr["f_map"], fr["f_status"], fr["f_uv"], fr["f_pos"], node, *args, None, 64)
    assert e.value.code == -1, e.value
    # nothing of the above touched the graph or the context: the scene's solve still gives the oracle's result
    tr = nrs.Trace(1024)
    r = ctx.track_deform_solve_rg(cam, g, tp["X_prev"], fr["f_map"], fr["f_status"], fr["f_uv"], fr["f_pos"], *args, tr, 64)
    g.close()
    assert np.array_equal(r["f_status"], o["f_status"]) and r["lost"] == o["lost"]
    assert np.allclose(r["pose_q"], o["pose_q"], atol=1e-6, rtol=0) and np.allclose(r["pose_t"], o["pose_t"], atol=1e-5, rtol=0)
    assert np.allclose(r["map_pos"], o["map_pos"], atol=1e-4, rtol=0)
