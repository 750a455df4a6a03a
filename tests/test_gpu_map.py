"""GPU parity: frame mapping (include/nrs.h nrs_map_frame, nrs_rgraph_resize, nrs_map_grow_graph) against tests/map_oracle.py on the
cases tests/test_map_oracle_cpu.py vets (tests/map_cases.py: no gate of theirs hangs on the last bit, so statuses must be identical).

Compared: rigid / deformable statuses, the counts, the mode and the accepted ids identical; rigid positions EXACTLY (the fp32 twins of
oracle/triang_oracle.py); deformable positions within the tolerances of tests/test_gpu_triang.py (2e-3 maximum, 1e-4 median: the LM
runs on g2o's numeric Jacobian); nrs_triangulate_batch on the same buffer equal to the call's deformable leg bit for bit."""
import numpy as np
import pytest

import map_cases as MC
import map_oracle as M
import nrs
import rgraph_oracle as RG
import track_frame_cases as TFC

pytestmark = pytest.mark.gpu


def _run(ctx, cs, **kw):
    tb = cs["tb"]
    cam = nrs.make_camera(tb["model"], tb["prm"])
    args = dict(rigidity_th=0.004, min_track=5, index_snapshot=cs["index_snapshot"])
    args.update(kw)
    return cam, ctx.map_frame(cam, tb, cs["deform_mag"], cs["rad_per_pixel"], **args)


def _same_float_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _held_to_the_oracle(r, ref, nan_bits=False):
    assert np.array_equal(r["cand"], ref["cand"])
    assert np.array_equal(r["rigid_status"], ref["rigid_status"]), (np.bincount(r["rigid_status"]), np.bincount(ref["rigid_status"]))
    assert np.array_equal(r["deform_status"], ref["deform_status"]), (np.bincount(r["deform_status"]), np.bincount(ref["deform_status"]))
    assert (r["n_rigid"], r["n_deformable"], r["mode"]) == (ref["n_rigid"], ref["n_deformable"], ref["mode"])
    assert np.array_equal(r["accepted_ids"], ref["accepted_ids"])
    worst = np.nanmax(np.abs(r["rigid_xyz"] - ref["rigid_xyz"])) if len(ref["cand"]) else 0.0
    print("rigid xyz: largest disagreement", worst)
    assert np.array_equal(np.isnan(r["rigid_xyz"]), np.isnan(ref["rigid_xyz"]))
    assert np.array_equal(np.nan_to_num(r["rigid_xyz"]), np.nan_to_num(ref["rigid_xyz"]))          # exact
    ok = ref["deform_status"] == 0
    if ok.any():
        err = np.linalg.norm(r["deform_xyz"][ok] - ref["deform_xyz"][ok], axis=1)
        print("deformable xyz: max", err.max(), "median", np.median(err))
        assert err.max() <= 2e-3 and np.median(err) <= 1e-4
    assert np.all(r["deform_xyz"][~ok] == 0)
    # the accepted positions are the voted leg's, in candidate order
    leg = r["rigid_xyz"] if r["mode"] == M.MODE_RIGID else r["deform_xyz"]
    idx = np.searchsorted(r["cand"], r["accepted_ids"])
    assert _same_float_bits(r["accepted_xyz"], leg[idx])


@pytest.mark.parametrize("name", MC.CASES)
def test_map_frame_matches_the_restatement(ctx, name):
    cs = MC.case(name)
    cam, r = _run(ctx, cs)
    _held_to_the_oracle(r, cs["ref"])
    # one path: nrs_triangulate_batch on the same buffer and the device-built candidate list gives the deformable leg's bits
    if len(r["cand"]):
        st, xyz = ctx.triangulate_batch(cam, cs["tb"], r["cand"], 5)
        nan = r["deform_status"] == M.D_NAN
        assert np.array_equal(st[~nan], r["deform_status"][~nan]) and np.all(st[nan] == 0)
        assert _same_float_bits(xyz[~nan], r["deform_xyz"][~nan])
    if name == "nan":
        k = list(r["cand"]).index(cs["tb"]["touched"])
        assert r["rigid_status"][k] == 0 and np.isnan(r["rigid_xyz"][k]).all() and cs["tb"]["touched"] not in r["accepted_ids"]


def test_bad_arguments_leave_the_context_usable(ctx):
    cs = MC.case("rigid_f4")
    tb = cs["tb"]
    cam = nrs.make_camera(tb["model"], tb["prm"])
    mag, rpp = cs["deform_mag"], cs["rad_per_pixel"]
    with pytest.raises(nrs.NrsError):
        ctx.map_frame(cam, tb, mag, float("nan"))
    with pytest.raises(nrs.NrsError):
        ctx.map_frame(cam, tb, mag, rpp, rigidity_th=float("inf"))
    with pytest.raises(nrs.NrsError):
        ctx.map_frame(cam, tb, mag, rpp, index_snapshot=tb["n_frames"])
    with pytest.raises(nrs.NrsError):
        ctx.map_frame(cam, tb, mag, rpp, index_snapshot=-2)
    with pytest.raises(nrs.NrsError):
        ctx.map_frame(nrs.make_camera(7, tb["prm"]), tb, mag, rpp)
    gone = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in tb.items()}
    c = int(np.nonzero(tb["status"] == 1)[0][0])
    gone["has_kp"][-1, c] = False                                  # a TRACKED id without a keypoint in the last snapshot
    with pytest.raises(nrs.NrsError, match="no keypoint in the last snapshot"):
        ctx.map_frame(cam, gone, mag, rpp)
    long = dict(tb, n_frames=22)                                   # 22 snapshots: the oldest one repeated in front
    for k in ("poses", "has_kp", "kp_xy", "has_lm", "lm_xyz"):
        long[k] = np.concatenate([tb[k][:1]] * 18 + [tb[k]])
    with pytest.raises(nrs.NrsError, match="at most 21"):
        ctx.map_frame(cam, long, np.zeros(22, np.float32), rpp)
    _held_to_the_oracle(_run(ctx, cs)[1], cs["ref"])


# ------------------------------------------------------------------------------------------------ the graph that grows
def _same_rows(g, D, ids):
    mx, mn, d0, st = g.rows(np.asarray(ids, np.int32))
    c = st.shape[1]                                                # the device graph's capacity (D may be larger: it has no edge out there)
    assert np.array_equal(st, D.st[ids][:, :c]) and np.all(D.st[ids][:, c:] == RG.NONE)
    ex = D.st[ids][:, :c] != RG.NONE
    for a, b in ((mx, D.maxd), (mn, D.mind), (d0, D.d0)):
        assert _same_float_bits(a[ex], b[ids][:, :c][ex])
    return st


def test_resize_between_add_edges_and_update(ctx):
    rng = np.random.default_rng(5)
    X = rng.normal(0, 1, (40, 3)).astype(np.float32)
    sigma, th = 1.2, 1.1
    g = nrs.RGraph(ctx, 8, sigma, th)
    fresh = nrs.RGraph(ctx, 40, sigma, th)                         # the larger capacity from the start, the same call sequence
    D = RG.DenseGraph(40, sigma, th)
    cap = 8

    def both(fn):
        fn(g, cap)
        fn(fresh, 40)

    ids8 = np.arange(8, dtype=np.int32)
    both(lambda G, c: G.add_edges(X[:c], ids8, ids8))
    D.add_edges(X, ids8, ids8)
    X2 = (X * np.float32(1.7)).astype(np.float32)
    up = np.array([1, 4, 6], np.int32)
    good = [g.update(X2[:8], up), fresh.update(X2, up), np.array([D.update_vertex(X2, int(i)) for i in up])]
    assert np.array_equal(good[0], good[1]) and np.array_equal(good[0], good[2])
    for new_cap, lo in ((13, 8), (40, 13)):
        g.resize(new_cap)
        cap = new_cap
        old = np.arange(lo, dtype=np.int32)
        st = _same_rows(g, D, old)                                 # old ids: as before; the new columns and rows: no edge
        assert np.all(st[:, lo:] == RG.NONE) and np.all(g.rows(np.arange(lo, new_cap, dtype=np.int32))[3] == RG.NONE)
        new = np.arange(lo, new_cap, dtype=np.int32)
        allp = np.arange(new_cap, dtype=np.int32)
        g.grow(X[:new_cap], new, allp)
        fresh.grow(X, new, allp)
        D.add_edges(X, new, allp)
        up = np.array([0, lo - 1, lo, new_cap - 1], np.int32)
        gd = [g.update(X2[:new_cap], up), fresh.update(X2, up), np.array([D.update_vertex(X2, int(i)) for i in up])]
        assert np.array_equal(gd[0], gd[1]) and np.array_equal(gd[0], gd[2])
        _same_rows(g, D, allp)
        a, b = g.get_edges(allp, 16), fresh.get_edges(allp, 16)
        assert np.array_equal(a[0], b[0])
        for k in range(len(allp)):
            m = min(int(a[0][k]), 16)
            assert np.array_equal(a[1][k, :m], b[1][k, :m]) and _same_float_bits(a[2][k, :m], b[2][k, :m]) and np.array_equal(a[4][k, :m], b[4][k, :m])
        assert g.edge(0, new_cap - 1) == fresh.edge(0, new_cap - 1) and g.edge(2, 5) == fresh.edge(2, 5)
    # failures leave the graph intact
    with pytest.raises(nrs.NrsError, match="nrs_rgraph_resize: capacity 12 is below"):
        g.resize(12)
    assert g.cap == 40
    _same_rows(g, D, np.arange(40))
    with pytest.raises(nrs.NrsError, match="nrs_rgraph_resize: capacity 200001 .*limit"):
        g.resize(200001)
    assert g.cap == 40
    _same_rows(g, D, np.arange(40))
    g.close()
    fresh.close()


def test_grow_graph_is_add_edge(ctx):
    """two new points against five others + themselves: RegularizationGraph::AddEdge one pair at a time (oracle/rgraph_oracle.py
    LiteralGraph), the new-new pair added from both sides"""
    rng = np.random.default_rng(9)
    X = rng.normal(0, 1, (7, 3)).astype(np.float32)
    sigma, th = 1.0, 1.1
    g = nrs.RGraph(ctx, 5, sigma, th)
    L = RG.LiteralGraph(sigma, th)
    old = np.arange(5, dtype=np.int32)
    g.add_edges(X[:5], old, old)
    for i in old:
        for j in old:
            if i != j:
                L.add_edge(int(i), int(j), X[j] - X[i])
    X2 = X.copy()
    X2[:5] *= np.float32(1.3)                                      # some history on the old edges, so that a rewrite would show
    assert np.array_equal(g.update(X2[:5], old), [L.update_vertex(X2, int(i)) for i in old])
    g.resize(7)
    new, others = np.array([5, 6], np.int32), np.arange(7, dtype=np.int32)   # current_mappoints_ids: TRACKED_WITH_3D + JUST_TRIANGULATED
    g.grow(X2, new, others)
    calls = []
    for i in new:                                                  # mapping.cc:240-256
        for j in others:
            if i != j:
                L.add_edge(int(i), int(j), X2[j] - X2[i])
                calls.append((int(i), int(j)))
    assert (5, 6) in calls and (6, 5) in calls
    for i in range(7):
        for j in range(7):
            if i != j:
                e, d = L.g[i][j], g.edge(i, j)
                assert d["status"] == e["st"] and _same_float_bits([d["d0"], d["max"], d["min"], d["w"]], [e["d0"], e["mx"], e["mn"], e["w"]]), (i, j)
    g.close()


def test_track_deform_on_a_resized_grown_graph(ctx):
    """scene B of tests/track_frame_cases.py with its graph built at 200 points, resized to 260 and grown: a2 agrees with the oracle as on
    the graph built at once (the comparisons of tests/test_gpu_track_frames.py)"""
    sc, before, good, o, otr = TFC.dense_oracle_run("B")
    tp, fr = sc["tp"], sc["frame"]
    X = tp["X_prev"]
    n, n0 = len(X), 200
    g = nrs.RGraph(ctx, n0, sc["sigma"], sc["stretch_th"])
    ids0 = np.arange(n0, dtype=np.int32)
    g.add_edges(X[:n0], ids0, ids0)
    g.resize(n)
    g.grow(X, np.arange(n0, n, dtype=np.int32), np.arange(n, dtype=np.int32))
    for (pos, upd), ref in zip(sc["updates"], good):
        assert np.array_equal(g.update(pos, upd), ref)
    cam = nrs.make_camera(tp["model"], tp["prm"])
    tr = nrs.Trace(1024)
    r = ctx.track_deform_solve_rg(cam, g, X, fr["f_map"], fr["f_status"], fr["f_uv"], fr["f_pos"], tp["pose_q"], tp["pose_t"], tp["scale"], tr, n)
    probe = np.array([sc["retry_pt"], 0, n0 - 1, n0, n - 1], np.int32)
    mx, mn, d0, st = g.rows(probe)
    g.close()
    assert np.allclose(r["pose_q"], o["pose_q"], atol=1e-6, rtol=0) and np.allclose(r["pose_t"], o["pose_t"], atol=1e-5, rtol=0)
    assert np.array_equal(r["f_status"], o["f_status"]) and r["lost"] == o["lost"]
    assert np.allclose(r["f_pos"], o["f_pos"], atol=1e-4, rtol=0) and np.allclose(r["map_pos"], o["map_pos"], atol=1e-4, rtol=0)
    D_after = o["graph"]
    assert np.array_equal(st, D_after.st[probe])
    ex = D_after.st[probe] != RG.NONE
    assert np.allclose(mx[ex], D_after.maxd[probe][ex], atol=2e-4, rtol=0) and np.allclose(mn[ex], D_after.mind[probe][ex], atol=2e-4, rtol=0)
