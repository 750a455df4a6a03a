"""GPU: nrs_dbscan_nd and nrs_flow_tracks_cluster (include/nrs.h "f6") against tests/flow_cluster_oracle.py on the cases of
tests/flow_cluster_cases.py (what each is made for is asserted on the CPU, tests/test_flow_cluster_cases_cpu.py).  Every comparison is
exact: labels and counts are integers, flows are fp32 bits.  Both neighbour forms -- the LDS tiles and, with NRS_DBND_NO_TILE, a wave per
point -- are held to the oracle, not merely to each other."""
import functools

import numpy as np
import pytest

import flow_cluster_cases as FC
import flow_cluster_oracle as FO
import init_cases as IC
import nrs
import nrs_frame_loop as FL
import nrs_synth as S
import stereo_init_oracle as SO

pytestmark = pytest.mark.gpu
F32 = np.float32
FORMS = ("tiles", "plain")


def _form(form):
    nrs.debug_set("NRS_DBND_NO_TILE", "1" if form == "plain" else None)


def _same_points(ctx, c):
    label, counts = ctx.dbscan_nd(*FC.for_device(c))
    assert np.array_equal(counts, c["counts"]), (c["name"], counts, c["counts"])
    assert np.array_equal(label, c["label"]), (c["name"], np.nonzero(label != c["label"])[0][:10])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dim", FC.EDGE_DIM)
def test_word_and_tile_edges(ctx, dim, form):
    _form(form)
    for n in FC.EDGE_N:
        _same_points(ctx, FC.edge_case(n, dim))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", FC.POINT_CASES)
def test_point_cases(ctx, name, form):
    _form(form)
    _same_points(ctx, FC.point_case(name))


@pytest.mark.parametrize("form", FORMS)
def test_order_sensitive_pairs_follow_the_sequential_sum(ctx, form):
    """the labels are the ascending sum's and not the pairwise sum's, pair by pair"""
    _form(form)
    c = FC.order_case()
    label, _ = ctx.dbscan_nd(*FC.for_device(c))
    for i, j, seq_in in c["pairs"]:
        assert (label[[i, j, j + 1]] >= 0).all() == seq_in and (c["label_tree"][[i, j, j + 1]] >= 0).all() != seq_in, (i, j)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("length,quantised", [(2, True), (31, True), (5, False)])
def test_flow_tracks(ctx, length, quantised, form):
    _form(form)
    c = FC.track_case(length, quantised)
    label, counts, flows = ctx.flow_tracks_cluster(c["tracks"])
    assert flows.shape == c["flows"].shape and np.array_equal(flows.view(np.int32), c["flows"].view(np.int32))       # fp32 bits
    assert np.array_equal(counts, c["counts"]) and np.array_equal(label, c["label"])
    label2, counts2, none = ctx.flow_tracks_cluster(c["tracks"], flows=False)                                        # flows_out is optional
    assert none is None and np.array_equal(label2, label) and np.array_equal(counts2, counts)
    label3, counts3 = ctx.dbscan_nd(flows, FO.flow_eps(flows.shape[1]), FO.MIN_POINTS)                               # the rule's eps and min_points
    assert np.array_equal(label3, label) and np.array_equal(counts3, counts)


@functools.lru_cache(maxsize=None)
def _three_d():
    """the stereo start's hand-made point sets with its oracle's result, once for both forms"""
    return [(c, SO.dbscan3d(c["xyz"], c["eps"], c["min_points"], True)) for c in S.make_cluster_cases() if len(c["xyz"])]


@pytest.mark.parametrize("form", FORMS)
def test_three_dimensions_are_dbscan3d_and_the_rows_carry_nothing_over(ctx, form):
    """dim = 3: the label is nrs_dbscan3d's raw label; nrs_dbscan3d, run behind a large call that used the same scratch rows, still gives
    its oracle's result"""
    _form(form)
    _same_points(ctx, FC.wide_case())
    for case, (o_raw, o_lab, o_counts) in _three_d():
        raw, lab, counts = ctx.dbscan3d(case["xyz"], case["eps"], case["min_points"], True)
        assert np.array_equal(raw, o_raw) and np.array_equal(lab, o_lab) and np.array_equal(counts, o_counts), case["name"]
        label, counts_nd = ctx.dbscan_nd(case["xyz"], case["eps"], case["min_points"])
        assert np.array_equal(label, raw) and counts_nd.tolist() == [counts[0], counts[1]], case["name"]
        if case["name"] == "blobs1024":                              # ... and a large call once more in between
            _same_points(ctx, FC.big60_case())


@pytest.mark.parametrize("form", FORMS)
def test_a_large_call_then_a_small_one_in_the_same_buffer(ctx, form):
    _form(form)
    for c in (FC.big60_case(), FC.tiny_case(), FC.big60_case(), FC.tiny_case()):
        _same_points(ctx, c)
    label, counts = ctx.dbscan_nd(np.zeros((0, 7), F32), 1.0, 3)                           # n = 0: (0, 0), nothing launched
    assert len(label) == 0 and counts.tolist() == [0, 0]
    label, counts, flows = ctx.flow_tracks_cluster(np.zeros((0, 4, 2), F32))
    assert len(label) == 0 and counts.tolist() == [0, 0] and flows.shape == (0, 6)


def test_refusals_leave_the_context_usable(ctx):
    c = FC.tiny_case()
    data = c["data"]
    big = nrs.DBSCAN_MAX_POINTS + 1
    refusals = [(dict(n=-1), "nrs_dbscan_nd: n = -1 (0 .. 16384)"), (dict(n=big), "nrs_dbscan_nd: n = 16385 (0 .. 16384)"),
                (dict(dim=0), "nrs_dbscan_nd: dim = 0 (1 .. 64)"), (dict(dim=65), "nrs_dbscan_nd: dim = 65 (1 .. 64)"),
                (dict(eps=0.0), "eps = 0 is not a positive finite number"), (dict(eps=-1.0), "eps = -1 is not"),
                (dict(eps=float("inf")), "eps = inf is not"), (dict(eps=float("nan")), "is not a positive finite number"),
                (dict(min_points=0), "nrs_dbscan_nd: min_points = 0 (at least 1)")]
    for kw, text in refusals:
        args = dict(eps=c["eps"], min_points=c["min_points"])
        args.update(kw)
        with pytest.raises(nrs.NrsError) as ei:
            ctx.dbscan_nd(data, **args)
        assert ei.value.code == -1 and text in str(ei.value), (kw, str(ei.value))
        _same_points(ctx, c)                                         # the context still works
    tr = FC.track_case(2)["tracks"]
    for kw, text in [(dict(n=-1), "nrs_flow_tracks_cluster: n = -1 (0 .. 16384)"), (dict(n=big), "nrs_flow_tracks_cluster: n = 16385"),
                     (dict(length=1), "nrs_flow_tracks_cluster: length = 1 keypoints (2 .. 33)"), (dict(length=34), "length = 34 keypoints (2 .. 33)")]:
        with pytest.raises(nrs.NrsError) as ei:
            ctx.flow_tracks_cluster(tr, **kw)
        assert ei.value.code == -1 and text in str(ei.value), (kw, str(ei.value))
        _same_points(ctx, c)
    # null pointers, straight through the C ABI
    lab, counts = np.zeros(5, np.int32), np.zeros(2, np.int32)
    p = lambda a: a.ctypes.data
    lib = ctx.lib
    for call in (lambda: lib.nrs_dbscan_nd(ctx.h, 5, 2, None, 0.5, 3, p(lab), p(counts)), lambda: lib.nrs_dbscan_nd(ctx.h, 5, 2, p(data), 0.5, 3, None, p(counts)),
                 lambda: lib.nrs_dbscan_nd(ctx.h, 5, 2, p(data), 0.5, 3, p(lab), None), lambda: lib.nrs_dbscan_nd(ctx.h, 0, 2, None, 0.5, 3, None, None),
                 lambda: lib.nrs_flow_tracks_cluster(ctx.h, 5, 2, None, None, p(lab), p(counts)),
                 lambda: lib.nrs_flow_tracks_cluster(ctx.h, 5, 2, p(tr), None, None, p(counts)),
                 lambda: lib.nrs_flow_tracks_cluster(ctx.h, 5, 2, p(tr), None, p(lab), None)):
        assert call() == -1 and b"null pointer" in lib.nrs_last_error(ctx.h)
        _same_points(ctx, c)
    assert lib.nrs_dbscan_nd(None, 5, 2, p(data), 0.5, 3, p(lab), p(counts)) == -1 and lib.nrs_flow_tracks_cluster(None, 5, 2, p(tr), None, p(lab), p(counts)) == -1


def _start(cluster_tracks, sq):
    gb = FL.GpuBackend(nrs, sq["model"], sq["prm"], IC.LOOP_KLT)
    try:
        mo = FL.MonoInitializer(gb, max_images=30, max_features=400, radians_per_pixel=F32(sq["radians_per_pixel"]), cluster_tracks=cluster_tracks)
        for f in range(6):                                           # (the sequence starts within five images: tests/test_gpu_init_loop.py)
            r = mo.process_new_image(sq["images"][f], sq["mask"])
            if r is not None:
                return mo, r
        raise AssertionError("the synthetic sequence did not start")
    finally:
        gb.close()


def test_mono_initializer_clusters_its_tracks_on_the_device():
    """MonoInitializer(cluster_tracks=True) on the synthetic sequence of the f6 loop test, up to its start: the labels of every image are the
    oracle's on the tracks the log holds, and the solve sees exactly what it sees without the clustering"""
    sq = IC.init_sequence()
    mo, r = _start(True, sq)
    plain, r0 = _start(False, sq)
    assert len(mo.log) == len(plain.log) >= 3 and [e["reset"] for e in mo.log] == [True] + [False] * (len(mo.log) - 1)
    for f, (e, e0) in enumerate(zip(mo.log, plain.log)):
        assert set(e) - set(e0) <= {"full_tracks", "feature_labels"}
        for k, v in e0.items():
            assert np.array_equal(v, e[k]), (f, k)                   # reset, counts, verdict, ref_xy, cur_xy, status: the init_essential entries
        if f == 0:
            continue
        full = e["full_tracks"]
        assert len(full) >= 100 and np.all(np.diff(full) > 0) and np.all(e["status"][full] == FL.TRACKED)
        tracks = np.stack([mo.log[1]["ref_xy"][full]] + [mo.log[g]["cur_xy"][full] for g in range(1, f + 1)], 1)
        assert tracks.shape == (len(full), f + 1, 2)
        label, counts, _ = FO.flow_tracks_cluster(tracks)
        assert np.array_equal(e["feature_labels"], label), f
    for k, v in r0.items():
        assert np.array_equal(v, r[k]), k
    last = mo.log[-1]
    assert np.array_equal(r["track_labels"], last["feature_labels"][np.searchsorted(last["full_tracks"], r["index"])])
    assert len(r["track_labels"]) == len(r["index"]) >= 100
