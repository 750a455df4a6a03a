"""GPU: the resident TemporalBuffer (include/nrs.h nrs_tbuf_*, nrs_map_frame_tbuf) against the host path of the same build -- the
Python TemporalBuffer of nrs_frame_loop flattened, and nrs_map_frame on that flat buffer on the same context.  Both paths run the same
mapping kernels on the same tables, so everything is compared as bit patterns; tests/test_tbuf_cases_cpu.py vets the replayed cases.

What the ring holds after each insert: the reference pops when size() > 20 BEFORE it inserts, so the sizes after the 23 inserts of the ring
test are 1 .. 21, 21, 21 (21 -> 20 -> 21 inside a call); they are asserted equal to nrs_frame_loop.TemporalBuffer's."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import map_cases as MC
import nrs
import nrs_frame_loop as FL
import tbuf_cases as TC

pytestmark = pytest.mark.gpu
F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _fill(tb, snaps, flags=True):
    for s in snaps:
        tb.insert(s["ids"], s["xy"], s["pos"], s["status"], s["pose"], s["mag"], has_lm=s.get("has_lm") if flags else None)


def _same_flat(tb, snaps, max_buffer_size=20):
    """nrs_tbuf_info / nrs_tbuf_flat against the host buffer fed the same frames"""
    want, wmag, wids = TC.host_flat(snaps, max_buffer_size)
    got, gmag, gids = tb.flat()
    last = snaps[-1]
    keep = (last["status"] == 0) | (last["status"] == 1)
    assert tb.info() == (want["n_frames"], len(wids), int((last["status"][keep] == 1).sum()))
    assert np.array_equal(gids, wids)
    assert np.array_equal(got["has_kp"], want["has_kp"]) and np.array_equal(got["has_lm"], want["has_lm"])
    assert np.array_equal(got["status"], want["status"])
    assert np.array_equal(_bits(got["kp_xy"]), _bits(want["kp_xy"])) and np.array_equal(_bits(got["lm_xyz"]), _bits(want["lm_xyz"]))
    assert np.array_equal(_bits(got["poses"]).reshape(-1), _bits(want["poses"]).reshape(-1)) and np.array_equal(_bits(gmag), _bits(wmag))
    return want, wmag, wids


def _same_result(r, ref, ids):
    """r: nrs_map_frame_tbuf (keypoint ids); ref: nrs_map_frame on a flat buffer whose row j is the id ids[j]"""
    ids = np.asarray(ids, np.int64)
    assert np.array_equal(r["cand"], ids[ref["cand"]])
    assert np.array_equal(r["rigid_status"], ref["rigid_status"]) and np.array_equal(r["deform_status"], ref["deform_status"])
    assert (r["n_rigid"], r["n_deformable"], r["mode"]) == (ref["n_rigid"], ref["n_deformable"], ref["mode"])
    assert np.array_equal(r["accepted_ids"], ids[ref["accepted_ids"]])
    for k in ("rigid_xyz", "deform_xyz", "accepted_xyz"):
        assert np.array_equal(_bits(r[k]), _bits(ref[k])), k


@functools.lru_cache(maxsize=None)
def _flat_reference(ctx, name):
    """nrs_map_frame on the flat case: computed once per case, shared by the three relabellings (read only)"""
    cs = MC.case(name)
    tb = cs["tb"]
    return ctx.map_frame(nrs.make_camera(tb["model"], tb["prm"]), tb, cs["deform_mag"], cs["rad_per_pixel"], rigidity_th=0.004, min_track=5,
                         index_snapshot=cs["index_snapshot"])


# ------------------------------------------------------------------------------------------------ 1. replay
@pytest.mark.parametrize("relabel", TC.RELABELS)
@pytest.mark.parametrize("name", MC.CASES)
def test_replay_gives_the_bits_of_the_flat_call(ctx, name, relabel):
    cs = MC.case(name)
    ids, snaps = TC.snapshots_of(cs, relabel)
    ref = _flat_reference(ctx, name)
    tb = nrs.TBuf(ctx, 20)
    try:
        _fill(tb, snaps)
        _same_flat(tb, snaps)
        r = tb.map_frame(nrs.make_camera(cs["tb"]["model"], cs["tb"]["prm"]), cs["rad_per_pixel"], 0.004, 5, cs["index_snapshot"])
    finally:
        tb.close()
    _same_result(r, ref, ids)
    if name == "nan":
        k = list(ref["cand"]).index(cs["tb"]["touched"])
        assert r["cand"][k] == ids[cs["tb"]["touched"]] and np.isnan(r["rigid_xyz"][k]).all() and r["cand"][k] not in r["accepted_ids"]
    if name == "count_0":
        assert len(r["cand"]) == 0 and r["mode"] == 2


# ------------------------------------------------------------------------------------------------ 2. the ring
def _ring_frame(t, n=70, step=9):
    """70 slots over a sliding id window (ids enter and leave), statuses 0 .. 5, a rotated order"""
    rng = np.random.default_rng(40 + t)
    k = rng.permutation(n)
    return dict(ids=(step * t + k).astype(np.int64), xy=rng.uniform(0, 600, (n, 2)).astype(F32), pos=rng.normal(0, 1, (n, 3)).astype(F32),
                status=((k + t) % 6).astype(np.int32), pose=np.concatenate([[0, 0, 0, 1], rng.normal(0, 1, 3)]).astype(F32), mag=F32(0.001 * t))


def test_ring_follows_the_host_buffer(ctx):
    tb = nrs.TBuf(ctx, 20)
    host = FL.TemporalBuffer(20)
    snaps, sizes = [], []
    try:
        for t in range(23):
            s = _ring_frame(t)
            snaps.append(s)
            host.insert(s["ids"], s["xy"], s["pos"], s["status"], s["pose"][:4], s["pose"][4:], s["mag"])
            tb.insert(s["ids"], s["xy"], s["pos"], s["status"], s["pose"], s["mag"])
            _same_flat(tb, snaps)
            sizes.append(tb.info()[0])
            assert sizes[-1] == len(host.snaps)
    finally:
        tb.close()
    assert sizes == list(range(1, 22)) + [21, 21]


# ------------------------------------------------------------------------------------------------ 3. row edges
def _edge_snaps(count):
    """distinct-id counts at the edges of the row scan: `count` ids over a span of 3 count + 1 with both ends of the span used; snapshot 0
    holds every other id, snapshot 1 keeps nothing, snapshot 2 (the last) holds all of them, TRACKED and TRACKED_WITH_3D alternating"""
    rng = np.random.default_rng(count)
    lo, span = 777, (3 * count + 1 if count > 1 else 1)
    inner = rng.choice(np.arange(1, span - 1), max(0, count - 2), replace=False) if count > 2 else np.zeros(0, np.int64)
    ids = lo + np.sort(np.concatenate([[0], inner, [span - 1]] if count > 1 else [[0]]).astype(np.int64))
    assert len(ids) == count and ids[-1] - ids[0] + 1 == span
    xy0 = np.stack([40 + 31.0 * (np.arange(count) % 19), 40 + 31.0 * (np.arange(count) // 19 % 15)], 1)

    def snap(f, sel, status):
        p = np.random.default_rng(count + f).permutation(len(sel))
        return dict(ids=ids[sel][p], xy=(xy0[sel][p] + 0.4 * f).astype(F32), pos=rng.normal(0, 1, (len(sel), 3)).astype(F32)[p] + F32([0, 0, 3]),
                    status=np.asarray(status, np.int32)[p], pose=np.array([0, 0, 0, 1, -0.003 * f, 0, 0], F32), mag=F32(0.001))
    every = np.arange(count)
    return ids, [snap(0, every[::2], np.zeros(len(every[::2]))), snap(1, every, np.full(count, 4)), snap(2, every, every % 2 if count > 1 else [1])]


@pytest.mark.parametrize("count", [1, 63, 64, 65, 1024, 1025, 2049])
def test_row_edges(ctx, count):
    ids, snaps = _edge_snaps(count)
    cam = nrs.make_camera(0, np.array([700, 700, 320, 240, 0, 0, 0, 0], F32))
    rpp = 1.0 / 700
    tb = nrs.TBuf(ctx, 20)
    try:
        _fill(tb, snaps, flags=False)
        want, wmag, wids = _same_flat(tb, snaps)
        assert np.array_equal(wids, ids) and tb.info() == (3, count, max(1, count // 2) if count > 1 else 1)
        assert not want["has_kp"][1].any()                         # the empty snapshot in the middle
        r = tb.map_frame(cam, rpp)
        ref = ctx.map_frame(cam, want, wmag, rpp)
        assert len(r["cand"]) == tb.info()[2]
        _same_result(r, ref, wids)
        # an empty snapshot as the last one: no candidates, 0 / 0 votes deformable, nothing to launch
        empty = dict(snaps[1], mag=F32(0.002))
        tb.insert(empty["ids"], empty["xy"], empty["pos"], empty["status"], empty["pose"], empty["mag"])
        _same_flat(tb, snaps + [empty])
        assert tb.info() == (4, count, 0)
        r = tb.map_frame(cam, rpp)
        assert len(r["cand"]) == 0 and len(r["accepted_ids"]) == 0 and (r["n_rigid"], r["n_deformable"], r["mode"]) == (0, 0, 2)
    finally:
        tb.close()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_buffer_and_the_context_usable(ctx):
    cs = MC.case("rigid_f4")
    ids, snaps = TC.snapshots_of(cs, "identity")
    cam = nrs.make_camera(cs["tb"]["model"], cs["tb"]["prm"])
    ref = _flat_reference(ctx, "rigid_f4")
    tb = nrs.TBuf(ctx, 20)
    other, ctx2 = nrs.TBuf(ctx, 20), nrs.Context()
    try:
        _fill(tb, snaps)
        before = tb.flat()
        s = snaps[-1]
        keep = np.nonzero((s["status"] == 0) | (s["status"] == 1))[0]

        def insert(**kw):
            a = dict(s, **kw)
            tb.insert(a["ids"], a["xy"], a["pos"], a["status"], a["pose"], a["mag"], has_lm=a["has_lm"])

        def refused(code, text, fn, on=ctx):
            with pytest.raises(nrs.NrsError, match=text) as e:
                fn()
            assert e.value.code == code
            assert re.search(text, on.lib.nrs_last_error(on.h).decode())

        dup = s["ids"].copy()
        dup[keep[5]] = dup[keep[2]]
        refused(-1, "duplicate keypoint id %d among the kept entries" % dup[keep[2]], lambda: insert(ids=dup))
        neg = s["ids"].copy()
        neg[keep[1]] = -3
        refused(-1, "negative keypoint id -3", lambda: insert(ids=neg))
        far = s["ids"].copy()
        far[keep[0]] = (1 << 22) + 5
        refused(-1, "more than the limit of 4194304 ids", lambda: insert(ids=far))
        pose = np.ascontiguousarray(s["pose"], F32)
        refused(-1, "null array with n = 5", lambda: ctx._chk(ctx.lib.nrs_tbuf_insert(tb.h, 5, None, None, None, None, None, nrs._p(pose, C.c_float), 0.0)))
        refused(-1, r"index_snapshot 4 outside \[-1, 4\)", lambda: tb.map_frame(cam, cs["rad_per_pixel"], index_snapshot=4))
        refused(-1, "index_snapshot -2 outside", lambda: tb.map_frame(cam, cs["rad_per_pixel"], index_snapshot=-2))
        refused(-1, "must be finite", lambda: tb.map_frame(cam, float("nan")))
        refused(-5, "holds no snapshot", lambda: other.map_frame(cam, cs["rad_per_pixel"]))
        refused(-1, "belongs to another context", lambda: tb.map_frame(cam, cs["rad_per_pixel"], ctx=ctx2), on=ctx2)
        with pytest.raises(nrs.NrsError) as e:
            nrs.TBuf(ctx, 21)
        assert e.value.code == -1
        # nothing moved: the same dense form, and the mapping call gives the flat call's bits
        after = tb.flat()
        assert tb.info()[0] == len(snaps) and np.array_equal(after[2], before[2]) and np.array_equal(_bits(after[1]), _bits(before[1]))
        for k in ("has_kp", "has_lm", "status"):
            assert np.array_equal(after[0][k], before[0][k])
        for k in ("kp_xy", "lm_xyz", "poses"):
            assert np.array_equal(_bits(after[0][k]), _bits(before[0][k]))
        _same_flat(tb, snaps)
        _same_result(tb.map_frame(cam, cs["rad_per_pixel"]), ref, ids)
        # a duplicate id among DROPPED entries is not looked at: the frame enters
        st = s["status"].copy()
        st[keep[5]] = 4
        insert(ids=dup, status=st)
        _same_flat(tb, snaps + [dict(s, ids=dup, status=st)])
        # ... and the other context is usable too
        assert ctx2.map_frame(cam, cs["tb"], cs["deform_mag"], cs["rad_per_pixel"])["mode"] == ref["mode"]
    finally:
        tb.close()
        other.close()
        ctx2.close()


# ------------------------------------------------------------------------------------------------ 5. reuse
def test_clear_then_a_smaller_sequence_shows_no_stale_rows(ctx):
    nrs.debug_set("NRS_POISON", "1")                               # fresh device buffers are filled with 0xFF: a read of an unwritten word shows
    big, small = MC.case("count_1025"), MC.case("rigid_f4")
    tb = nrs.TBuf(ctx, 20)
    try:
        ids_b, snaps_b = TC.snapshots_of(big, "offset_gaps")
        _fill(tb, snaps_b)
        _same_flat(tb, snaps_b)
        cam_b = nrs.make_camera(big["tb"]["model"], big["tb"]["prm"])
        _same_result(tb.map_frame(cam_b, big["rad_per_pixel"]), _flat_reference(ctx, "count_1025"), ids_b)
        tb.clear()
        assert tb.info() == (0, 0, 0)
        with pytest.raises(nrs.NrsError) as e:
            tb.map_frame(cam_b, big["rad_per_pixel"])
        assert e.value.code == -5
        ids_s, snaps_s = TC.snapshots_of(small, "reversed")
        _fill(tb, snaps_s)
        _same_flat(tb, snaps_s)
        cam_s = nrs.make_camera(small["tb"]["model"], small["tb"]["prm"])
        _same_result(tb.map_frame(cam_s, small["rad_per_pixel"]), _flat_reference(ctx, "rigid_f4"), ids_s)
    finally:
        tb.close()
