"""GPU parity: a21-a23 LucasKanadeTracker (reference modules/matching/lucas_kanade_tracker.cc) through
the C ABI against the oracle (oracle/lk_oracle.py), given this build's own restatement of the
OpenCV pyramid (parity unpinned at the pyramid boundary).

Bars: templates (int16 windows), status codes and n_good: exact; means and tracked positions:
exact as well (same fixed-point sampling, same sequential float32 sums, no FMA contraction) -- the
tests allow 1e-3 px / 1e-6 relative as the stated tolerance but assert bit-equality where it holds."""
import numpy as np
import pytest

import lk_oracle as LK
import nrs
import nrs_synth as S

pytestmark = pytest.mark.gpu


def _setup(ctx, n, seed, **kw):
    sq = S.make_lk_sequence(n, seed, **kw)
    ctx.klt_configure()
    ctx.klt_set_reference(sq["im0"], sq["pts"])
    lk = LK.LucasKanadeOracle()
    lk.set_reference(sq["im0"], sq["pts"])
    return sq, lk


def test_templates_match_oracle(ctx):
    sq, lk = _setup(ctx, 60, 3)
    assert ctx.klt_num_points() == len(sq["pts"])
    for i, t in enumerate(ctx.klt_get_templates(0, len(sq["pts"]))):              # every point (one device read)
        for level in range(5):
            assert bool(t["valid"][level]) == (lk.Iref[level][i] is not None)
            if lk.Iref[level][i] is not None:
                assert np.array_equal(t["gray"][level], lk.Iref[level][i])           # pyramid + sampling: bit-exact
                assert np.array_equal(t["grad"][level], lk.Idref[level][i])
                assert t["mean"][level, 0] == lk.meanI[level][i] and t["mean"][level, 1] == lk.meanI2[level][i]
            else:
                assert t["mean"][level, 0] == -1 and t["mean"][level, 1] == -1


@pytest.mark.parametrize("n,seed,flow", [(80, 5, 6.0), (150, 6, 3.0), (150, 7, 12.0)])
def test_track_matches_oracle(ctx, n, seed, flow):
    sq, lk = _setup(ctx, n, seed, flow_px=flow)
    st = np.zeros(len(sq["pts"]), np.int32)
    st[::17] = 3                                        # BAD points are skipped and left untouched
    guess = sq["pts"] + np.float32(0.7)
    xy, st2, good, ssim = ctx.klt_track(sq["im1"], guess, st)
    oxy, ost, ogood, ossim = lk.track(sq["im1"], guess.copy(), st)
    assert np.array_equal(st2, ost)                     # status codes: exact
    assert good == ogood
    ok = np.isin(ost, (0, 1, 2))
    assert np.allclose(xy[ok], oxy[ok], atol=1e-3, rtol=0)
    assert np.array_equal(xy, oxy)                      # and in fact bit-identical
    assert np.allclose(ssim[ok], ossim[ok], atol=1e-5)
    assert np.array_equal(xy[st == 3], guess[st == 3])
    # sanity: the tracker found the synthetic flow
    err = np.linalg.norm(xy[ost == 0] - sq["truth"][ost == 0], axis=1)
    assert np.median(err) < 0.5


def test_track_without_initial_flow_and_failures(ctx):
    sq, lk = _setup(ctx, 120, 9, flow_px=25.0)          # large flow: drift cap / SSIM failures appear
    st = np.zeros(len(sq["pts"]), np.int32)
    xy, st2, good, _ = ctx.klt_track(sq["im1"], sq["pts"], st, initial_flow=False, min_ssim=0.9)
    oxy, ost, ogood, _ = lk.track(sq["im1"], sq["pts"].copy(), st, initial_flow=False, min_ssim=0.9)
    assert np.array_equal(st2, ost) and good == ogood
    assert np.array_equal(xy, oxy)
    assert len(set(ost.tolist())) > 1                   # more than one status code is exercised


def test_border_points_and_mask(ctx):
    sq = S.make_lk_sequence(40, 11)
    h, w = sq["im0"].shape
    pts = np.concatenate([sq["pts"], np.array([[2.0, 3.0], [w - 3.0, h - 2.0], [w + 40.0, 10.0], [15.5, 15.5]], np.float32)])
    mask = np.full((h, w), 255, np.uint8)
    mask[200:260, 300:380] = 0
    ctx.klt_configure()
    ctx.klt_set_reference(sq["im0"], pts, mask)
    lk = LK.LucasKanadeOracle()
    lk.set_reference(sq["im0"], pts, mask)
    for i in range(len(pts)):
        t = ctx.klt_get_template(i)
        assert [bool(v) for v in t["valid"]] == [lk.Iref[l][i] is not None for l in range(5)], i
    st = np.zeros(len(pts), np.int32)
    xy, st2, good, _ = ctx.klt_track(sq["im1"], pts, st)
    oxy, ost, ogood, _ = lk.track(sq["im1"], pts.copy(), st)
    assert np.array_equal(st2, ost) and good == ogood
    assert (ost == 4).sum() >= 2                        # OUT_IMAGE_BOUNDARIES


def test_photometric_round_trip_and_clear(ctx):
    sq, lk = _setup(ctx, 30, 13)
    t = ctx.klt_get_template(4)
    n0 = ctx.klt_num_points()
    ctx.klt_insert_template(t)                          # PointReuse re-inserts stored templates (tracking.cc:473-503)
    assert ctx.klt_num_points() == n0 + 1
    t2 = ctx.klt_get_template(n0)
    for k in ("xy", "gray", "grad", "mean", "valid"):
        assert np.array_equal(t[k], t2[k])
    pts = np.concatenate([sq["pts"], sq["pts"][4:5]])
    xy, st, good, _ = ctx.klt_track(sq["im1"], pts, np.zeros(n0 + 1, np.int32))
    assert np.array_equal(xy[4], xy[n0]) and st[4] == st[n0]
    ctx.klt_clear()
    assert ctx.klt_num_points() == 0
    with pytest.raises(nrs.NrsError):
        ctx.klt_track(sq["im1"], pts, np.zeros(n0 + 1, np.int32))


def test_full_size_properties(ctx):
    """5k points on 640x480 (the size of BASELINE configs): tracking a frame against itself is the
    identity (size-independent property), and every point keeps its status."""
    sq = S.make_lk_sequence(5000, 21)
    ctx.klt_configure()
    ctx.klt_set_reference(sq["im0"], sq["pts"])
    st = np.zeros(len(sq["pts"]), np.int32)
    xy, st2, good, ssim = ctx.klt_track(sq["im0"], sq["pts"], st)
    assert good == len(sq["pts"]) and np.all(st2 == 0)
    assert np.max(np.abs(xy - sq["pts"])) < 0.05
    assert np.nanmin(ssim) > 0.99


def test_batched_templates_equal_single_point_calls(ctx):
    """nrs_klt_get_templates / nrs_klt_insert_templates are the single-point calls in a loop."""
    sq, lk = _setup(ctx, 40, 13)
    n = ctx.klt_num_points()
    batch = ctx.klt_get_templates(0, n)
    for i in (0, 5, n - 1):
        one = ctx.klt_get_template(i)
        for k in ("xy", "gray", "grad", "mean", "valid"):
            assert np.array_equal(batch[i][k], one[k]), k
    # re-insert a few into a fresh two-level tracker, in one call and one by one
    sel = [batch[i] for i in (1, 7, 20)]
    res = []
    for batched in (True, False):
        ctx.klt_clear()
        ctx.klt_configure(21, 1)
        if batched:
            ctx.klt_insert_templates(sel)
        else:
            for t in sel:
                ctx.klt_insert_template(t)
        assert ctx.klt_num_points() == 3
        pts = np.stack([t["xy"] for t in sel])
        res.append(ctx.klt_track(sq["im1"], pts + np.float32(0.5), np.zeros(3, np.int32)))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    ctx.klt_clear()
    ctx.klt_configure()


def test_archived_templates_equal_the_host_hand_over(ctx):
    """nrs_klt_archive_templates / nrs_klt_insert_archived: the map's photometric information kept in device memory by map point id.
    Archive some slots under arbitrary keys, overwrite one entry, then insert from the archive into (i) a fresh two-level tracker of
    ANOTHER context (PointReuse's tracker) and (ii) the archiving tracker itself -- byte for byte what get_templates + insert_templates
    hand over, and the same track results.  Unknown keys, bad slots and a tracker with more levels than the archive are refused."""
    sq, lk = _setup(ctx, 40, 13)
    n = ctx.klt_num_points()
    host = ctx.klt_get_templates(0, n)
    slots, keys = np.array([3, 7, 20, 11], np.int32), np.array([900, 2, 57, 900], np.int32)     # (key 900 is archived twice: the later slot stands)
    ctx.klt_archive_templates(slots, keys)
    other = nrs.Context()
    try:
        use_keys, use_slots = [2, 900, 57], [7, 11, 20]
        xy = np.stack([host[s]["xy"] for s in use_slots]) + np.float32(0.5)
        res = []
        for archived in (True, False):
            other.klt_clear()
            other.klt_configure(21, 1)
            if archived:
                other.klt_insert_archived(ctx, use_keys, xy)
            else:
                other.klt_insert_templates([dict(host[s], xy=xy[i]) for i, s in enumerate(use_slots)])
            assert other.klt_num_points() == 3
            got = other.klt_get_templates(0, 3)
            res.append((got, other.klt_track(sq["im1"], xy, np.zeros(3, np.int32))))
        for a, b in zip(res[0][0], res[1][0]):
            for k in ("xy", "gray", "grad", "mean", "valid"):
                assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(res[0][1][0], res[1][1][0]) and np.array_equal(res[0][1][1], res[1][1][1])
        # into the archiving tracker itself (a reused point becomes a new slot of the frame's tracker): all five levels
        ctx.klt_insert_archived(ctx, [57], host[20]["xy"][None])
        t = ctx.klt_get_template(n)
        for k in ("xy", "gray", "grad", "mean", "valid"):
            assert np.array_equal(t[k], host[20][k]), k
        with pytest.raises(nrs.NrsError):
            other.klt_insert_archived(ctx, [5], xy[:1])              # nothing archived under key 5
        with pytest.raises(nrs.NrsError):
            ctx.klt_archive_templates([n + 5], [1])                 # no such slot
        two = nrs.Context()
        try:
            two.klt_configure(21, 1)
            two.klt_set_reference(sq["im0"], sq["pts"][:4])
            two.klt_archive_templates([0], [0])
            with pytest.raises(nrs.NrsError):
                ctx.klt_insert_archived(two, [0], xy[:1])           # a five-level tracker cannot take a two-level entry
        finally:
            two.close()
    finally:
        other.close()
    ctx.klt_clear()
    ctx.klt_configure()


# ---- the template stores where they grow (csrc/nrs_klt.hip TemplateSet::reserve).  A store's first capacity is max(n + n / 2, 256) and it
# never shrinks, so every test here starts from contexts of its own; what is expected is read from the tracker before the growth.
KEYS = ("xy", "gray", "grad", "mean", "valid")
OUT_IMAGE_BOUNDARIES = 4


def _same_bytes(got, want, tag):
    assert len(got) == len(want), tag
    for i, (a, b) in enumerate(zip(got, want)):
        for k in KEYS:
            assert a[k].tobytes() == b[k].tobytes(), (tag, i, k)


def _grown_tracker():
    """200 stored points (capacity 300), then the first 150 inserted again: 350 points, which forces the store to grow with all 200 kept.
    Returns the context, the sequence, the 200 points, their templates as read BEFORE the growth and their track on im1 before it."""
    sq = S.make_lk_sequence(260, 17)
    pts = sq["pts"][:200]
    assert len(pts) == 200
    c = nrs.Context()
    c.klt_configure()
    c.klt_set_reference(sq["im0"], pts)
    before = c.klt_get_templates(0, 200)
    assert sum(int(t["valid"][0]) for t in before) > 150 and len({t["gray"].tobytes() for t in before}) > 150      # (the slots differ: a mix-up shows)
    track0 = c.klt_track(sq["im1"], pts + np.float32(0.7), np.zeros(200, np.int32))
    c.klt_insert_templates(before[:150])
    assert c.klt_num_points() == 350
    return c, sq, pts, before, track0


def test_tracker_growth_keeps_the_stored_templates():
    c, sq, pts, before, track0 = _grown_tracker()
    try:
        _same_bytes(c.klt_get_templates(0, 200), before, "kept")
        _same_bytes(c.klt_get_templates(200, 150), before[:150], "inserted")
        guess = np.concatenate([pts, pts[:150]]) + np.float32(0.7)
        xy, st, good, _ = c.klt_track(sq["im1"], guess, np.zeros(350, np.int32))
        assert np.array_equal(xy[:150], xy[200:], equal_nan=True) and np.array_equal(st[:150], st[200:])
        assert np.array_equal(xy[:200], track0[0], equal_nan=True) and np.array_equal(st[:200], track0[1])      # ... and what they gave before the growth
        assert good == track0[2] + int((st[200:] == 0).sum()) and (st == 0).sum() > 175
    finally:
        c.close()


def test_tracker_growth_entered_through_insert_archived():
    c, sq, pts, before, _ = _grown_tracker()
    try:
        c.klt_archive_templates(np.arange(200), np.arange(200))
        xy = pts + np.float32(0.25)
        c.klt_insert_archived(c, np.arange(200), xy)                # 550 > 525: the store grows inside the call, 350 kept
        assert c.klt_num_points() == 550
        _same_bytes(c.klt_get_templates(0, 350), before + before[:150], "kept")
        _same_bytes(c.klt_get_templates(350, 200), [dict(t, xy=xy[i]) for i, t in enumerate(before)], "archived")
    finally:
        c.close()


def test_archive_growth_keeps_its_entries_and_their_has_bytes():
    """key 10 (archive capacity 256), then key 1000 (capacity 1501): key 10's entry and its device-side "has" byte are carried over, the
    "has" bytes of the keys between read zero -- on the host (insert_archived refuses them) and on the device (point_reuse finds key 999
    never filled, and key 10 filled)"""
    sq = S.make_lk_sequence(40, 13)
    pts = sq["pts"]
    c, other = nrs.Context(), nrs.Context()
    try:
        c.klt_configure()
        c.klt_set_reference(sq["im0"], pts)
        host = c.klt_get_templates(0, len(pts))
        c.klt_archive_templates([3], [10])
        c.klt_archive_templates([7], [1000])
        other.klt_configure()
        xy = np.stack([host[3]["xy"], host[7]["xy"]]) + np.float32(0.5)
        other.klt_insert_archived(c, [10, 1000], xy)
        _same_bytes(other.klt_get_templates(0, 2), [dict(host[3], xy=xy[0]), dict(host[7], xy=xy[1])], "archive")
        for key in (11, 999):
            with pytest.raises(nrs.NrsError):
                other.klt_insert_archived(c, [key], xy[:1])
        assert other.klt_num_points() == 2
        # the device side: a map of 1000 points, all held by the frame but 10 and 999, which project onto two of the stored points
        h, w = sq["im0"].shape
        prm = np.array([64, 64, w / 2, h / 2, 0, 0, 0, 0], np.float32)
        uv = np.stack([host[3]["xy"], host[7]["xy"]]).astype(np.float64)
        map_pos = np.tile(np.array([[0.05, 0.05, 2]], np.float32), (1000, 1))
        map_pos[[10, 999]] = np.stack([(uv[:, 0] - prm[2]) / prm[0] * 2, (uv[:, 1] - prm[3]) / prm[1] * 2, np.full(2, 2.0)], 1).astype(np.float32)
        frame_slot = np.arange(1000)
        frame_slot[[10, 999]] = -1
        n0 = c.klt_num_points()
        d = c.point_reuse(nrs.make_camera(S.PINHOLE, prm), np.array([0, 0, 0, 1], np.float32), np.zeros(3, np.float32), (w, h), map_pos, frame_slot,
                          np.zeros(1000, np.int32), [], 0.75, False)
        assert d["cand_id"].tolist() == [10, 999]
        assert d["status"][1] == OUT_IMAGE_BOUNDARIES and not d["accepted"][1]          # never filled (test_key_that_was_never_archived)
        assert d["status"][0] == 0 and d["accepted"][0] and np.abs(d["xy"][0] - d["seed_xy"][0]).max() < 0.1      # its own image: it stays
        assert d["n_new"] == 0 and c.klt_num_points() == n0
    finally:
        c.close()
        other.close()


def test_archive_starts_over_under_another_level_count():
    sq = S.make_lk_sequence(40, 13)
    pts = sq["pts"]
    c, two, five = nrs.Context(), nrs.Context(), nrs.Context()
    try:
        c.klt_configure()
        c.klt_set_reference(sq["im0"], pts)
        c.klt_archive_templates([3], [5])
        c.klt_clear()
        c.klt_configure(21, 1)
        c.klt_set_reference(sq["im0"], pts[:4])
        want = c.klt_get_templates(0, 1)
        assert want[0]["gray"].shape[0] == 2
        c.klt_archive_templates([0], [9])
        two.klt_configure(21, 1)
        five.klt_configure()
        with pytest.raises(nrs.NrsError):
            two.klt_insert_archived(c, [5], pts[:1])                # archived under five levels only: gone with the restart
        two.klt_insert_archived(c, [9], pts[:1])
        _same_bytes(two.klt_get_templates(0, 1), want, "two levels")
        with pytest.raises(nrs.NrsError):
            five.klt_insert_archived(c, [9], pts[:1])               # the new entry has two levels: a five-level tracker cannot take it
    finally:
        c.close()
        two.close()
        five.close()
