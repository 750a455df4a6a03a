"""GPU: the resident stereo pair (include/nrs.h nrs_front_process_stereo and "the resident stereo pair").

  * nrs_front_process_stereo: every output of either eye equals tests/front_oracle.py byte for byte, and the left eye's equal
    nrs_front_process(left) on a second context -- in the pair launches and with NRS_FRONT_PER_EYE;
  * the slot rules: the left slot serves the nrs_*_front calls as after nrs_front_process(left); a one-image call or a configuration
    leaves no pair behind;
  * nrs_stereo_match_pattern_front, nrs_init_stereo_front and nrs_stereo_match_lk_front give, bit for bit, what the host-pointer forms give
    on the downloaded grey bytes, and what the oracles give where the host-pointer forms are held to them exactly."""
import numpy as np
import pytest

import eval_oracle as E
import front_cases as FC
import front_oracle as FO
import lk_cases as LC
import nrs
import nrs_synth as S
import stereo_cases as SC

pytestmark = pytest.mark.gpu
F32 = np.float32
STATE, INVALID = -5, -1
KLT = dict(win=21, max_iters=10, epsilon=1e-4, min_eig=1e-4)


def _padded(img, ch, pad):
    """(h x stride raw bytes, stride): the rows of img followed by `pad` bytes of 0xEE"""
    h, w = img.shape[:2]
    raw = np.full((h, w * ch + pad), 0xEE, np.uint8)
    raw[:, :w * ch] = img.reshape(h, w * ch)
    return raw, w * ch + pad


@pytest.mark.parametrize("ch", [1, 3, 4])
# tiles divide the image / the CLAHE padding branch / past one block of 256 in x (w > 256, w % 256 != 0, w % 8 != 0: the second block's
# x >= w guard, which the other two sizes never reach, and the padding branch again)
@pytest.mark.parametrize("wh", [(64, 48), (70, 52), (300, 44)], ids=lambda s: "%dx%d" % s)
def test_pair_equals_the_oracle_per_eye(wh, ch):
    w, h = wh
    left = FC.blobs(h, w, ch, 100 + w + ch)
    right = (FC.blobs(h, w, ch, 200 + w + ch) // 2 + FC.noise(h, w, ch, 300 + w + ch) // 2).astype(np.uint8)
    filters = [("bright", 225), FC.border(h, w)]
    (raw_l, sl), (raw_r, sr) = _padded(left, ch, 5), _padded(right, ch, 12)
    a, b = nrs.Context(), nrs.Context()
    try:
        a.front_configure(filters)
        b.front_configure(filters)
        ref_r = FO.front_process(right, [])
        mono = b.front_process(left)
        for per_eye in (None, "1"):
            a.debug_set("NRS_FRONT_PER_EYE", per_eye)
            out = a.front_process_stereo(raw_l, raw_r, stride_l=sl, stride_r=sr, width=w, channels=ch)
            tag = (wh, ch, per_eye)
            FC.check_against_oracle(out, left, filters, tag)
            for k in ("gray", "clahe"):
                assert np.array_equal(out[k + "_right"], ref_r[k]), (tag, k, "right")
            for k in ("gray", "clahe", "global"):
                assert np.array_equal(out[k], mono[k]), (tag, k, "mono")
            assert len(out["masks"]) == 2 and all(np.array_equal(x, y) for x, y in zip(out["masks"], mono["masks"])), tag
            assert (out["global"] == 0).any() and not np.array_equal(out["clahe"], out["clahe_right"])
        # the contiguous form and a subset of the outputs
        a.debug_set("NRS_FRONT_PER_EYE", None)
        sub = a.front_process_stereo(left, right, outputs=("clahe_right",))
        assert list(sub) == ["clahe_right"] and np.array_equal(sub["clahe_right"], ref_r["clahe"])
    finally:
        a.close()
        b.close()


def _frames(w, h, seed):
    """two RGB frames of one texture (the second shifted by a few pixels) with a saturated blob and a black corner"""
    rng = np.random.default_rng(seed)
    tex = np.clip(np.rint(S._texture(h + 8, w + 8, rng, 0)), 0, 254).astype(np.uint8)
    out = []
    for dx, dy in ((0, 0), (3, 2)):
        g = tex[4 + dy:4 + dy + h, 4 + dx:4 + dx + w].copy()
        g[h // 3:h // 3 + h // 6, w // 2:w // 2 + w // 6] = 255
        g[:h // 8, :w // 8] = 0
        out.append(np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2)))
    return out


def test_left_slot_serves_the_front_calls_as_after_a_single_frame():
    w, h = 160, 120
    f0, f1 = _frames(w, h, 77)
    a, b = nrs.Context(), nrs.Context()
    try:
        for c in (a, b):
            c.klt_configure(max_level=4, **KLT)
            c.shi_configure(5)
            c.front_configure([("bright", 225)])
        a.front_process_stereo(f0, f1, outputs=False)
        b.front_process(f0, outputs=False)
        ea, eb = a.shi_extract_front(None, nrs.FRONT_CLAHE, True), b.shi_extract_front(None, nrs.FRONT_CLAHE, True)
        assert ea[2] == eb[2] and ea[2] > 8 and np.array_equal(ea[0], eb[0]) and np.array_equal(ea[1], eb[1])
        pts = np.vstack([ea[0], [[w // 2 + 4.5, h // 3 + 5.25]]]).astype(F32)                 # one point inside the masked blob
        a.klt_set_reference_front(pts, nrs.FRONT_GRAY, True)
        b.klt_set_reference_front(pts, nrs.FRONT_GRAY, True)
        for x, y in zip(a.klt_get_templates(0, len(pts)), b.klt_get_templates(0, len(pts))):
            for k in ("xy", "mean", "valid"):
                assert np.array_equal(x[k], y[k], equal_nan=True), k
            ok = x["valid"] != 0
            assert np.array_equal(x["gray"][ok], y["gray"][ok]) and np.array_equal(x["grad"][ok], y["grad"][ok])
        a.front_process_stereo(f1, f0, outputs=False)
        b.front_process(f1, outputs=False)
        st = np.zeros(len(pts), np.int32)
        ra, rb = a.klt_track_front(pts, st, nrs.FRONT_GRAY), b.klt_track_front(pts, st, nrs.FRONT_GRAY)
        assert np.array_equal(ra[0], rb[0], equal_nan=True) and np.array_equal(ra[1], rb[1]) and ra[2] == rb[2]
        assert np.array_equal(ra[3][ra[1] == 0], rb[3][rb[1] == 0])
    finally:
        a.close()
        b.close()


def _refused(fn):
    with pytest.raises(nrs.NrsError) as ei:
        fn()
    return ei.value.code


def test_slot_rules_and_refusals():
    sc = SC.pattern_scene()
    cam = nrs.make_camera(0, SC.PRM)
    c, t = nrs.Context(), nrs.Context()
    try:
        t.klt_configure(max_level=1, **KLT)
        xy = sc["xy"][:3]
        consumers = [lambda s: c.stereo_match_pattern_front(cam, SC.BF_PATTERN, xy, shape=s),
                     lambda s: c.init_stereo_front(cam, xy, shape=s),
                     lambda s: nrs.stereo_lk_front(t, c, cam, SC.BF_PATTERN, xy, shape=s),
                     lambda s: nrs.stereo_lk_front(c, c, cam, SC.BF_PATTERN, xy, shape=s)]
        good, wrong = (SC.PH, SC.PW), ((SC.PH, SC.PW + 8), (SC.PH - 8, SC.PW))
        for fn in consumers:                                        # nothing processed yet
            assert _refused(lambda: fn(good)) == STATE
        c.front_process_stereo(sc["left"], sc["right"], outputs=False)
        for fn in consumers[:3]:
            fn(good)
            for s in wrong:                                         # another size than the resident pair's
                assert _refused(lambda: fn(s)) == STATE
        assert "resident pair is 64 x 48" in str(pytest.raises(nrs.NrsError, lambda: consumers[2](wrong[0])).value)   # (the other context's text)
        assert _refused(lambda: c.stereo_match_pattern_front(cam, SC.BF_PATTERN, xy, image=2)) == INVALID
        c.front_process(sc["left"], outputs=False)                  # a single frame invalidates the right slot ...
        for fn in consumers:
            assert _refused(lambda: fn(good)) == STATE
        c.klt_set_reference_front(xy, nrs.FRONT_GRAY, True)         # ... and is itself resident
        c.front_process_stereo(sc["left"], sc["right"], outputs=False)
        consumers[0](good)
        c.front_configure([("bright", 225)])                       # configuring drops both slots
        for fn in consumers:
            assert _refused(lambda: fn(good)) == STATE
        assert _refused(lambda: c.klt_set_reference_front(xy, nrs.FRONT_GRAY, True, shape=good)) == STATE
        # refusals of the pair call itself
        l3 = FC.noise(SC.PH, SC.PW, 3, 1)
        assert _refused(lambda: c.front_process_stereo(l3, FC.noise(SC.PH, SC.PW + 2, 3, 2))) == INVALID          # sizes differ
        assert _refused(lambda: c.front_process_stereo(l3, FC.noise(SC.PH - 2, SC.PW, 3, 2))) == INVALID
        assert _refused(lambda: c.front_process_stereo(l3, FC.noise(SC.PH, SC.PW, 4, 2))) == INVALID              # channel counts differ
        assert _refused(lambda: c.front_process_stereo(l3, None)) == INVALID                                      # a null right image
        raw, s = _padded(l3, 3, 0)
        for sl, sr in ((s, s - 1), (s - 1, s)):                     # a stride below the row length, either eye
            assert _refused(lambda: c.front_process_stereo(raw, raw, stride_l=sl, stride_r=sr, width=SC.PW, channels=3)) == INVALID
        assert _refused(lambda: c.front_process_stereo(raw, raw, stride_l=s, stride_r=s, width=SC.PW, channels=2)) == INVALID
        for fn in consumers:                                        # a refused call leaves no pair behind
            assert _refused(lambda: fn(good)) == STATE
        c.front_process_stereo(l3, l3, outputs=False)               # the context still works
        consumers[0](good)
    finally:
        c.close()
        t.close()


def _same_match(dev, ora):
    """tests/test_gpu_stereo.py's comparison with tests/eval_oracle.py: everything exact"""
    xyz, status, score, match = dev
    o_xyz, o_status, o_score, o_match = ora
    assert np.array_equal(status, o_status) and np.array_equal(match, o_match)
    assert np.array_equal(score.view(np.uint64)[~np.isnan(o_score)], o_score.view(np.uint64)[~np.isnan(o_score)])
    assert np.array_equal(np.isnan(score), np.isnan(o_score)) and np.array_equal(np.isnan(xyz), np.isnan(o_xyz))
    ok = o_status == E.OK
    assert np.array_equal(xyz[ok].view(np.uint32), o_xyz[ok].view(np.uint32))


@pytest.mark.parametrize("plain", [False, True], ids=["mfma", "plain"])
def test_pattern_matcher_on_the_resident_pair(plain):
    sc = SC.pattern_scene()
    cam = nrs.make_camera(0, SC.PRM)
    dev, host = nrs.Context(), nrs.Context()
    try:
        if plain:
            nrs.debug_set("NRS_STEREO_NO_MFMA", "1")
        out = dev.front_process_stereo(sc["left"], sc["right"], outputs=("gray", "gray_right", "clahe", "clahe_right"))
        assert np.array_equal(out["gray"], sc["left"]) and np.array_equal(out["gray_right"], sc["right"])
        for n in (0, 1, 17):
            xy = sc["xy"][:n]
            d = dev.stereo_match_pattern_front(cam, SC.BF_PATTERN, xy)
            hst = host.stereo_match_pattern(cam, SC.BF_PATTERN, out["gray"], out["gray_right"], xy)
            for x, y in zip(d, hst):
                assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), n
            _same_match(d, sc["oracle%d" % n])
        st = d[1]
        assert (st == E.OK).any() and (st == E.LOW_CORRELATION).any() and (st == E.OUT_OF_BOUNDS).any() and (st == E.SATURATED).any()
        # the selector applies to both eyes
        d = dev.stereo_match_pattern_front(cam, SC.BF_PATTERN, sc["xy"], image=nrs.FRONT_CLAHE)
        hst = host.stereo_match_pattern(cam, SC.BF_PATTERN, out["clahe"], out["clahe_right"], sc["xy"])
        for x, y in zip(d, hst):
            assert np.array_equal(x, y, equal_nan=True)
    finally:
        dev.close()
        host.close()


FIELDS = ("verdict", "n_matched", "n_gated", "n_clusters", "n_noise", "n_selected")
ARRAYS = ("match_status", "code", "raw_label", "label", "selected")


def test_init_stereo_on_the_resident_pair():
    sc = SC.init_scene()
    o = sc["oracle"]
    cam = nrs.make_camera(0, SC.PRM)
    dev, host = nrs.Context(), nrs.Context()
    try:
        out = dev.front_process_stereo(sc["raw_left"], sc["raw_right"], outputs=("gray", "gray_right"))
        assert np.array_equal(out["gray"], sc["left"]) and np.array_equal(out["gray_right"], sc["right"])
        r = dev.init_stereo_front(cam, sc["xy"], **sc["opts"])
        hst = host.init_stereo(cam, out["gray"], out["gray_right"], sc["xy"], **sc["opts"])
        assert set(r) == set(hst)
        for k in r:                                                 # every field of the result
            assert np.array_equal(np.asarray(r[k]), np.asarray(hst[k]), equal_nan=True), k
        # ... and the oracle, as tests/test_gpu_stereo_init.py holds the host-pointer form to it
        for k in FIELDS:
            assert int(r[k]) == int(o[k]), (k, r[k], o[k])
        for k in ARRAYS:
            assert np.array_equal(r[k], o[k]), k
        assert np.array_equal(np.isnan(r["xyz"]), np.isnan(o["xyz"]))
        ok = o["match_status"] == E.OK
        assert np.array_equal(r["xyz"][ok].view(np.uint32), o["xyz"][ok].view(np.uint32))
        assert r["selected_xyz"].tobytes() == o["selected_xyz"].tobytes()
        assert F32(r["median_depth"]).tobytes() == F32(o["median_depth"]).tobytes()
        assert r["verdict"] == 0 and r["n_clusters"] >= 1 and r["n_noise"] > 0
        e = dev.init_stereo_front(cam, np.zeros((0, 2), F32), **sc["opts"])                      # no keypoints: the host form's verdict
        assert e["verdict"] == 1 and e["n_matched"] == 0
        assert _refused(lambda: dev.init_stereo_front(cam, sc["xy"], **dict(sc["opts"], eps=0.0))) == INVALID
    finally:
        dev.close()
        host.close()


def test_lk_stereo_on_the_resident_pair():
    # 161 x 123: the smallest size tests/test_gpu_klt_cases.py uses with max_level 1 (two levels: 161 x 123 and 81 x 62)
    sq = LC.pair(161, 123, 5)
    im0, im1, pts = sq["im0"], sq["im1"], np.ascontiguousarray(sq["pts"], F32)
    cam = nrs.make_camera(0, SC.PRM)
    main, cs, cs2 = nrs.Context(), nrs.Context(), nrs.Context()
    try:
        main.klt_configure(max_level=4, **KLT)
        for c in (cs, cs2):
            c.klt_configure(max_level=1, **KLT)
        out = main.front_process_stereo(im0, im1, outputs=("gray", "gray_right"))
        main.klt_set_reference_front(pts[:10], nrs.FRONT_GRAY, True)            # the tracking templates of the main context
        before = main.klt_get_templates(0, 10)[3]
        d = nrs.stereo_lk_front(cs, main, cam, SC.BF_PATTERN, pts)
        hst = nrs.stereo_lk(cs2, cam, SC.BF_PATTERN, out["gray"], out["gray_right"], pts)
        for x, y, name in zip(d, hst, ("xyz", "status", "right_xy", "track_status")):
            assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), name
        print("LK stereo: %d of %d tracked, %d with a point" % ((d[3] == 1).sum(), len(pts), (d[1] == E.OK).sum()))
        assert (d[3] == 1).sum() > len(pts) // 2 and (d[1] == E.OK).any()
        assert cs.klt_num_points() == len(pts)
        assert main.klt_num_points() == 10                          # the main context's templates are left alone
        after = main.klt_get_templates(0, 10)[3]
        for k in before:
            assert np.array_equal(before[k], after[k], equal_nan=True), k
        # one context for both roles: the same result, and its tracking templates are replaced
        d2 = nrs.stereo_lk_front(main, main, cam, SC.BF_PATTERN, pts[:7])
        cs2.klt_configure(max_level=1, **KLT)
        assert main.klt_num_points() == 7 and np.isfinite(d2[2]).any()
        assert nrs.stereo_lk_front(cs, main, cam, SC.BF_PATTERN, pts[:0])[0].shape == (0, 3)
    finally:
        for c in (main, cs, cs2):
            c.close()
