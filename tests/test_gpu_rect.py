"""GPU: stereo rectification on the device (include/nrs.h nrs_front_rectify_configure / nrs_front_rectify_maps /
nrs_front_process_stereo_raw) against tests/rect_oracle.py on the designed cameras of tests/rect_cases.py.

  * the fp32 maps of both eyes equal the oracle's bit for bit;
  * the rectified eyes equal the oracle's remap byte for byte, every front-end output equals tests/front_oracle.py on the oracle's
    rectified image and nrs_front_process_stereo fed the downloaded rectified eyes on a second context -- fused and with
    NRS_RECT_OWN_LAUNCH, with the rect_* outputs and without them (the instantiation that writes no colour pixel);
  * the resident consumers give, bit for bit, what they give after nrs_front_process_stereo on the rectified bytes;
  * lifetime and refusals; the frame loop fed raw eyes against the frame loop fed the oracle's rectified eyes."""
import numpy as np
import pytest

import front_cases as FC
import front_oracle as FO
import nrs
import nrs_frame_loop as FL
import nrs_synth as S
import rect_cases as RC
import rect_oracle as RO
import stereo_cases as SC
from map_loop_backend import OPTS, RAD_PER_PIXEL

pytestmark = pytest.mark.gpu
F32 = np.float32
STATE, INVALID = -5, -1
KLT = dict(win=21, max_iters=10, epsilon=1e-4, min_eig=1e-4)
FRONT = ("gray", "clahe", "global", "masks", "gray_right", "clahe_right")


def _configure(ctx, c):
    ctx.front_rectify_configure((c["src_w"], c["src_h"]), (c["dst_w"], c["dst_h"]), c["left"], c["right"])


def _refused(fn):
    with pytest.raises(nrs.NrsError) as ei:
        fn()
    return ei.value.code


@pytest.mark.parametrize("name", RC.NAMES)
def test_maps_equal_the_oracle_bit_for_bit(name):
    c = RC.cases()[name]
    ctx = nrs.Context()
    try:
        _configure(ctx, c)
        for e, (ox, oy) in enumerate(RC.maps(name)):
            mx, my = ctx.front_rectify_maps(e)
            for dev, ora, axis in ((mx, ox, "x"), (my, oy, "y")):
                bad = np.argwhere(dev.view(np.uint32) != ora.view(np.uint32))
                assert len(bad) == 0, (name, e, axis, len(bad), bad[:4].tolist(), dev[tuple(bad[0])], ora[tuple(bad[0])])
        only_y = np.zeros((c["dst_h"], c["dst_w"]), F32)             # either pointer may be null
        ctx._chk(ctx.lib.nrs_front_rectify_maps(ctx.h, 1, None, only_y.ctypes.data))
        assert np.array_equal(only_y.view(np.uint32), RC.maps(name)[1][1].view(np.uint32))
    finally:
        ctx.close()


def _same(a, b, tag):
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, (tag, len(bad), bad[:4].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("name", RC.NAMES)
def test_rectified_pair_equals_the_oracle(name, ch):
    c = RC.cases()[name]
    w, h = c["dst_w"], c["dst_h"]
    left, right = RC.raw_pair(name, ch)
    rect_l, rect_r = RC.rectified_pair(name, ch)
    filters = [("bright", 225), FC.border(h, w)]
    ref_l, ref_r = FO.front_process(rect_l, FC.to_oracle(filters)), FO.front_process(rect_r, [])      # once: shared by the four forms below
    (raw_l, sl), (raw_r, sr) = RC.padded(left, ch, 5), RC.padded(right, ch, 12)                       # 0xEE behind every row, another stride per eye
    a, b = nrs.Context(), nrs.Context()
    try:
        a.front_configure(filters)
        b.front_configure(filters)
        _configure(a, c)
        pair = None
        for own in (None, "1"):
            a.debug_set("NRS_RECT_OWN_LAUNCH", own)
            for outputs in (True, FRONT):
                tag = (name, ch, own, outputs is True)
                out = a.front_process_stereo_raw(raw_l, raw_r, outputs=outputs, stride_l=sl, stride_r=sr, width=c["src_w"], channels=ch)
                assert set(out) == set(FRONT) | ({"rect_left", "rect_right"} if outputs is True else set())
                if outputs is True:
                    _same(out["rect_left"], rect_l, tag + ("rect_left",))
                    _same(out["rect_right"], rect_r, tag + ("rect_right",))
                    if pair is None:                                # the pair call on the DOWNLOADED rectified eyes, second context
                        pair = b.front_process_stereo(out["rect_left"], out["rect_right"])
                for k in ("gray", "clahe", "global"):
                    _same(out[k], ref_l[k], tag + (k, "oracle"))
                    _same(out[k], pair[k], tag + (k, "pair"))
                for k in ("gray", "clahe"):
                    _same(out[k + "_right"], ref_r[k], tag + (k, "right", "oracle"))
                    _same(out[k + "_right"], pair[k + "_right"], tag + (k, "right", "pair"))
                assert len(out["masks"]) == len(ref_l["masks"]) == len(pair["masks"]) == 2
                for i in range(2):
                    _same(out["masks"][i], ref_l["masks"][i], tag + ("mask", i, "oracle"))
                    _same(out["masks"][i], pair["masks"][i], tag + ("mask", i, "pair"))
        # the contiguous form, nothing downloaded: the pair is resident at the rectified size
        a.debug_set("NRS_RECT_OWN_LAUNCH", None)
        assert a.front_process_stereo_raw(left, right, outputs=False) == {} and a._front_shape == (h, w)
    finally:
        a.close()
        b.close()


def test_resident_consumers_after_a_raw_pair():
    """the pattern scene of stereo_cases as the RAW pair, rectified by the `ties` camera (64 x 48 -> 70 x 52, a shift of a few 1/64 pixel: the
    scene survives and the matcher still matches): the matcher and the tracker on the pair the raw call left resident against the same
    calls after nrs_front_process_stereo on the rectified bytes"""
    sc, c = SC.pattern_scene(), RC.cases()["ties"]
    cam = nrs.make_camera(0, SC.PRM)
    a, b = nrs.Context(), nrs.Context()
    try:
        for ctx in (a, b):
            ctx.klt_configure(max_level=1, **KLT)
        _configure(a, c)
        out = a.front_process_stereo_raw(sc["left"], sc["right"], outputs=("rect_left", "rect_right"))
        (lx, ly), (rx, ry) = RC.maps("ties")
        _same(out["rect_left"], RO.remap(sc["left"], lx, ly), "rect_left")
        _same(out["rect_right"], RO.remap(sc["right"], rx, ry), "rect_right")
        b.front_process_stereo(out["rect_left"], out["rect_right"], outputs=False)
        assert a._front_shape == b._front_shape == (c["dst_h"], c["dst_w"])
        for image in (nrs.FRONT_GRAY, nrs.FRONT_CLAHE):
            da, db = a.stereo_match_pattern_front(cam, SC.BF_PATTERN, sc["xy"], image=image), b.stereo_match_pattern_front(cam, SC.BF_PATTERN, sc["xy"], image=image)
            for x, y in zip(da, db):
                assert x.shape == y.shape and x.tobytes() == y.tobytes()
        assert (da[1] == 0).sum() >= 4                              # the comparison covers matched keypoints
        pts = sc["xy"][:12]
        for ctx in (a, b):
            ctx.klt_set_reference_front(pts, nrs.FRONT_GRAY, True)
        for x, y in zip(a.klt_get_templates(0, len(pts)), b.klt_get_templates(0, len(pts))):
            for k in x:
                assert np.array_equal(x[k], y[k], equal_nan=True), k
        # the next pair: the eyes swapped, tracked from the reference
        out = a.front_process_stereo_raw(sc["right"], sc["left"], outputs=("rect_left", "rect_right"))
        b.front_process_stereo(out["rect_left"], out["rect_right"], outputs=False)
        st = np.zeros(len(pts), np.int32)
        ra, rb = a.klt_track_front(pts, st, nrs.FRONT_GRAY), b.klt_track_front(pts, st, nrs.FRONT_GRAY)
        assert ra[0].tobytes() == rb[0].tobytes() and np.array_equal(ra[1], rb[1]) and ra[2] == rb[2]
        assert (ra[1] == 0).any() and ra[3][ra[1] == 0].tobytes() == rb[3][rb[1] == 0].tobytes()      # (a lost point has no SSIM)
    finally:
        a.close()
        b.close()


def test_lifetime_and_refusals():
    wide, small = RC.cases()["rational"], RC.cases()["rot_dist"]
    sc = SC.pattern_scene()
    cam = nrs.make_camera(0, SC.PRM)
    c = nrs.Context()
    try:
        wl, wr = RC.raw_pair("rational", 3)
        sl, sr = RC.raw_pair("rot_dist", 3)
        # before any configuration
        assert _refused(lambda: c.front_process_stereo_raw(wl, wr)) == STATE
        assert "no rectification has been configured" in str(pytest.raises(nrs.NrsError, lambda: c.front_rectify_maps(0, shape=(4, 4))).value)
        assert _refused(lambda: c.front_rectify_maps(0, shape=(4, 4))) == STATE
        # the configuration's refusals
        good = (small["left"], small["right"])
        cfg = lambda src, dst, l, r: c.front_rectify_configure(src, dst, l, r)
        assert _refused(lambda: cfg((64, 48), (70, 52), None, good[1])) == INVALID and _refused(lambda: cfg((64, 48), (70, 52), good[0], None)) == INVALID
        for src, dst in (((0, 48), (70, 52)), ((64, -1), (70, 52)), ((16385, 48), (70, 52)), ((64, 48), (0, 52)), ((64, 48), (70, 16385))):
            assert _refused(lambda: cfg(src, dst, *good)) == INVALID
        for field, idx in (("K", 2), ("dist", 1), ("R", 4), ("P", 0)):
            for bad in (np.inf, np.nan):
                e = {k: np.array(v, np.float64).copy() for k, v in good[1].items()}
                e[field].reshape(-1)[idx] = bad
                assert _refused(lambda: cfg((64, 48), (70, 52), good[0], e)) == INVALID
                assert "right eye: %s[%d] is not finite" % (field, idx) in c.lib.nrs_last_error(c.h).decode()
        flat = dict(good[0], P=np.zeros((3, 3)))
        assert _refused(lambda: cfg((64, 48), (70, 52), flat, good[1])) == INVALID and "det(P R)" in c.lib.nrs_last_error(c.h).decode()
        assert _refused(lambda: c.front_process_stereo_raw(wl, wr)) == STATE          # a refused configuration configures nothing
        # the wide camera first; then filters: nrs_front_configure keeps the maps
        _configure(c, wide)
        before = [c.front_rectify_maps(e) for e in (0, 1)]
        filters = [("bright", 225)]
        c.front_configure(filters)
        for e in (0, 1):
            for x, y in zip(before[e], c.front_rectify_maps(e)):
                assert x.tobytes() == y.tobytes()
        out = c.front_process_stereo_raw(wl, wr)
        rl, rr = RC.rectified_pair("rational", 3)
        _same(out["rect_left"], rl, "wide left")
        _same(out["rect_right"], rr, "wide right")
        FC.check_against_oracle(out, rl, filters, "wide")
        # a raw pair of another size, another channel count than 1 / 3 / 4, a null right eye, a stride below the row
        assert _refused(lambda: c.front_process_stereo_raw(sl, sr)) == INVALID
        assert "the raw eyes are 64 x 48, the configured ones 300 x 44" in c.lib.nrs_last_error(c.h).decode()
        assert _refused(lambda: c.front_process_stereo_raw(wl[:-1], wr[:-1])) == INVALID
        assert _refused(lambda: c.front_process_stereo_raw(wl, None)) == INVALID
        raw, s = RC.padded(wl, 3, 0)
        assert _refused(lambda: c.front_process_stereo_raw(raw, raw, stride_l=s, stride_r=s - 1, width=300, channels=3)) == INVALID
        assert _refused(lambda: c.front_process_stereo_raw(raw, raw, stride_l=s, stride_r=s, width=300, channels=2)) == INVALID
        # a PREDEFINED mask has the RECTIFIED size
        c.front_configure([("predefined", FC.disk_mask(wide["src_h"], wide["src_w"]))])
        assert _refused(lambda: c.front_process_stereo_raw(wl, wr)) == INVALID
        pre = [("predefined", FC.disk_mask(wide["dst_h"], wide["dst_w"]))]
        c.front_configure(pre)
        FC.check_against_oracle(c.front_process_stereo_raw(wl, wr), rl, pre, "predefined")
        # a second configuration, smaller: a correct frame at the new size in the same buffers; configuring drops the resident pair
        consumer = lambda: c.stereo_match_pattern_front(cam, SC.BF_PATTERN, sc["xy"][:3])
        consumer()
        c.front_configure(filters)
        _configure(c, small)
        assert _refused(consumer) == STATE
        for e, (ox, oy) in enumerate(RC.maps("rot_dist")):
            mx, my = c.front_rectify_maps(e)
            assert mx.shape == (52, 70) and mx.tobytes() == ox.tobytes() and my.tobytes() == oy.tobytes()
        out = c.front_process_stereo_raw(sl, sr)
        rl, rr = RC.rectified_pair("rot_dist", 3)
        _same(out["rect_left"], rl, "small left")
        _same(out["rect_right"], rr, "small right")
        FC.check_against_oracle(out, rl, filters, "small")
        _same(out["gray_right"], FO.to_gray(rr), "small right grey")
        consumer()
        assert _refused(lambda: c.stereo_match_pattern_front(cam, SC.BF_PATTERN, sc["xy"][:3], shape=(48, 64))) == STATE      # w x h is the rectified size
        # a one-image call afterwards leaves no pair behind, and is itself resident; the maps outlive it
        c.front_process(sl, outputs=False)
        assert _refused(consumer) == STATE
        c.klt_configure(max_level=1, **KLT)
        c.klt_set_reference_front(sc["xy"][:3], nrs.FRONT_GRAY, True)
        _same(c.front_process_stereo_raw(sl, sr, outputs=("rect_right",))["rect_right"], rr, "after a single frame")
        consumer()
    finally:
        c.close()


def test_frame_loop_on_raw_eyes_equals_the_loop_on_rectified_eyes():
    """three stereo frames at 96 x 64.  One backend is configured with the rectification and handed the RAW eyes; the other is handed the
    oracle's rectified eyes.  Both eyes take the same camera -- a zoom of 2 % about a centre off the pixel grid, so rows stay rows -- and the
    logs must agree byte for byte"""
    w, h = 96, 64
    sq = S.make_stereo_init_sequence(wh=(w, h), bf=720.0)
    frames = [1, 2]
    e = RC.eye(RC.cam(100, 48.3, 32.2), RC.cam(98, 48, 32))
    mx, my = RO.build_map(e, w, h)
    assert len(np.unique(RO.fix(mx, my)[2])) == 32                   # no identity: every fraction occurs
    raw_l = {f: np.ascontiguousarray(np.repeat(sq["images"][f][:, :, None], 3, 2)) for f in [0] + frames}
    raw_r = {f: np.ascontiguousarray(np.repeat(sq["right"][:, :, None], 3, 2)) for f in [0] + frames}
    rect_l = {f: RO.remap(raw_l[f], mx, my) for f in raw_l}
    rect_r = {f: RO.remap(raw_r[f], mx, my) for f in raw_r}
    # (the generator's eps = 6 mm, min_points = 5 are sized for the keypoint density of 320 x 240.  At 96 x 64 the extractor leaves about 45
    # keypoints of which ten find a match, and the loop needs ten tracked points per frame: a 4-pixel grid joins them -- the stereo start
    # takes any keypoints -- and twice the radius with three points keeps the matched ones in one cluster)
    opts = dict(bf=sq["bf"], z_min=sq["z_min"], z_max=sq["z_max"], eps=2 * sq["eps"], min_points=3)
    gx, gy = np.meshgrid(np.arange(22, 88, 4), np.arange(10, 56, 4))
    grid = np.stack([gx.ravel(), gy.ravel()], 1).astype(F32)
    proj = lambda pc: FL.project_f32(sq["model"], sq["prm"], pc)
    logs = []
    for rectify, lefts, rights in ((dict(src_wh=(w, h), dst_wh=(w, h), left=e, right=e), raw_l, raw_r), (None, rect_l, rect_r)):
        b = FL.GpuBackend(nrs, sq["model"], sq["prm"], OPTS, dense_graph=True, front=True, rectify=rectify)
        try:
            b.front_stereo(lefts[0], rights[0])
            xy = np.vstack([b.extract_features(lefts[0], None, None)[0], grid]).astype(F32)
            r = b.init_stereo(lefts[0], rights[0], xy, **opts)
            print("rectify" if rectify else "plain", "keypoints", len(xy), "verdict", r["verdict"], "selected", r["n_selected"])
            assert r["verdict"] == 0 and b.n_front_calls == 1
            loop = FL.FrameLoop.from_stereo_initialization(b, proj, sq["wh"], r, lefts[0], mapping=True, rad_per_pixel=RAD_PER_PIXEL,
                                                           camera=(sq["model"], sq["prm"]))
            for f in frames:
                ok = loop.track_image_with_stereo(lefts[f], rights[f])
                print("  frame", f, "tracked with 3D", loop.log[-1]["n_tracked"], "lost", len(loop.log[-1]["lost"]))
                assert ok
            assert b.n_front_calls == 1 + len(frames)
            logs.append((r, loop.log, loop.map_pos.copy(), loop.kp.copy(), loop.status.copy()))
        finally:
            b.close()
    (ra, la, pa, ka, sa), (rb, lb, pb, kb, sb) = logs
    for k in ra:
        assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k]), equal_nan=True), k
    assert len(la) == len(lb) == len(frames)
    for x, y in zip(la, lb):
        for k in ("pose_q", "pose_t", "pos_by_map", "kp_2d"):
            assert x[k].tobytes() == y[k].tobytes(), k
        assert np.array_equal(x["status_by_map"], y["status_by_map"]) and np.array_equal(x["status_after_mapping"], y["status_after_mapping"])
        for k in ("lost", "reused", "n_tracked", "keyframe", "n_2d", "map_size", "mapping"):
            assert x[k] == y[k], k
    assert pa.tobytes() == pb.tobytes() and ka.tobytes() == kb.tobytes() and np.array_equal(sa, sb)
