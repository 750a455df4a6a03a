"""GPU: the frame resize on the device (include/nrs.h nrs_front_resize_configure / nrs_front_resize_taps / nrs_front_process_raw) against
tests/resize_oracle.py on the designed sizes of tests/resize_cases.py.

  * the tap tables equal the oracle's exactly;
  * the resized frame equals the oracle's resize byte for byte, the grey equals tests/front_oracle.py's grey of the oracle's resize, and
    every front-end output equals nrs_front_process fed the oracle's resize on a second context -- fused and with NRS_RESIZE_OWN_LAUNCH,
    with the resized output and without it (the instantiation that writes no colour pixel);
  * the resident consumers give, bit for bit, what the host-pointer forms give on the downloaded images (1440 x 1080 -> 720 x 540);
  * lifetime and refusals; the frame loop and the monocular initialiser fed raw frames against the same fed the oracle's resized frames."""
import numpy as np
import pytest

import front_cases as FC
import front_oracle as FO
import init_cases as IC
import nrs
import nrs_frame_loop as FL
import nrs_synth as S
import rect_cases as RC
import resize_cases as ZC
import resize_oracle as RO

pytestmark = pytest.mark.gpu
F32 = np.float32
STATE, INVALID = -5, -1
KLT = dict(win=21, max_level=4, max_iters=10, epsilon=1e-4, min_eig=1e-4)
FRONT = ("gray", "clahe", "global", "masks")


def _configure(ctx, name):
    sw, sh, dw, dh = ZC.CASES[name]
    ctx.front_resize_configure((sw, sh), (dw, dh))


def _refused(fn):
    with pytest.raises(nrs.NrsError) as ei:
        fn()
    return ei.value.code


def _same(a, b, tag):
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    bad = np.argwhere(a != b)
    assert len(bad) == 0, (tag, len(bad), bad[:4].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


@pytest.mark.parametrize("name", ZC.NAMES)
def test_taps_equal_the_oracle(name):
    sw, sh, dw, dh = ZC.CASES[name]
    want = ZC.taps(name)
    ctx = nrs.Context()
    try:
        _configure(ctx, name)
        got = ctx.front_resize_taps()
        assert got["box"] == want["box"]
        for k in ("sx", "ax", "sy", "by"):
            assert got[k].dtype == want[k].dtype, k
            _same(got[k], want[k], (name, k))
        only_by = np.zeros((dh, 2), np.int16)                        # every pointer may be null
        ctx._chk(ctx.lib.nrs_front_resize_taps(ctx.h, None, None, None, only_by.ctypes.data, None))
        _same(only_by, want["by"], (name, "by alone"))
    finally:
        ctx.close()


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("name", ZC.NAMES)
def test_raw_frame_equals_the_oracle(name, ch):
    sw, sh, dw, dh = ZC.CASES[name]
    img, want = ZC.raw(name, ch), ZC.resized(name, ch)
    filters = ZC.filters(name)
    raw, stride = ZC.padded(img, ch, 7)                              # 0xEE behind every row
    a, b = nrs.Context(), nrs.Context()
    try:
        a.front_configure(filters)
        b.front_configure(filters)
        _configure(a, name)
        ref = b.front_process(want)                                  # once: shared by the four forms below
        _same(ref["gray"], FO.to_gray(want), (name, ch, "the reference's grey"))
        for own in (None, "1"):
            a.debug_set("NRS_RESIZE_OWN_LAUNCH", own)
            for outputs in (True, FRONT):
                tag = (name, ch, own, outputs is True)
                out = a.front_process_raw(raw, outputs=outputs, stride=stride, width=sw, channels=ch)
                assert set(out) == set(FRONT) | ({"resized"} if outputs is True else set())
                if outputs is True:
                    _same(out["resized"], want, tag + ("resized",))
                _same(out["gray"], FO.to_gray(want), tag + ("gray", "oracle"))       # (so that the two sides are not both the device)
                for k in ("gray", "clahe", "global"):
                    _same(out[k], ref[k], tag + (k,))
                assert len(out["masks"]) == len(ref["masks"]) == len(filters)
                for i in range(len(filters)):
                    _same(out["masks"][i], ref["masks"][i], tag + ("mask", i))
            for kind in ("ramp", "extremes"):                        # the other images: the resized frame and its grey
                out = a.front_process_raw(ZC.raw(name, ch, kind), outputs=("resized", "gray"))
                _same(out["resized"], ZC.resized(name, ch, kind), (name, ch, own, kind))
                _same(out["gray"], FO.to_gray(ZC.resized(name, ch, kind)), (name, ch, own, kind, "gray"))
        # the contiguous form, nothing downloaded: the frame is resident at the resized size
        a.debug_set("NRS_RESIZE_OWN_LAUNCH", None)
        assert a.front_process_raw(img, outputs=False) == {} and a._front_shape == (dh, dw)
    finally:
        a.close()
        b.close()


def _frames(w, h, seed):
    """two RGB frames of one band-limited texture (the second shifted by a few pixels) with a saturated blob and a black corner"""
    rng = np.random.default_rng(seed)
    tex = np.clip(np.rint(S._texture(h + 16, w + 16, rng, 0)), 0, 254).astype(np.uint8)
    out = []
    for dx, dy in ((0, 0), (6, 4)):
        g = tex[8 + dy:8 + dy + h, 8 + dx:8 + dx + w].copy()
        g[h // 3:h // 3 + h // 6, w // 2:w // 2 + w // 6] = 255
        g[:h // 8, :w // 8] = 0
        out.append(np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2)))
    return out


def test_resident_consumers_after_a_raw_frame():
    """the Endomapper size, 1440 x 1080 -> 720 x 540 (nrs.half_size; the box branch): the extractor and the tracker on the frame the raw call
    left resident against the host-pointer entry points fed the downloaded bytes"""
    sw, sh = 1440, 1080
    dw, dh = nrs.half_size(sw, sh)
    assert (dw, dh) == (720, 540)
    f0, f1 = _frames(sw, sh, 77)
    filters = [("bright", 225), FC.border(dh, dw)]
    dev, host = nrs.Context(), nrs.Context()
    try:
        for c in (dev, host):
            c.klt_configure(**KLT)
            c.shi_configure(5)
        dev.front_configure(filters)
        dev.front_resize_configure((sw, sh), (dw, dh))
        assert dev.front_resize_taps()["box"] == 1
        o0 = dev.front_process_raw(f0)
        r0 = RO.resize(f0, dw, dh)
        _same(o0["resized"], r0, "resized")
        _same(o0["gray"], FO.to_gray(r0), "gray")
        assert o0["gray"].shape == (dh, dw) and (o0["global"] == 0).any() and (o0["global"] != 0).any()
        xy_d, id_d, n_d = dev.shi_extract_front(None, nrs.FRONT_CLAHE, True)
        xy_h, id_h, n_h = host.shi_extract(o0["clahe"], None, o0["global"])
        assert n_d == n_h and n_d > 8 and np.array_equal(xy_d, xy_h) and np.array_equal(id_d, id_h)
        pts = xy_h[(np.arange(64) * len(xy_h)) // 64].astype(F32)     # evenly over the extractor's (row-major) order
        dev.klt_set_reference_front(pts, nrs.FRONT_GRAY, True)
        host.klt_set_reference(o0["gray"], pts, o0["global"])
        td, th = dev.klt_get_templates(0, len(pts)), host.klt_get_templates(0, len(pts))
        assert any(t["valid"][0] for t in td)
        for x, y in zip(td, th):
            for k in ("xy", "mean", "valid"):
                assert np.array_equal(x[k], y[k], equal_nan=True), k
            ok = x["valid"] != 0
            for k in ("gray", "grad"):
                assert np.array_equal(x[k][ok], y[k][ok]), k
        # the next raw frame: uploaded once, nothing downloaded, tracked on the resident grey
        assert dev.front_process_raw(f1, outputs=False) == {}
        g1 = FO.to_gray(RO.resize(f1, dw, dh))
        st = np.zeros(len(pts), np.int32)
        rd = dev.klt_track_front(pts, st, nrs.FRONT_GRAY, initial_flow=True, min_ssim=0.7)
        rh = host.klt_track(g1, pts, st, initial_flow=True, min_ssim=0.7)
        assert np.array_equal(rd[0], rh[0], equal_nan=True) and np.array_equal(rd[1], rh[1]) and rd[2] == rh[2]
        passed = rd[1] == 0
        assert np.array_equal(rd[3][passed], rh[3][passed])
        print("n_good", rd[2], "of", len(pts))
        assert rd[2] > 4
        assert _refused(lambda: dev.klt_track_front(pts, st, nrs.FRONT_GRAY, shape=(sh, sw))) == STATE       # w x h is the resized size
    finally:
        dev.close()
        host.close()


def test_lifetime_and_refusals():
    big, small = "wide", "odd_both"
    bw, bh, bdw, bdh = ZC.CASES[big]
    sw, sh, sdw, sdh = ZC.CASES[small]
    c = nrs.Context()
    try:
        bimg, simg = ZC.raw(big, 3), ZC.raw(small, 3)
        # before any configuration
        assert _refused(lambda: c.front_process_raw(bimg)) == STATE
        assert "no resize has been configured" in c.lib.nrs_last_error(c.h).decode()
        assert _refused(lambda: c.front_resize_taps()) == STATE
        # the configuration's refusals: a zero size (half_size(1, 1)), a negative one, one past the limit
        for src, dst in (((1, 1), nrs.half_size(1, 1)), ((0, 48), (32, 24)), ((64, -1), (32, 24)), ((16385, 48), (32, 24)), ((64, 48), (0, 24)), ((64, 48), (32, 16385))):
            assert _refused(lambda: c.front_resize_configure(src, dst)) == INVALID
        assert "resized size 32 x 16385 (1 .. 16384 each)" in c.lib.nrs_last_error(c.h).decode()
        assert _refused(lambda: c.front_process_raw(bimg)) == STATE                       # a refused configuration configures nothing
        # the wide size first; then filters: nrs_front_configure keeps the tables
        _configure(c, big)
        before = c.front_resize_taps()
        filters = [("bright", 225)]
        c.front_configure(filters)
        after = c.front_resize_taps()
        for k in ("sx", "ax", "sy", "by"):
            assert before[k].tobytes() == after[k].tobytes() == ZC.taps(big)[k].tobytes(), k
        out = c.front_process_raw(bimg)
        _same(out["resized"], ZC.resized(big, 3), "wide")
        FC.check_against_oracle(out, ZC.resized(big, 3), filters, "wide")
        # a raw frame of another size, another channel count than 1 / 3 / 4, a stride below the row, an empty frame
        assert _refused(lambda: c.front_process_raw(simg)) == INVALID
        assert "the raw frame is 37 x 29, the configured one 531 x 71" in c.lib.nrs_last_error(c.h).decode()
        assert _refused(lambda: c.front_process_raw(bimg[:-1])) == INVALID
        raw, s = ZC.padded(bimg, 3, 0)
        assert _refused(lambda: c.front_process_raw(raw, stride=s - 1, width=bw, channels=3)) == INVALID
        assert _refused(lambda: c.front_process_raw(raw, stride=s, width=bw, channels=2)) == INVALID
        assert _refused(lambda: c.front_process_raw(raw, stride=s, width=0, channels=3)) == INVALID
        # a PREDEFINED mask has the RESIZED size
        c.front_configure([("predefined", FC.disk_mask(bh, bw))])
        assert _refused(lambda: c.front_process_raw(bimg)) == INVALID
        pre = [("predefined", FC.disk_mask(bdh, bdw))]
        c.front_configure(pre)
        FC.check_against_oracle(c.front_process_raw(bimg), ZC.resized(big, 3), pre, "predefined")
        # a second configuration with another size replaces the tables: a correct frame at the new size in the same buffers; configuring
        # drops the resident frame
        pts, st = np.array([[100.0, 17.0]], F32), np.zeros(1, np.int32)
        c.klt_configure(win=21, max_level=1, max_iters=10, epsilon=1e-4, min_eig=1e-4)
        consumer = lambda: c.klt_set_reference_front(pts, nrs.FRONT_GRAY, True)
        consumer()
        c.front_configure(filters)
        _configure(c, small)
        assert _refused(consumer) == STATE
        got = c.front_resize_taps()
        for k in ("sx", "ax", "sy", "by"):
            assert got[k].shape == ZC.taps(small)[k].shape and got[k].tobytes() == ZC.taps(small)[k].tobytes(), k
        assert _refused(lambda: c.front_process_raw(bimg)) == INVALID
        out = c.front_process_raw(simg)
        _same(out["resized"], ZC.resized(small, 3), "small")
        FC.check_against_oracle(out, ZC.resized(small, 3), filters, "small")
        assert _refused(lambda: c.klt_set_reference_front(pts, nrs.FRONT_GRAY, True, shape=(sh, sw))) == STATE     # w x h is the resized size
        # nrs_front_process (not raw) still works afterwards, at the plain size, and the tables outlive it
        FC.check_against_oracle(c.front_process(simg), simg, filters, "plain")
        assert c._front_shape == (sh, sw)
        _same(c.front_process_raw(simg, outputs=("resized",))["resized"], ZC.resized(small, 3), "after a plain frame")
        # the right-eye slot is invalidated by a raw frame; the stereo raw path is unaffected by a resize configuration
        rc = RC.cases()["rot_dist"]
        c.front_rectify_configure((rc["src_w"], rc["src_h"]), (rc["dst_w"], rc["dst_h"]), rc["left"], rc["right"])
        maps = [c.front_rectify_maps(e) for e in (0, 1)]
        rl, rr = RC.raw_pair("rot_dist", 3)
        c.front_process_stereo_raw(rl, rr, outputs=False)
        pair_consumer = lambda: c.klt_set_reference_front(pts[:1] * 0 + 30, nrs.FRONT_GRAY, True)
        pair_consumer()
        _configure(c, big)                                           # a resize configuration keeps the maps ...
        for e in (0, 1):
            for x, y in zip(maps[e], c.front_rectify_maps(e)):
                assert x.tobytes() == y.tobytes()
        out = c.front_process_stereo_raw(rl, rr)
        want_l, want_r = RC.rectified_pair("rot_dist", 3)
        _same(out["rect_left"], want_l, "stereo raw left")
        _same(out["rect_right"], want_r, "stereo raw right")
        FC.check_against_oracle(out, want_l, filters, "stereo raw")
        c.front_rectify_configure((rc["src_w"], rc["src_h"]), (rc["dst_w"], rc["dst_h"]), rc["left"], rc["right"])      # ... and the reverse
        assert c.front_resize_taps()["sx"].tobytes() == ZC.taps(big)["sx"].tobytes()
        c.front_process_stereo_raw(rl, rr, outputs=False)
        c.front_process_raw(bimg, outputs=False)
        assert _refused(lambda: c.front_process_stereo_raw(rl, None)) == INVALID
        import stereo_cases as SC
        cam = nrs.make_camera(0, SC.PRM)
        assert _refused(lambda: c.stereo_match_pattern_front(cam, SC.BF_PATTERN, np.array([[100.0, 17.0]], F32))) == STATE      # no right eye after a raw frame
    finally:
        c.close()


def test_resize_needs_the_front_mode():
    with pytest.raises(ValueError, match="resize needs the front mode"):
        FL.GpuBackend(nrs, S.PINHOLE, S.HAMLYN_PINHOLE, KLT, resize=dict(src_wh=(640, 480), dst_wh=(320, 240)))


def test_frame_loop_on_raw_frames_equals_the_loop_on_resized_frames():
    """four frames.  One backend is configured with the resize and handed the RAW frames, twice the size; the other is handed the oracle's
    resized frames.  The logs must agree byte for byte"""
    frames = 4
    sq = S.make_frame_sequence(200, frames, 12, S.PINHOLE)
    w, h = sq["wh"]
    raws, smalls = [], []
    rng = np.random.default_rng(4)
    for g in sq["images"]:
        g = g.copy()
        g[h // 2 - 30:h // 2 + 30, w // 2 - 40:w // 2 + 40] = 255          # a specular patch over tracked points
        big = np.repeat(np.repeat(g, 2, 0), 2, 1).astype(np.int16)
        big += rng.integers(-3, 4, big.shape).astype(np.int16)              # (no pixel-doubled image: the four pixels of a block differ)
        raw = np.ascontiguousarray(np.repeat(np.clip(big, 0, 255).astype(np.uint8)[:, :, None], 3, 2))
        raw[h - 60:h + 60, w - 80:w + 80] = 255
        raws.append(raw)
        smalls.append(RO.resize(raw, w, h))
    assert raws[0].shape == (2 * h, 2 * w, 3) and smalls[0].shape == (h, w, 3) and not np.array_equal(smalls[0][:, :, 0], sq["images"][0])
    filters = [("bright", 225), ("border", 20, 20, 50, 20, 0)]
    proj = lambda pc: FL.project_f32(sq["model"], sq["prm"], pc)
    opts = dict(win=21, max_level=4, max_iters=10, epsilon=1e-4, min_eig=1e-4)

    def run(backend, images):
        try:
            loop = FL.FrameLoop(backend, proj, sq["wh"], sq["scale"], sq["kp0"], sq["X0"], sq["graph"], sq["pose_q"][0], sq["pose_t"][0],
                                images[0], images_to_insert_keyframe=1)
            for f in range(1, frames):
                assert loop.track_image(images[f])
            return loop.log, backend.klt_get_templates(backend.ctx.klt_num_points()), backend.n_front_calls
        finally:
            backend.close()
    alog, at, an = run(FL.GpuBackend(nrs, sq["model"], sq["prm"], opts, front=filters, resize=dict(src_wh=(2 * w, 2 * h), dst_wh=nrs.half_size(2 * w, 2 * h))), raws)
    blog, bt, bn = run(FL.GpuBackend(nrs, sq["model"], sq["prm"], opts, front=filters), smalls)
    assert an == bn and len(alog) == len(blog) == frames - 1 and any(L["keyframe"] for L in alog) and alog[-1]["n_2d"] > 0
    for f, (x, y) in enumerate(zip(alog, blog), 1):
        for k in ("pose_q", "pose_t", "status_by_map", "pos_by_map", "kp_2d"):
            assert x[k].tobytes() == y[k].tobytes(), (f, k)
        for k in ("lost", "reused", "keyframe", "n_tracked", "n_2d"):
            assert x[k] == y[k], (f, k)
    assert len(at) == len(bt)
    for x, y in zip(at, bt):
        for k in ("xy", "mean", "valid"):
            assert np.array_equal(x[k], y[k], equal_nan=True), k


def test_mono_initializer_on_raw_frames_equals_it_on_resized_frames():
    """MonoInitializer.reset and one process_new_image on raw frames of 641 x 481 -- an odd size, half_size gives 320 x 240: the general
    branch -- against the same on the oracle's resized frames"""
    sq = IC.init_sequence()
    w, h = sq["wh"]
    sw, sh = 2 * w + 1, 2 * h + 1
    assert nrs.half_size(sw, sh) == (w, h)
    raws = []
    for g in sq["images"][:2]:
        big = np.repeat(np.repeat(g, 2, 0), 2, 1)
        big = np.pad(big, ((0, 1), (0, 1)), mode="edge")
        raws.append(np.ascontiguousarray(np.repeat(big[:, :, None], 3, 2)))
    smalls = [RO.resize(r, w, h) for r in raws]
    assert raws[0].shape == (sh, sw, 3) and smalls[0].shape == (h, w, 3)
    filters = [FC.border(h, w)]
    logs = []
    for resize, images in ((dict(src_wh=(sw, sh), dst_wh=(w, h)), raws), (None, smalls)):
        b = FL.GpuBackend(nrs, sq["model"], sq["prm"], IC.LOOP_KLT, front=filters, resize=resize)
        try:
            mo = FL.MonoInitializer(b, max_images=30, max_features=400, min_tracks=50, radians_per_pixel=F32(sq["radians_per_pixel"]))
            mo.reset(images[0])
            n_ref = len(mo.kp)
            mo.process_new_image(images[1])
            print("resize" if resize else "plain", "features", n_ref, "log", [(e["reset"], e["n_features"], e["n_tracks"], e["verdict"]) for e in mo.log])
            logs.append((n_ref, mo.log, mo.kp.copy(), mo.ref_kp.copy(), mo.status.copy(), b.n_front_calls))
        finally:
            b.close()
    (na, la, ka, ra, sa, ca), (nb, lb, kb, rb, sb, cb) = logs
    assert na == nb and na >= 50 and ca == cb == 2                   # one front-end call per frame
    assert len(la) == len(lb) == 1 and not la[0]["reset"] and la[0]["n_tracks"] >= 50       # the second frame was tracked, not taken as a new reference
    for k in la[0]:
        assert np.array_equal(np.asarray(la[0][k]), np.asarray(lb[0][k]), equal_nan=True), k
    assert ka.tobytes() == kb.tobytes() and ra.tobytes() == rb.tobytes() and np.array_equal(sa, sb)
