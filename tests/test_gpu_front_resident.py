"""GPU: the resident hand-over of the image front end (include/nrs.h nrs_klt_set_reference_front / nrs_klt_track_front /
nrs_shi_extract_front).  The frame is uploaded once (nrs_front_process); the tracker and the extractor then run on the resident grey /
CLAHE image and Global mask and must give the SAME BITS as the host-pointer entry points fed the downloaded bytes."""
import numpy as np
import pytest

import nrs
import nrs_frame_loop as FL
import nrs_synth as S
import front_cases as FC
import front_oracle as FO

pytestmark = pytest.mark.gpu

STATE = -5
OPTS = dict(win=21, max_level=4, max_iters=10, epsilon=1e-4, min_eig=1e-4)


def _frames(w, h, seed):
    """two RGB frames of one band-limited texture (the second shifted by a few pixels) with a saturated blob and a black corner"""
    rng = np.random.default_rng(seed)
    tex = np.clip(np.rint(S._texture(h + 8, w + 8, rng, 0)), 0, 254).astype(np.uint8)
    out = []
    for dx, dy in ((0, 0), (3, 2)):
        g = tex[4 + dy:4 + dy + h, 4 + dx:4 + dx + w].copy()
        g[h // 3:h // 3 + h // 6, w // 2:w // 2 + w // 6] = 255
        g[:h // 8, :w // 8] = 0
        out.append(np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2)))
    return out


def _same_templates(ta, tb):
    """positions, means and filled flags of every (point, level); window contents where the level is filled -- a level the tracker did not
    fill (beyond the pyramid, window outside the image, masked) keeps whatever its buffer held, in either context"""
    assert len(ta) == len(tb)
    for a, b in zip(ta, tb):
        for k in ("xy", "mean", "valid"):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        ok = a["valid"] != 0
        for k in ("gray", "grad"):
            assert np.array_equal(a[k][ok], b[k][ok]), k


@pytest.mark.parametrize("wh", [(160, 120), (640, 480)], ids=lambda s: "%dx%d" % s)
def test_front_variants_equal_the_host_pointer_forms(wh):
    w, h = wh
    f0, f1 = _frames(w, h, 31 + w)
    # (160x120: a 21x21 template window under BorderFilter + BrightFilter is masked almost everywhere; the small frame keeps the blob's mask only)
    filters = [("bright", 225), FC.border(h, w)] if w >= 640 else [("bright", 225)]
    dev, host = nrs.Context(), nrs.Context()
    try:
        for c in (dev, host):
            c.klt_configure(**{k: OPTS[k] for k in ("win", "max_level", "max_iters", "epsilon", "min_eig")})
            c.shi_configure(5)
        dev.front_configure(filters)
        o0 = dev.front_process(f0)
        assert (o0["global"] == 0).any() and (o0["global"] != 0).any()
        # ExtractFeatures on the CLAHE image under the Global mask (tracking.cc:217-221)
        xy_d, id_d, n_d = dev.shi_extract_front(None, nrs.FRONT_CLAHE, True)
        xy_h, id_h, n_h = host.shi_extract(o0["clahe"], None, o0["global"])
        assert n_d == n_h and n_d > 8 and np.array_equal(xy_d, xy_h) and np.array_equal(id_d, id_h)
        for a, b in zip(dev.shi_buffers(), host.shi_buffers()):
            assert np.array_equal(a, b)
        unmasked = host.shi_extract(o0["clahe"], None, None)[2]
        dev.shi_extract_front(None, nrs.FRONT_CLAHE, False)     # (keeps the two extractors' id counters and buffers in step)
        assert unmasked > n_h                                   # the mask does drop keypoints
        # SetReferenceImage on the grey image under the Global mask (tracking.cc:367,383)
        pts = np.vstack([xy_h, [[w // 2 + 4.5, h // 3 + 5.25]]]).astype(np.float32)      # one point inside the masked blob
        dev.klt_set_reference_front(pts, nrs.FRONT_GRAY, True)
        host.klt_set_reference(o0["gray"], pts, o0["global"])
        td, th = dev.klt_get_templates(0, len(pts)), host.klt_get_templates(0, len(pts))
        _same_templates(td, th)
        assert not td[-1]["valid"].any() and any(t["valid"][0] for t in td)
        # Track on the next frame's grey image (tracking.cc:303-307): the frame is uploaded once, nothing is downloaded
        assert dev.front_process(f1, outputs=False) == {}
        g1 = FO.to_gray(f1)
        st = np.zeros(len(pts), np.int32)
        rd = dev.klt_track_front(pts, st, nrs.FRONT_GRAY, initial_flow=True, min_ssim=0.7)
        rh = host.klt_track(g1, pts, st, initial_flow=True, min_ssim=0.7)
        assert np.array_equal(rd[0], rh[0], equal_nan=True) and np.array_equal(rd[1], rh[1]) and rd[2] == rh[2]
        passed = rd[1] == 0                                     # (the SSIM of a point that never reached the gate is not written)
        assert np.array_equal(rd[3][passed], rh[3][passed])
        print("n_good", wh, rd[2], "of", len(pts))
        assert w < 640 or rd[2] > 4                            # the large frame does track (the small one has room for few whole templates)
        # a keyframe's extraction on the grey image with the held keypoints (tracking.cc:353,372-380): the stateful second call
        held = rd[0][rd[1] == 0]
        o1 = dev.front_process(f1, outputs=("gray", "global"))
        assert np.array_equal(o1["gray"], g1)
        e_d = dev.shi_extract_front(held, nrs.FRONT_GRAY, True)
        e_h = host.shi_extract(o1["gray"], held, o1["global"])
        assert e_d[2] == e_h[2] and np.array_equal(e_d[0], e_h[0]) and np.array_equal(e_d[1], e_h[1])
        for a, b in zip(dev.shi_buffers(), host.shi_buffers()):
            assert np.array_equal(a, b)
    finally:
        dev.close()
        host.close()


def test_state_refusals():
    c = nrs.Context()
    try:
        pts = np.array([[60.0, 50.0]], np.float32)
        st = np.zeros(1, np.int32)

        def refused(fn):
            with pytest.raises(nrs.NrsError) as ei:
                fn()
            return ei.value.code
        calls = [lambda s: c.klt_set_reference_front(pts, nrs.FRONT_GRAY, True, shape=s),
                 lambda s: c.klt_track_front(pts, st, nrs.FRONT_GRAY, shape=s),
                 lambda s: c.shi_extract_front(None, nrs.FRONT_GRAY, True, shape=s)]
        for fn in calls:                                        # nothing processed yet
            assert refused(lambda: fn((120, 160))) == STATE
        c.front_configure([("bright", 225)])
        for fn in calls:
            assert refused(lambda: fn((120, 160))) == STATE
        img = FC.noise(120, 160, 3, 2)
        c.front_process(img, outputs=False)
        for fn in calls:                                        # another size than the resident frame's
            assert refused(lambda: fn((120, 168))) == STATE and refused(lambda: fn((100, 160))) == STATE
        calls[0]((120, 160))
        calls[1]((120, 160))
        calls[2]((120, 160))
        assert refused(lambda: c.klt_set_reference_front(pts, 2, True)) == -1      # unknown image selector
        c.front_configure([("bright", 200)])                   # configuring drops the resident frame
        for fn in calls:
            assert refused(lambda: fn((120, 160))) == STATE
    finally:
        c.close()


class _HostFrontBackend(FL.GpuBackend):
    """the loop's steps on host-made inputs: grey image and Global mask from tests/front_oracle.py, host-pointer entry points"""

    def __init__(self, filters, *a, **k):
        super().__init__(*a, **k)
        self._filters, self._cache = FC.to_oracle(filters), {}

    def _host(self, im):
        if id(im) not in self._cache:
            r = FO.front_process(im, self._filters)
            self._cache[id(im)] = (im, r["gray"], r["global"])
        return self._cache[id(im)][1:]

    def klt_set_reference(self, im, pts):
        g, m = self._host(im)
        self.ctx.klt_set_reference(g, pts, m)

    def klt_track(self, im, pts, status, min_ssim):
        return super().klt_track(self._host(im)[0], pts, status, min_ssim)

    def reuse_track_archived(self, im, pts, mps, min_ssim):
        return super().reuse_track_archived(self._host(im)[0], pts, mps, min_ssim)

    def extract_features(self, im, held_xy, mask=None):
        g, m = self._host(im)
        return super().extract_features(g, held_xy, m)


def test_frame_loop_with_the_front_end_equals_the_loop_on_host_made_masks():
    frames = 4
    sq = S.make_frame_sequence(200, frames, 12, S.PINHOLE)
    w, h = sq["wh"]
    raws = []
    for g in sq["images"]:
        g = g.copy()
        g[h // 2 - 30:h // 2 + 30, w // 2 - 40:w // 2 + 40] = 255          # a specular patch over tracked points
        raws.append(np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2)))
    filters = [("bright", 225), ("border", 20, 20, 50, 20, 0)]             # data/hamlyn_19/filters.txt with th 225
    proj = lambda pc: FL.project_f32(sq["model"], sq["prm"], pc)

    def run(backend):
        try:
            loop = FL.FrameLoop(backend, proj, sq["wh"], sq["scale"], sq["kp0"], sq["X0"], sq["graph"], sq["pose_q"][0], sq["pose_t"][0],
                                raws[0], images_to_insert_keyframe=1)
            for f in range(1, frames):
                assert loop.track_image(raws[f])
            return loop.log, backend.klt_get_templates(backend.ctx.klt_num_points())
        finally:
            backend.close()
    glog, gt = run(FL.GpuBackend(nrs, sq["model"], sq["prm"], OPTS, front=filters))
    hlog, ht = run(_HostFrontBackend(filters, nrs, sq["model"], sq["prm"], OPTS))
    assert any(L["keyframe"] for L in glog) and glog[-1]["n_2d"] > 0
    for f, (g, o) in enumerate(zip(glog, hlog), 1):
        for k in ("pose_q", "pose_t", "status_by_map", "pos_by_map", "kp_2d"):
            assert np.array_equal(g[k], o[k], equal_nan=True), (f, k)
        for k in ("lost", "reused", "keyframe", "n_tracked", "n_2d"):
            assert g[k] == o[k], (f, k)
    _same_templates(gt, ht)
    # the masks did take part: the templates under the specular patch are invalid at the first keyframe
    assert any(not t["valid"].all() for t in gt)
