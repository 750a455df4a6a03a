"""CPU: hand-checkable pins of tests/front_oracle.py, the NumPy restatement the image front end (include/nrs.h f5) is held to."""
import numpy as np

import front_oracle as FO


def test_ellipse_rows_11_and_20():
    # 11x11: r = c = 5, dx = rint(5 sqrt((25 - dy^2) / 25)) = 0 3 4 5 5 5 5 5 4 3 0
    sp = FO.ellipse_spans(11, 11)
    assert [(j2 - j1 - 1) // 2 for j1, j2 in sp] == [0, 3, 4, 5, 5, 5, 5, 5, 4, 3, 0]
    assert all(j1 == 5 - d and j2 == 5 + d + 1 for (j1, j2), d in zip(sp, [0, 3, 4, 5, 5, 5, 5, 5, 4, 3, 0]))
    # 20x20: r = c = 10, dy = -10..9; dx = rint(sqrt(100 - dy^2)): sqrt(19) = 4.36, sqrt(36) = 6, sqrt(51) = 7.14, sqrt(64) = 8,
    # sqrt(75) = 8.66, sqrt(84) = 9.17, sqrt(91) = 9.54, sqrt(96) = 9.80, sqrt(99) = 9.95; the right end is cut at column 20
    dx = [0, 4, 6, 7, 8, 9, 9, 10, 10, 10, 10, 10, 10, 10, 9, 9, 8, 7, 6, 4]
    assert FO.ellipse_spans(20, 20) == [(10 - d, min(10 + d + 1, 20)) for d in dx]


def test_erode_10x10_anchor():
    # anchor 5: the window of output x covers x-5 .. x+4, so ONE zero at p zeroes the outputs p-4 .. p+5 (and the same in y)
    img = np.full((40, 40), 255, np.uint8)
    img[20, 17] = 0
    out = FO.erode_rect(img, 10, 10)
    ys, xs = np.nonzero(out == 0)
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (13, 22, 16, 25) and len(xs) == 100
    # pixels outside the image take no part: an all-255 image stays all-255, borders included
    assert (FO.erode_rect(np.full((7, 9), 255, np.uint8), 21, 21) == 255).all()
    assert (FO.erode_ellipse(np.full((7, 9), 255, np.uint8), 20) == 255).all()


def test_erode_ellipse_single_zero_is_the_reflected_element():
    img = np.full((31, 31), 255, np.uint8)
    img[15, 15] = 0
    out = FO.erode_ellipse(img, 11)
    # output (y, x) is zero iff the element holds the offset (15 - y, 15 - x); the 11x11 ellipse is symmetric
    want = np.full((31, 31), 255, np.uint8)
    for i, (j1, j2) in enumerate(FO.ellipse_spans(11, 11)):
        want[15 - (i - 5), 15 - (j2 - 1 - 5):15 - (j1 - 5) + 1] = 0
    assert np.array_equal(out, want)


def test_clahe_constant_image_is_one_lut():
    # every tile sees the same histogram, so every LUT is the same and the blend (weights sum to 1 up to rounding of
    # a*w + a*(1-w)) returns lut[v]: 160x120, tile 20x15 = 300 px, clip 3: bin v holds 300 -> 3, excess 297 -> batch 1, residual 41,
    # step 6: bins 0, 6, ..., 240 get one more.  cumsum at v = 77: 78 bins of 1 + 13 steps (0..72) + 3 = 94 -> rint(94 * 0.85) = 80
    img = np.full((120, 160), 77, np.uint8)
    luts, tw, th = FO.clahe_luts(img)
    assert (tw, th) == (20, 15) and FO.clahe_clip_limit(3.0, 300) == 3
    assert (luts == luts[0, 0]).all() and luts[0, 0, 77] == 80
    assert (FO.clahe(img) == 80).all()


def test_clahe_clip_floor():
    assert FO.clahe_clip_limit(3.0, 8 * 6) == 1            # int(3 * 48 / 256) = 0 -> floored to 1 (64x48)
    assert FO.clahe_clip_limit(3.0, 20 * 15) == 3          # int(3.52)
    assert FO.clahe_clip_limit(3.0, 80 * 60) == 56         # 640x480
    hist = np.zeros(256, np.int64)
    hist[10], hist[200] = 40, 8                            # 48 px
    one, three = FO.clahe_redistribute(hist, 1), FO.clahe_redistribute(hist, 3)
    assert one.sum() == 48 and three.sum() == 48
    # clip 1: excess 46 -> step 5: bins 0, 5, ..., 225 get one; clip 3: excess 42 -> step 6: bins 0, 6, ..., 246
    assert one[10] == 2 and one[200] == 2 and one[5] == 1 and one[230] == 0
    assert three[10] == 3 and three[200] == 3 and three[6] == 1 and three[246] == 1 and three[252] == 0


def test_clahe_residual_loop():
    def run(excess_bins, clip):
        hist = np.zeros(256, np.int64)
        for b, v in excess_bins:
            hist[b] = v
        return FO.clahe_redistribute(hist, clip)
    # residual 0: excess 256 -> batch 1, nothing left over
    r0 = run([(3, 10 + 256)], 10)
    assert r0[3] == 11 and (np.delete(r0, 3) == 1).all()
    # residual 1: step 256, only bin 0
    r1 = run([(3, 10 + 257)], 10)
    assert r1[0] == 2 and r1[3] == 11 and (np.delete(r1, [0, 3]) == 1).all()
    # residual 255: step 1, bins 0..254 get one, bin 255 none
    r255 = run([(3, 10 + 255)], 10)
    assert r255[255] == 0 and r255[3] == 11 and (np.delete(r255, [3, 255]) == 1).all()


def test_gray_fixed_point():
    px = np.array([[[255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 2, 3]]], np.uint8)
    # 9798 + 19235 + 3735 = 32768: white stays 255; (255*9798 + 16384) >> 15 = 76; G: 150; B: 29; (9798 + 38470 + 11205 + 16384) >> 15 = 2
    assert FO.to_gray(px).tolist() == [[255, 76, 150, 29, 2]]
    assert np.array_equal(FO.to_gray(np.dstack([px, np.full((1, 5, 1), 9, np.uint8)])), FO.to_gray(px))   # alpha ignored


def test_gauss_weights_and_blur_support():
    w = FO.gauss_weights()
    assert len(w) == 11 and all(a == b for a, b in zip(w, w[::-1])) and abs(float(sum(w)) - 1.0) < 1e-6
    assert float(w[0]) * float(w[0]) * 255 > 1.0           # the smallest weight product still rounds to >= 1: ~1.12
    rng = np.random.default_rng(5)
    for shape in ((48, 64), (7, 9), (61, 83)):
        gray = rng.integers(0, 256, shape).astype(np.uint8)
        gray[rng.uniform(size=shape) < 0.97] = 10          # a few bright pixels
        er = FO.erode_ellipse(FO.bright_threshold(gray, 128), 11)
        blur = FO.gaussian_blur(er)
        assert np.array_equal(blur != 0, FO.dilate_rect_reflect101(er, 11) != 0)
    assert (FO.gaussian_blur(np.full((20, 30), 255, np.uint8)) == 255).all()


def test_border_filter_black_image_and_roi():
    assert (FO.border_filter(np.zeros((48, 64), np.uint8), 2, 2, 2, 2) == 0).all()
    out = FO.border_filter(np.full((60, 80), 9, np.uint8), 5, 6, 7, 8)
    # ROI x 7..71, y 5..53, eroded by 21x21 (x-10..x+10): outside pixels take no part, so only the ROI's inner edges move
    ys, xs = np.nonzero(out)
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (17, 61, 15, 43)
    assert FO.border_roi(64, 48, 20, 20, 50, 20) is None and FO.border_roi(64, 48, 24, 24, 0, 0) is None
