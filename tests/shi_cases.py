"""The designed cases of f3 (Shi-Tomasi extraction, csrc/nrs_shi.hip) that tests/test_shi_cases_cpu.py vets on the CPU (the oracle's literal
pass against its closed form, and every entry of `claims`) and tests/test_gpu_shi_cases.py runs through the C ABI.  Plain NumPy, seeded;
no GPU, no `nrs` and no oracle import here: what a case claims about its input is stated from its construction and checked by the CPU test.

A case is a dict:
  name      unique
  nms       the extractor's NMS window (0..15)
  calls     [(image h x w uint8, held_xy n x 2 float32 or None, mask h x w uint8 or None), ...] passed through ONE extractor
  capacity  {call index: capacity} for the calls that do not give w * h
  claims    what the input is built to reach; tests/test_shi_cases_cpu.py has one checker per key and asserts every key of every case

Sizes are written w x h.  The score pass writes score rows 0 .. h-4, columns 1 .. w-2 (`written`); column 0, column w-1 and rows h-3 .. h-1
are never written and keep a -1 mark for the life of the extractor.

  ties_checker2[_nms0|_nms15]  0/255 checkerboard of 2 x 2 blocks, 64x40: a handful of distinct scores, keypoints 8-adjacent with equal score
  ties_checker4, ties_checker8 plateaus of equal maxima with gaps wider than the window
  dense_rows_<w>x<h>            uniform noise at nms 0: every written cell is a keypoint, w-2 a row (past one wave, past one 256-column chunk,
                                a keypoint either side of columns 255 | 256); second call under a mask that clears every third column;
                                dense_rows_300x8 has a third call with a capacity below the count
  marks_unwritten               marks in cells the score pass never writes suppress their 31 x 31 box on every later call; an interior one does not
  marks_many                    3000 held points (a dozen k_shi_mark workgroups), most of them duplicates, with the rounding boundaries
  size_change                   64x40 -> 41x41 -> 64x40 -> 300x5 -> 64x40 in one extractor
  geometry_<w>x<h>_<kind>_nms<n> the last-row pass at w == h, w == h + 1, h == 5 and w >> h, twice (the second call reads the first call's last row)
  threshold                     low contrast: scores either side of 80 within 10
  saturated                     0/255 steps, isolated 255 pixels and a 255 frame, all touching the border: gradients of +-1020

REFUSALS: held arrays whose SECOND point must be refused (the first is good), for the 64x40 image REFUSAL_IMAGE.

  nan_score_nms<n>              a score that IS NaN, on the second call of a sequence; it passes `!(cur < 80)`, beats nothing and is beaten by nothing

NaN scores.  A NaN score needs a negative radicand tr^2 - 4 det in float32.  Searched on the CPU with the oracle's closed form for 33 s:
20 000 random 8x6 and 5 000 random 12x9 images of each of six families (uniform noise, two-valued 0/255, two-valued with two equal rows,
low contrast 120..126, rank-one outer products, one step edge at a random angle), drawn in turn and passed through ONE extractor per size,
so that every image is also the second call after the one before it.  Five of the 150 000 calls left a NaN, every one on a two-valued image
that followed a uniform-noise image; the two looked at closer have it in the row the last-row pass writes (score row h-4), where the tensor
mixes this call's gradient rows h-3, h-2 with the previous call's last-row X gradients.  The same images through a fresh extractor give no
NaN, and no image of the rest of this table does.  `nan_score` is the first pair found; the literal pass and the closed form agree on it."""
import numpy as np

F32 = np.float32
W, H = 64, 40


def noise(w, h, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w)).astype(np.uint8)


def smooth(w, h, seed):
    """band-limited noise stretched to 0..255: distinct scores, sparse maxima"""
    a = np.random.default_rng(seed).normal(size=(h + 8, w + 8))
    for _ in range(2):
        a = (a[:-2] + a[1:-1] + a[2:]) / 3
        a = (a[:, :-2] + a[:, 1:-1] + a[:, 2:]) / 3
    a = a[2:2 + h, 2:2 + w]
    return (255 * (a - a.min()) / (a.max() - a.min())).astype(np.uint8)


def checker(w, h, block):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy // block) + (xx // block)) % 2) * 255).astype(np.uint8)


def written(w, h):
    """boolean h x w map of the cells the score pass writes"""
    m = np.zeros((h, w), bool)
    m[:h - 3, 1:w - 1] = True
    return m


def _xy(cells):
    return np.array(cells, F32).reshape(-1, 2)


def _case(name, nms, calls, claims, capacity=None):
    calls = [(np.ascontiguousarray(im, np.uint8), None if held is None else np.ascontiguousarray(held, F32).reshape(-1, 2),
              None if mask is None else np.ascontiguousarray(mask, np.uint8)) for im, held, mask in calls]
    for im, held, mask in calls:
        assert im.shape[1] >= im.shape[0] >= 5 and max(im.shape) <= 300 and (mask is None or mask.shape == im.shape)
        for a in (im, held, mask):
            if a is not None:
                a.setflags(write=False)
    assert 1 <= len(calls) <= 5
    return dict(name=name, nms=nms, calls=calls, claims=claims, capacity=dict(capacity or {}))


CASES = []

# ---- ties ----------------------------------------------------------------------------------------------------------------------------------
_HELD_TIES = _xy([(20, 12), (41, 25)])                             # second call: the same image with two interior marks
for _nms, _tag, _min_kp in ((5, "", 1000), (0, "_nms0", 2000), (15, "_nms15", 1000)):
    _im = checker(W, H, 2)
    CASES.append(_case("ties_checker2" + _tag, _nms, [(_im, None, None), (_im, _HELD_TIES, None)],
                       dict(cells_ge80_min=2000, distinct_scores_max=16, keypoints_min=_min_kp, adjacent_equal_pair=True)))
for _b, _min_kp in ((4, 400), (8, 100)):
    _im = checker(W, H, _b)
    CASES.append(_case("ties_checker%d" % _b, 5, [(_im, None, None), (_im, _HELD_TIES, None)],
                       dict(keypoints_min=_min_kp, adjacent_equal_pair=True, distinct_scores_max=16)))

# ---- dense rows ----------------------------------------------------------------------------------------------------------------------------
DENSE_WIDTHS, DENSE_HEIGHTS = (255, 256, 257, 258, 300), (6, 8)


def third_column_mask(w, h):
    m = np.full((h, w), 255, np.uint8)
    m[:, ::3] = 0
    return m


for _w in DENSE_WIDTHS:
    for _h in DENSE_HEIGHTS:
        _calls = [(noise(_w, _h, 1000 + _w + _h), None, None), (noise(_w, _h, 2000 + _w + _h), None, third_column_mask(_w, _h))]
        _cap = None
        if (_w, _h) == (300, 8):
            _calls.append((noise(_w, _h, 3000 + _w + _h), None, None))
            _cap = {2: 700}                                         # (h - 3)(w - 2) = 1490 keypoints
        CASES.append(_case("dense_rows_%dx%d" % (_w, _h), 0, _calls, dict(dense=True), _cap))

# ---- marks ---------------------------------------------------------------------------------------------------------------------------------
UNWRITTEN_MARKS = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (0, 20), (W - 1, 20), (30, H - 1), (30, H - 3)]
INTERIOR_MARK = (32, 18)
CASES.append(_case("marks_unwritten", 0,
                   [(noise(W, H, 11), _xy(UNWRITTEN_MARKS + [INTERIOR_MARK]), None), (noise(W, H, 12), None, None), (noise(W, H, 13), None, None)],
                   dict(dense_minus_boxes=[UNWRITTEN_MARKS + [INTERIOR_MARK], UNWRITTEN_MARKS, UNWRITTEN_MARKS])))


def _marks_many():
    """3000 held points on ~300 cells.  Every point is an integer cell plus an offset whose rounding is written out here: +-0.25 and +-0.49
    stay, +0.5 goes UP (half away from zero), and the listed boundary values land where the comment says."""
    rng = np.random.default_rng(21)
    cx, cy = rng.integers(1, W - 2, 300), rng.integers(1, H - 2, 300)           # (a + 0.5 offset must still land inside)
    pick = rng.integers(0, 300, 2990)
    kind = rng.integers(0, 6, 2990)
    off = np.array([0.0, 0.25, -0.25, 0.49, -0.49, 0.5])[kind]
    up = (kind == 5).astype(np.int64)
    ox, oy = off, np.roll(off, 1)
    ux, uy = up, np.roll(up, 1)
    pts = np.stack([cx[pick] + ox, cy[pick] + oy], 1)
    cells = set(zip((cx[pick] + ux).tolist(), (cy[pick] + uy).tolist()))
    boundary = [((-0.4, 7.0), (0, 7)),                             # -0.4 -> cell 0
                ((-0.49, 8.5), (0, 9)),                            # -0.49 -> 0, 8.5 -> 9
                ((9.0, -0.4), (9, 0)),
                ((10.5, -0.49), (11, 0)),                          # 10.5 -> 11
                ((W - 1 + 0.49, 11.0), (W - 1, 11)),               # w - 1 + 0.49 -> w - 1
                ((12.0, H - 1 + 0.49), (12, H - 1)),
                ((W - 1.5, H - 1.5), (W - 1, H - 1)),              # w - 1.5 -> w - 1
                ((0.5, 0.5), (1, 1)),
                ((-0.0, 13.0), (0, 13)),
                ((2.5, 3.5), (3, 4))]
    pts = np.concatenate([pts, np.array([b[0] for b in boundary])]).astype(F32)
    cells |= {b[1] for b in boundary}
    order = rng.permutation(len(pts))
    return pts[order], sorted(cells)


_PTS_MANY, _CELLS_MANY = _marks_many()
CASES.append(_case("marks_many", 0, [(noise(W, H, 22), _PTS_MANY, None), (noise(W, H, 23), None, None)],
                   dict(marked_cells=_CELLS_MANY, held_min=3000, duplicates_min=2000)))

# ---- refusals (data for the GPU test; the oracle must raise for each) ------------------------------------------------------------------------
REFUSAL_IMAGE = noise(W, H, 31)
REFUSAL_IMAGE.setflags(write=False)
_GOOD = (20.25, 10.0)
REFUSALS = []
for _v, _tag in ((-0.5, "minus_half"), (np.nan, "nan"), (np.inf, "inf"), (-np.inf, "minus_inf"), (1e30, "1e30")):
    REFUSALS.append(("x_" + _tag, _xy([_GOOD, (_v, 12.0)])))
    REFUSALS.append(("y_" + _tag, _xy([_GOOD, (12.0, _v)])))
REFUSALS.append(("x_w_minus_half", _xy([_GOOD, (W - 0.5, 12.0)])))
REFUSALS.append(("y_h_minus_half", _xy([_GOOD, (12.0, H - 0.5)])))

# ---- a size change inside one extractor ------------------------------------------------------------------------------------------------------
CASES.append(_case("size_change", 3,
                   [(noise(64, 40, 41), _xy([(0, 5), (63, 30), (10, 39), (50, 37), (0, 0)]), None), (noise(41, 41, 42), None, None),
                    (noise(64, 40, 43), None, None), (noise(300, 5, 44), None, None), (noise(64, 40, 45), None, None)],
                   dict(fresh_at_every_size=True)))

# ---- geometry of the last-row pass -----------------------------------------------------------------------------------------------------------
GEOMETRY_SIZES = ((5, 5), (6, 5), (300, 5), (41, 41), (42, 41), (7, 7))
for _w, _h in GEOMETRY_SIZES:
    for _kind, _make in (("dense", noise), ("smooth", smooth)):
        for _nms in (0, 2):
            _s = 50 + 7 * _w + _h
            CASES.append(_case("geometry_%dx%d_%s_nms%d" % (_w, _h, _kind, _nms), _nms,
                               [(_make(_w, _h, _s), None, None), (_make(_w, _h, _s + 1), None, None)],
                               dict(last_row_memory=True)))

# ---- threshold -------------------------------------------------------------------------------------------------------------------------------
CASES.append(_case("threshold", 0, [(noise(W, H, 67, 120, 127), None, None)], dict(near_threshold=(5, 5))))


# ---- saturated -------------------------------------------------------------------------------------------------------------------------------
def _saturated():
    steps = np.zeros((H, W), np.uint8)
    steps[:, 20:] = 255                                            # a vertical edge from the first row to the last
    steps[25:, :] = 255 - steps[25:, :]                            # a horizontal edge from the first column to the last, crossing it
    dots = np.zeros((H, W), np.uint8)
    for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (1, 1), (2, 0), (0, 7), (W - 1, 9), (31, H - 1), (33, H - 2), (17, 0), (40, 20), (42, 20)):
        dots[y, x] = 255
    frame = np.zeros((H, W), np.uint8)
    frame[0, :] = frame[-1, :] = 255
    frame[:, 0] = frame[:, -1] = 255
    return steps, dots, frame


CASES.append(_case("saturated", 2, [(_im, None, None) for _im in _saturated()], dict(gradient_1020=True, tensor_below_2_24=True)))

# ---- a NaN score -----------------------------------------------------------------------------------------------------------------------------
_NAN_PREV = np.array([[36, 163, 196, 104, 97, 202, 176, 150], [94, 68, 42, 99, 172, 169, 72, 83], [108, 40, 211, 169, 40, 245, 154, 185],
                      [130, 0, 223, 160, 110, 178, 238, 82], [158, 157, 86, 52, 39, 73, 125, 69], [109, 129, 247, 9, 126, 79, 44, 169]], np.uint8)
_NAN_IMAGE = 255 * np.array([[1, 1, 1, 0, 0, 1, 0, 1], [0, 0, 0, 0, 1, 0, 1, 0], [0, 0, 0, 1, 0, 1, 0, 1],
                             [0, 1, 1, 0, 0, 0, 1, 1], [0, 1, 1, 1, 0, 0, 0, 1], [1, 0, 1, 0, 1, 1, 1, 0]], np.uint8)
for _nms in (0, 2):
    CASES.append(_case("nan_score_nms%d" % _nms, _nms, [(_NAN_PREV, None, None), (_NAN_IMAGE, None, None), (noise(8, 6, 71), None, None)],
                       dict(nan_cells=[[], [(3, 2)], []])))

NAMES = [c["name"] for c in CASES]
assert len(set(NAMES)) == len(NAMES)
BY_NAME = dict(zip(NAMES, CASES))
