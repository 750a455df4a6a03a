"""The Lucas-Kanade cases tests/test_lk_cases_cpu.py vets on the CPU (NumPy oracle against the C++ restatement) and
tests/test_gpu_klt_cases.py runs through the C ABI: short pyramids, odd level sizes, dead windows, the border gates, bad numbers and
configurations other than the default.

A case is a dict: im0 (reference image), im1 (tracked image), pts (reference points), guess, status (input LandmarkStatus), mask
(None or h x w bytes for set-reference), cfg (max_level, max_iters, epsilon, min_eig), initial_flow, min_ssim, and `truth` where the
pair has one.  `case(name)` builds it once, `oracle(name)` runs oracle/lk_oracle.py on it once; both are shared by every test and
must not be written to.  Every builder asserts on the oracle's result that its case exercises what it is named after (`_vet_*`), and
`vet_table()` that the table as a whole produces every status code.

Sizes (a level exists while the next halving stays above the 21-pixel window):
  161 x 123 -> 81 x 62 -> 41 x 31               3 levels, every halving odd in one dimension
   97 x  45 -> 49 x 23                           2 levels
   23 x  22                                      1 level: no position passes the post-update test 12 <= x < w - 12, so every point
                                                 ends OUT_IMAGE_BOUNDARIES or BAD_FEATURE; templates, statuses and positions still compare
  175 x 177 -> 88 x 89 -> 44 x 45 -> 22 x 23    4 levels, an odd size at every level in one dimension or the other

The gates (DESIGN.md 4 "Lucas-Kanade tracker"), with o = floor(coordinate at the level - 10) the window origin:
  set-reference  -10 <= o < dim - 10            a template is made
  track          -11 <= o < dim - 11            previous point (else the level is skipped, OUT at level 0) and every iterate
  SSIM           -11 <= o < dim - 22            final position.  No finite position is decided by this test (vet_ssim_gate_reach says why
                                                 and checks it on every case): it is held on its inside, up to o = dim - 23
                                                 (ssim_border_l0), and on its non-finite side, where a NaN position that left the iteration
                                                 usable is refused (ssim_nonfinite_l0).  gates_*_l0 also put GUESSES at o = dim - 23,
                                                 dim - 22, dim - 21."""
import functools

import numpy as np

import lk_oracle as LK
import nrs_synth as S

F32 = np.float32
DEFAULT = dict(max_level=4, max_iters=10, epsilon=1e-4, min_eig=1e-4)
USABLE = (0, 1, 2)


def n_levels(w, h, max_level):
    n = 1
    while n <= max_level and (w + 1) // 2 > 21 and (h + 1) // 2 > 21:
        w, h, n = (w + 1) // 2, (h + 1) // 2, n + 1
    return n


@functools.lru_cache(maxsize=None)
def pair(w, h, seed, flow=2.0):
    sq = S.make_lk_sequence(40, seed, wh=(w, h), flow_px=flow)
    for v in sq.values():
        v.setflags(write=False)
    return sq


def _case(im0, im1, pts, guess=None, status=None, mask=None, cfg=None, initial_flow=True, min_ssim=0.7, truth=None):
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 2)
    c = dict(im0=np.ascontiguousarray(im0), im1=np.ascontiguousarray(im1), pts=pts,
             guess=np.ascontiguousarray(pts + F32(0.7) if guess is None else guess, F32).reshape(-1, 2),
             status=np.zeros(len(pts), np.int32) if status is None else np.ascontiguousarray(status, np.int32), mask=mask,
             cfg=dict(DEFAULT, **(cfg or {})), initial_flow=initial_flow, min_ssim=min_ssim, truth=truth)
    assert len(c["guess"]) == len(pts) == len(c["status"])
    return c


def run_oracle(c, **cfg):
    """(tracker, (xy, status, n_good, ssim)) of oracle/lk_oracle.py on case c, with configuration entries replaced by cfg"""
    lk = LK.LucasKanadeOracle(21, **dict(c["cfg"], **cfg))
    lk.set_reference(c["im0"], c["pts"], c["mask"])
    return lk, lk.track(c["im1"], c["guess"].copy(), c["status"].copy(), c["initial_flow"], c["min_ssim"])


def oracle_templates(lk):
    """the oracle's templates in the layout of nrs.Context.klt_get_templates: gray (n, L, 21, 21), grad (n, L, 21, 21, 2), mean (n, L, 2),
    valid (n, L); zeros where a level holds no template"""
    n, L = len(lk.prev), lk.max_level + 1
    gray, grad = np.zeros((n, L, 21, 21), np.int16), np.zeros((n, L, 21, 21, 2), np.int16)
    mean, valid = np.zeros((n, L, 2), F32), np.zeros((n, L), np.uint8)
    for l in range(L):
        mean[:, l, 0], mean[:, l, 1] = lk.meanI[l], lk.meanI2[l]
        for i in range(n):
            if lk.Iref[l][i] is not None:
                gray[i, l], grad[i, l], valid[i, l] = lk.Iref[l][i], lk.Idref[l][i], 1
    return dict(gray=gray, grad=grad, mean=mean, valid=valid)


def _grid(xs, ys, seed):
    """hand-placed points: a grid with seeded sub-pixel offsets"""
    rng = np.random.default_rng(seed)
    g = np.array([(x, y) for y in ys for x in xs], np.float64)
    return (g + rng.uniform(-0.4, 0.4, g.shape)).astype(F32)


# ---- short pyramids (default configuration: max_level 4) and odd halvings with a full pyramid ------------------------------------------
def _short(w, h, seed, pts=None, cfg=None):
    sq = pair(w, h, seed)
    truth = sq["truth"] if pts is None else None
    return _case(sq["im0"], sq["im1"], sq["pts"] if pts is None else pts, cfg=cfg, truth=truth)


def _vet_short(c):
    """a short pyramid tracks what the same pair tracks with max_level = k - 1, and the tracker does run at every level it has"""
    h, w = c["im0"].shape
    k = n_levels(w, h, c["cfg"]["max_level"])
    assert k < c["cfg"]["max_level"] + 1
    lk, r = run_oracle(c)
    lk2, r2 = run_oracle(c, max_level=k - 1)
    assert r[2] == r2[2] and np.array_equal(r[1], r2[1])
    assert all(any(t is not None for t in lk.Iref[l]) for l in range(k)) and all(t is None for l in range(k, 5) for t in lk.Iref[l])
    return r


def _vet_full(c):
    h, w = c["im0"].shape
    assert n_levels(w, h, c["cfg"]["max_level"]) == c["cfg"]["max_level"] + 1
    lk, r = run_oracle(c)
    assert r[2] >= len(c["pts"]) - 2 and all(any(t is not None for t in lv) for lv in lk.Iref)


# ---- dead windows ------------------------------------------------------------------------------------------------------------------------
def _dead(value, in_reference, max_level):
    """a 44 x 44 patch of `value` centred on point 0 of the 161 x 123 pair, in the tracked image (or the reference image); two more
    points straddle the patch's edge, the others lie outside"""
    sq = pair(161, 123, 5)
    p0 = sq["pts"][0]
    cx, cy = int(p0[0]), int(p0[1])
    assert 22 <= cx < 161 - 22 and 22 <= cy < 123 - 22
    im0, im1 = sq["im0"].copy(), sq["im1"].copy()
    (im0 if in_reference else im1)[cy - 22:cy + 22, cx - 22:cx + 22] = value
    extra = np.array([[cx + 22.0, cy + 3.5], [cx - 4.25, cy - 22.0]], F32)           # windows half inside the patch
    pts = np.concatenate([sq["pts"], extra])
    c = _case(im0, im1, pts, guess=pts + F32(0.3), cfg=dict(max_level=max_level))
    # point 0's level-0 window at the guess (22 x 22 pixels: 21 + the bilinear neighbour) is constant
    ox, oy = int(np.floor(c["guess"][0, 0] - 10)), int(np.floor(c["guess"][0, 1] - 10))
    win = (im0 if in_reference else im1)[oy:oy + 22, ox:ox + 22]
    assert win.shape == (22, 22) and np.all(win == value)
    return c


def _vet_dead(c, value, in_reference):
    lk, (xy, st, good, ssim) = run_oracle(c)
    if value == 0 and not in_reference:
        # meanJ2 = 0: alpha, beta and the step are not finite; the next window origin is outside the image
        assert st[0] == LK.OUT_IMAGE_BOUNDARIES and np.all(np.isnan(xy[0]))
    elif value == 0:
        assert lk.meanI2[0][0] == 0 and st[0] == LK.BAD_FEATURE                   # alpha = 0, A = 0: min eigenvalue
    else:
        assert st[0] != 0 and np.all(np.isfinite(xy[0]))                            # nothing to hold on to, nothing undefined
    assert good >= len(st) - 6 and (st[1:-2] == 0).sum() >= len(st) - 8            # the points outside the patch track


# ---- gates ---------------------------------------------------------------------------------------------------------------------------------
GW, GH = 161, 123


def _dim(dim0, level):
    for _ in range(level):
        dim0 = (dim0 + 1) // 2
    return dim0


def _gate_probes(axis, max_level):
    """reference points whose window-origin floor at the TOP level is at the set-reference and track bounds and one either side (integer
    and x.5 level coordinates), with the guess on the point; then interior-clamped reference points with GUESSES whose floor at the top
    level is at the track bounds, and at level 0 at the SSIM bounds.  The other coordinate sits mid-image.  (max_level 0 probes level 0,
    max_level 1 level 1.)"""
    dim0, other = (GW, 61.25) if axis == 0 else (GH, 80.75)
    pts, guess, tag = [], [], []

    def put(p, g, t):
        a, b = ([p, other], [g, other]) if axis == 0 else ([other, p], [other, g])
        pts.append(a); guess.append(b); tag.append(t)
    top, dim = max_level, _dim(dim0, max_level)
    for f in (-12, -11, -10, -9, dim - 13, dim - 12, dim - 11, dim - 10, dim - 9):
        for frac in (0.0, 0.5):
            v = (f + 10 + frac) * (1 << top)
            put(v, v, ("ref", top, f))
    floors = [(-12, "trk"), (-11, "trk"), (-10, "trk"), (dim - 12, "trk"), (dim - 11, "trk"), (dim - 10, "trk")]
    if top == 0:
        floors += [(dim - 23, "ssim"), (dim - 22, "ssim"), (dim - 21, "ssim")]
    for f, kind in floors:
        for frac in (0.0, 0.5):
            g = (f + 10 + frac) * (1 << top)
            put(float(np.clip(g, 14.0, dim0 - 15.0)), g, (kind, top, f))
    return np.array(pts, F32), np.array(guess, F32), tag


def _gates(axis, max_level):
    sq = pair(GW, GH, 5)
    pts, guess, tag = _gate_probes(axis, max_level)
    # (no probe can end as a good track: all lie within 12 px of the border; four interior points keep the case honest about that)
    pts, guess = np.concatenate([pts, sq["pts"][:4]]), np.concatenate([guess, sq["pts"][:4] + F32(0.7)])
    tag = tag + [("in", 0, 0)] * 4
    c = _case(sq["im0"], sq["im0"], pts, guess=guess, cfg=dict(max_level=max_level))      # tracked against itself: the answer is the point
    c["tag"] = tag
    return c


def _vet_gates(c, axis):
    lk, (xy, st, good, ssim) = run_oracle(c)
    dim0, tag, top = (GW, GH)[axis], c["tag"], c["cfg"]["max_level"]
    dim = _dim(dim0, top)
    # set-reference: a template exactly when -10 <= floor < dim - 10.
    # track, previous point: the level is entered (a window of the tracked image is sampled) exactly when there is a template and
    # -11 <= floor < dim - 11.  Its lower bound lies below set-reference's, so there it is the missing template that decides (the
    # outcome is the same); at the upper bound floor = dim - 11 has a template and is refused by the track gate, dim - 12 is sampled.
    # A refused probe is never updated at any level: it ends OUT_IMAGE_BOUNDARIES with the bits it went in with.
    seen = {}
    for i, t in enumerate(tag):
        if t[0] == "ref":
            f = t[2]
            has = lk.Iref[top][i] is not None
            assert has == (-10 <= f < dim - 10), (i, t)
            assert bool(lk.last_sampled[i, top]) == (-10 <= f < dim - 11), (i, t)
            if not lk.last_sampled[i].any():
                assert st[i] == LK.OUT_IMAGE_BOUNDARIES and np.array_equal(xy[i], c["guess"][i]), (i, t)
            seen[f] = (has, bool(lk.last_sampled[i, top]))
    assert seen[-11] == (False, False) and seen[-10] == (True, True)
    assert seen[dim - 12] == (True, True) and seen[dim - 11] == (True, False) and seen[dim - 10] == (False, False)
    # track, iterate: a guess outside is never sampled at the top level, is OUT_IMAGE_BOUNDARIES and comes back as it went in (scaled
    # down and up by powers of two); a guess inside is sampled
    sides = set()
    for i, t in enumerate(tag):
        if t[0] == "trk":
            inside = -11 <= t[2] < dim - 11
            assert bool(lk.last_sampled[i, top]) == inside, (i, t)
            if not inside:
                assert st[i] == LK.OUT_IMAGE_BOUNDARIES and np.array_equal(xy[i], c["guess"][i]), (i, t)
            sides.add((t[2] < 0, inside))
    assert sides == {(True, True), (True, False), (False, True), (False, False)}
    if top == 0:
        fl = sorted({t[2] - (dim0 - 22) for t in tag if t[0] == "ssim"})
        assert fl == [-1, 0, 1]                                                     # GUESSES either side of the SSIM bound and on it
    assert np.all(st[-4:] == 0) and (st == LK.OUT_IMAGE_BOUNDARIES).sum() > 4


# ---- the SSIM gate ---------------------------------------------------------------------------------------------------------------------------
def ssim_decided(lk, st):
    """the points that left the iteration usable and were refused by the SSIM gate's position test"""
    return np.isin(lk.last_track_status, USABLE) & (st == LK.OUT_IMAGE_BOUNDARIES)


def _ssim_nonfinite():
    """the black patch of the dead-window cases with max_level 0 and ONE iteration: the iteration ends with a NaN position and a usable
    status, and it is the SSIM gate's position test that refuses the point"""
    c = _dead(0, False, 0)
    c["cfg"] = dict(c["cfg"], max_iters=1)
    return c


def _vet_ssim_nonfinite(c):
    lk, (xy, st, good, ssim) = run_oracle(c)
    d = ssim_decided(lk, st)
    assert d[0] and np.all(np.isnan(lk.last_track_xy[0])) and np.all(np.isnan(xy[0])) and np.isnan(ssim[0])
    assert np.all(np.isnan(lk.last_track_xy[d]).any(axis=1))                      # (no finite position is refused there: see below)
    assert good >= len(st) - 6


def _ssim_border():
    """reference points whose tracks end within a pixel or two of x = w - 12 and y = h - 12, the largest positions the iteration lets
    through: the SSIM gate's inner side of its upper bound (window origin w - 23, h - 23)"""
    sq = pair(GW, GH, 5)
    xs = [(GW - 12.1 - 0.15 * k, 24.0 + 5.0 * k) for k in range(18)]
    ys = [(28.0 + 7.0 * k, GH - 12.1 - 0.15 * k) for k in range(18)]
    pts = np.array(xs + ys, F32)
    return _case(sq["im0"], sq["im0"], pts, guess=pts + F32([0.2, 0.2]), cfg=dict(max_level=0))


def _vet_ssim_border(c):
    lk, (xy, st, good, ssim) = run_oracle(c)
    reached = np.isfinite(ssim)
    o = np.floor(lk.last_track_xy[reached] - F32(10)).astype(int)
    assert (o[:, 0] == GW - 23).sum() >= 3 and (o[:, 1] == GH - 23).sum() >= 3      # the last origin inside the bound, on both axes
    assert not ssim_decided(lk, st).any()


def vet_ssim_gate_reach():
    """The SSIM gate's position test, -11 <= o < dim - 22, decides no FINITE position, and this is checked on every case of the table.
    A point reaches the gate usable only after an update at level 0, and every updated position has passed 12 <= x < dim - 12, i.e.
    2 <= o < dim - 22.  The one later change is the half step back of the oscillation exit, x - delta / 2 with the previous delta equal
    to -delta within 0.01: a point between this iterate and the previous one, both of which passed the same test.  So the gate's bounds
    are held on their inside (ssim_border) and on the non-finite side (ssim_nonfinite, the dead-black cases); an implementation with
    another finite bound there cannot be told apart by any input."""
    n_nonfinite = 0
    for n in NAMES:
        c = case(n)
        lk, (xy, st, good, ssim) = _oracle_full(n)
        h, w = c["im0"].shape
        us = np.isin(lk.last_track_status, USABLE)
        p = lk.last_track_xy[us]
        fin = np.isfinite(p).all(axis=1)
        o = np.floor(p[fin] - F32(10))
        assert np.all((o >= 2) & (o < np.array([w - 22, h - 22]))), n
        assert np.all(st[us][~fin] == LK.OUT_IMAGE_BOUNDARIES), n
        assert np.all(st[us][fin] != LK.OUT_IMAGE_BOUNDARIES), n
        n_nonfinite += int((~fin).sum())
    assert n_nonfinite >= 1


# ---- bad numbers ---------------------------------------------------------------------------------------------------------------------------
BAD_VALUES = (np.nan, np.inf, -np.inf, 1e30, -1e30)


def _bad_numbers(initial_flow):
    sq = pair(161, 123, 5)
    pts = np.concatenate([sq["pts"], sq["pts"][:2]])
    n = len(pts)
    assert n >= 13
    guess = (pts + F32(0.7)).astype(F32)
    for k, v in enumerate(BAD_VALUES):
        guess[k, 0] = v                                                            # as x of points 0..4
        guess[5 + k, 1] = v                                                        # as y of points 5..9
    pts[n - 2, 0] = np.nan                                                         # a NaN reference point, x and y
    pts[n - 1, 1] = np.nan
    return _case(sq["im0"], sq["im1"], pts, guess=guess, cfg=dict(max_level=2), initial_flow=initial_flow)


def _vet_bad_numbers(c):
    lk, (xy, st, good, ssim) = run_oracle(c)
    n = len(st)
    assert all(lk.Iref[l][i] is None for l in range(3) for i in (n - 2, n - 1)) and np.all(st[n - 2:] == LK.OUT_IMAGE_BOUNDARIES)
    if c["initial_flow"]:
        assert np.all(st[:10] == LK.OUT_IMAGE_BOUNDARIES) and np.all(st[10:n - 2] == 0)
        assert np.array_equal(xy[:10], c["guess"][:10], equal_nan=True)            # x 2^-2, x 2, x 2: the guess's own bits
    else:
        assert np.all(st[:n - 2] == 0) and np.all(np.isfinite(xy[:n - 2]))          # the guess is not read


# ---- configurations, statuses, a mask ------------------------------------------------------------------------------------------------------
CONFIGS = {"ref_default": (3, 30, 0.01, 1e-4), "l0": (0, 10, 1e-4, 1e-4), "l1_one_iter": (1, 1, 1e-4, 1e-3), "l2_three_iters": (2, 3, 1e-4, 1e-4)}


def _config(key, masked=False):
    """the 161 x 123 pair and a grid of hand-placed points, with every input status code (i mod 6) and, on every seventh point, a guess
    9 px off (the drift cap and the SSIM gate reject some of those)"""
    ml, it, eps, me = CONFIGS[key]
    sq = pair(161, 123, 5)
    pts = np.concatenate([sq["pts"], _grid((24, 52, 80, 108, 136), (22, 48, 74, 100), 17)])
    status = (np.arange(len(pts)) % 6).astype(np.int32)
    guess = (pts + F32(0.7)).astype(F32)
    guess[::7] += F32([9.0, -4.5])
    mask = None
    if masked:
        mask = np.full(sq["im0"].shape, 255, np.uint8)
        mask[40:70, 60:110] = 0
    return _case(sq["im0"], sq["im1"], pts, guess=guess, status=status, mask=mask, cfg=dict(max_level=ml, max_iters=it, epsilon=eps, min_eig=me))


def _vet_config(c):
    lk, (xy, st, good, ssim) = run_oracle(c)
    assert set(c["status"].tolist()) == set(range(6))
    un = ~np.isin(c["status"], USABLE)
    assert np.array_equal(st[un], c["status"][un]) and np.array_equal(xy[un], c["guess"][un])
    assert good > 5
    if c["mask"] is not None:
        _, r2 = run_oracle(dict(c, mask=None))
        full = LK.LucasKanadeOracle(21, **c["cfg"])
        full.set_reference(c["im0"], c["pts"])
        dropped = sum(1 for l in range(len(lk.Iref)) for a, b in zip(lk.Iref[l], full.Iref[l]) if a is None and b is not None)
        assert dropped > 0 and not np.array_equal(st, r2[1])                        # the mask takes templates away and points with them


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
def _far_guess():
    """max_level 0 with every guess 9 px off: the drift cap (BAD), the SSIM gate (BAD_FEATURE) and good tracks side by side"""
    sq = pair(161, 123, 5)
    return _case(sq["im0"], sq["im1"], sq["pts"], guess=sq["pts"] + F32([9.0, -4.5]), cfg=dict(max_level=0))


def _vet_far_guess(c):
    _, (xy, st, good, ssim) = run_oracle(c)
    assert (st == 0).sum() >= 3 and (st == LK.BAD).sum() >= 2 and (st == LK.BAD_FEATURE).sum() >= 3
    assert np.array_equal(xy[st == LK.BAD], c["guess"][st == LK.BAD])              # the drift cap puts the start position back


_P23 = _grid((3, 7, 11, 15, 19), (4, 11, 18), 3)
_P97 = _grid((14, 23, 32, 41, 50, 59, 68, 77), (14, 22, 30), 4)

BUILDERS = {
    "short_161x123": (lambda: _short(161, 123, 5), _vet_short),
    "short_97x45": (lambda: _short(97, 45, 6, _P97), _vet_short),
    "short_23x22": (lambda: _short(23, 22, 7, _P23), _vet_short),
    "odd_161x123_l2": (lambda: _short(161, 123, 5, cfg=dict(max_level=2)), _vet_full),
    "odd_175x177_l3": (lambda: _short(175, 177, 7, cfg=dict(max_level=3)), _vet_full),
    "far_guess_l0": (_far_guess, _vet_far_guess),
    "ssim_nonfinite_l0": (_ssim_nonfinite, _vet_ssim_nonfinite),
    "ssim_border_l0": (_ssim_border, _vet_ssim_border),
    "bad_numbers_flow": (lambda: _bad_numbers(True), _vet_bad_numbers),
    "bad_numbers_noflow": (lambda: _bad_numbers(False), _vet_bad_numbers),
    "cfg_ref_default": (lambda: _config("ref_default"), _vet_config),
    "cfg_l0": (lambda: _config("l0"), _vet_config),
    "cfg_l1_one_iter": (lambda: _config("l1_one_iter"), _vet_config),
    "cfg_l2_three_iters": (lambda: _config("l2_three_iters"), _vet_config),
    "cfg_l2_three_iters_mask": (lambda: _config("l2_three_iters", masked=True), _vet_config),
}
for _ml in (2, 0):
    for _tag, _v, _ref in (("black", 0, False), ("white", 255, False), ("grey", 128, False), ("black_ref", 0, True)):
        BUILDERS["dead_%s_l%d" % (_tag, _ml)] = (lambda v=_v, r=_ref, m=_ml: _dead(v, r, m), lambda c, v=_v, r=_ref: _vet_dead(c, v, r))
for _ml in (0, 1):
    for _ax in (0, 1):
        BUILDERS["gates_%s_l%d" % ("xy"[_ax], _ml)] = (lambda a=_ax, m=_ml: _gates(a, m), lambda c, a=_ax: _vet_gates(c, a))

NAMES = sorted(BUILDERS)
SHORT = [n for n in NAMES if n.startswith("short_")]
UNMASKED = [n for n in NAMES if not n.endswith("_mask")]


@functools.lru_cache(maxsize=None)
def case(name):
    build, vet = BUILDERS[name]
    c = build()
    vet(c)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _oracle_full(name):
    return run_oracle(case(name))


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(templates in klt_get_templates layout, (xy, status, n_good, ssim)) of the NumPy oracle on case(name)"""
    lk, r = _oracle_full(name)
    t = oracle_templates(lk)
    for v in list(t.values()) + [r[0], r[1], r[3]]:
        v.setflags(write=False)
    return t, r


def vet_table():
    """the table as a whole: every status code 0-5 is PRODUCED by the tracker (on a point that went in usable) or kept by it"""
    out = set()
    for n in NAMES:
        c, (_, r) = case(n), oracle(n)
        out |= set(r[1][np.isin(c["status"], USABLE)].tolist())
    assert out == set(range(6)), out
