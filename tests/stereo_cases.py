"""Inputs shared by the tests of the resident stereo pair (tests/test_front_stereo_host_cpu.py, tests/test_gpu_front_stereo.py) and of the
stereo start past one chunk, one trip and one tie (tests/test_stereo_cases_cpu.py, tests/test_stereo_init_oracle_cpu.py,
tests/test_gpu_stereo.py, tests/test_gpu_stereo_init.py): each scene is built once, with its oracle result, and handed out read-only.

The matchers read GREY bytes.  A scene's raw frames are made so that the front end's grey conversion gives the scene's images back: one
channel is copied, and three equal channels g give (g * 32768 + 2^14) >> 15 = g."""
import functools

import numpy as np

import eval_oracle as E
import nrs_synth as S
import stereo_init_oracle as SO

F32 = np.float32
PRM = np.array([383.19, 383.05, 155.97, 124.34], F32)
BF_PATTERN, BF_INIT = 2000.0, 400.0
PW, PH, PDISP = 64, 48, 5                                          # the pattern scene: the matcher refuses anything below 32 a side


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def pattern_scene():
    """64 x 48.  Right eye: the left eye shifted by PDISP px in the rows above 21, a second, unrelated texture below -- so a keypoint whose
    template lies in the upper part is matched (status 0) and one in the lower part is not (status 3, LOW_CORRELATION).  17 keypoints (one
    more than the matcher's group of 16, so the padding to the group size is exercised): 0 matched (it is the n = 1 case), then matched and
    unmatched ones with integer and fractional coordinates, one within 7 px of the top border (OUT_OF_BOUNDS) and one whose template holds
    a 255 pixel (SATURATED)."""
    rng = np.random.default_rng(23)
    tex = np.clip(np.rint(S._texture(PH, PW + PDISP, rng, 0)), 0, 250).astype(np.uint8)
    other = np.clip(np.rint(S._texture(PH, PW, np.random.default_rng(24), 0)), 0, 250).astype(np.uint8)
    left = tex[:, :PW].copy()
    right = np.ascontiguousarray(tex[:, PDISP:PDISP + PW])          # the left pixel (x, y) is found at (x - PDISP, y)
    right[21:] = other[21:]
    up = [(32.0, 10.0), (40.0, 12.0), (35.25, 11.5), (44.0, 9.0), (29.5, 13.0), (38.75, 10.0), (42.0, 13.0), (33.0, 13.0)]       # rows <= 20
    low = [(30.0, 28.0), (36.5, 28.0), (41.0, 28.0), (27.0, 28.0), (44.0, 28.0), (34.0, 28.0), (39.25, 28.0)]                   # rows 21 .. 35
    xy = np.array(up + low + [(30.0, 5.0), (37.0, 7.0)], F32)      # ... the border keypoint and the saturated one
    left[2, 35] = 255                                              # inside the last keypoint's template (rows 0 .. 14, columns 30 .. 44) only
    assert len(xy) == 17
    sc = dict(left=left, right=right, xy=xy)
    for n in (0, 1, 17):
        sc["oracle%d" % n] = E.stereo_match_pattern(PRM, BF_PATTERN, left, right, xy[:n])
    return _freeze(sc)


@functools.lru_cache(maxsize=None)
def init_scene():
    """the smallest scene of tests/test_gpu_stereo_init.py (96 x 64: a band of disparity 0 and one of disparity 8, z_min exactly on the depth
    of disparity 8.5), with raw frames of three equal channels.  eps = 1, min_points = 1 cut its nine gated points into three clusters and
    a noise point, so every code 0 .. 3 occurs (tests/test_front_stereo_host_cpu.py checks that with the oracle alone)"""
    p = S.make_stereo_pair((96, 64), 3, (0, 8), 40, row_pad=0)
    p["opts"] = dict(bf=BF_INIT, z_min=float(F32(BF_INIT) / F32(8.5)), z_max=60.0, eps=1.0, min_points=1)
    p["oracle"] = SO.init_stereo(PRM, p["left"], p["right"], p["xy"], **p["opts"])
    p["raw_left"] = np.ascontiguousarray(np.repeat(p["left"][:, :, None], 3, 2))
    p["raw_right"] = np.ascontiguousarray(np.repeat(p["right"][:, :, None], 3, 2))
    return _freeze(p)


# ---- the large clustering cases (nrs_synth.make_large_cluster_cases): labels once per process
LARGE_CLUSTER_CASES = S.make_large_cluster_cases()
BRUTE_FORCE_MAX_POINTS = 4160          # dbscan3d_fixed_point sweeps once per hop of the longest chain: held to the oracle up to this size only


def cluster_case(name):
    return next(c for c in LARGE_CLUSTER_CASES if c["name"] == name)


@functools.lru_cache(maxsize=None)
def cluster_expected(name, check=False):
    """-> {True / False: what stereo_init_oracle.dbscan3d returns with noise competing / not}: the sequential pass runs once (the raw labels
    do not depend on the ranking).  check: also assert the case's `holds` on the neighbour matrix, which is not kept (256 MiB at 16384)"""
    c = cluster_case(name)
    nb = SO.neighbours(c["xyz"], c["eps"])
    raw, core = SO.dbscan3d_raw(c["xyz"], c["eps"], c["min_points"], nb=nb)
    if check:
        c["holds"](c, raw, core, nb)
    raw.setflags(write=False)
    return {nc: (raw,) + SO.rank_labels(raw, nc) for nc in (True, False)}


# ---- the matcher's ties and near-ties.  A workgroup of the matrix-core form owns 64 x 32 search positions, one of the plain form 16 x 16
MF_TILE, PL_TILE = (64, 32), (16, 16)
LATTICE = np.array([[60, 200], [140, 90]], np.uint8)


def _keypoints(cells, fracs):
    return np.array([(ox + 7 + fracs[k % len(fracs)][0], oy + 7 + fracs[k % len(fracs)][1]) for k, (ox, oy) in enumerate(cells)], F32)


def _cells(xy):
    return sorted({(int(F32(x - F32(7))), int(F32(y - F32(7)))) for x, y in xy})


@functools.lru_cache(maxsize=None)
def lattice_scene(second_workgroup):
    """Both images repeat LATTICE with period 2 in x and y, so a template scores exactly 1.0 (TI = T2 = I2) at every search position of
    its own parity: ties within a lane's registers, between lane groups, waves, rows and workgroups.  20 keypoints over the four phases.
      second_workgroup False   96 x 64 (2 x 2 workgroups): the winner is the first position of the first workgroup
      second_workgroup True    160 x 96 (3 x 3): the right image's rows 0 .. 39 and columns 0 .. 69 are noise, so only positions with
                               px >= 70 and py >= 40 see the lattice alone: the first tie lies in the second workgroup in x AND y (a
                               70 x 40 corner alone would leave clean windows in row 0 from px = 70 on), later ones in workgroups (2, 1),
                               (1, 2) and (2, 2)"""
    w, h = (160, 96) if second_workgroup else (96, 64)
    img = LATTICE[np.ix_(np.arange(h) % 2, np.arange(w) % 2)]
    left, right = img.copy(), img.copy()
    if second_workgroup:
        noise = np.random.default_rng(71).integers(0, 251, (h, w)).astype(np.uint8)
        right[:40, :] = noise[:40, :]
        right[:, :70] = noise[:, :70]
    rng = np.random.default_rng(72)
    cells = [(int(rng.integers(10, (w - 27) // 2)) * 2 + px, int(rng.integers(0, (h - 27) // 2)) * 2 + py) for k in range(5) for px in (0, 1)
             for py in (0, 1)]
    xy = _keypoints(cells, [(0.0, 0.0), (0.25, 0.5), (0.5, 0.0), (0.75, 0.75)])
    sc = dict(wh=(w, h), left=left, right=right, xy=xy, first_tile=(1, 1) if second_workgroup else (0, 0))
    sc["oracle"] = E.stereo_match_pattern(PRM, BF_PATTERN, left, right, xy)
    return _freeze(sc)


def lattice_holds(sc):
    """from the oracle's score maps: the maximum is exactly 1.0, attained in several workgroups (and 16 x 16 tiles) in x and in y, first in
    workgroup sc["first_tile"]; every one of the four phases occurs"""
    maps = E.ScoreMaps(sc["left"], sc["right"])
    cells = _cells(sc["xy"])
    assert {(ox % 2, oy % 2) for ox, oy in cells} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for ox, oy in cells:
        s = maps.map(ox, oy)
        ys, xs = np.nonzero(s == s.max())
        assert s.max() == 1.0 and len(xs) > 50
        assert (xs[0] // MF_TILE[0], ys[0] // MF_TILE[1]) == sc["first_tile"], (ox, oy, xs[0], ys[0])
        assert (xs[0] % 2, ys[0] % 2) == (ox % 2, oy % 2)
        for tile in (MF_TILE, PL_TILE):
            assert len(set(xs // tile[0])) >= 2 and len(set(ys // tile[1])) >= 2
        lane_regs = {(x // 4, y) for x, y in zip(xs, ys)}            # the four registers of a lane hold px = 4 g .. 4 g + 3 of one row
        assert len(lane_regs) < len(xs)                             # ... so two ties share a lane's registers
    st = sc["oracle"][1]
    assert np.isin(st, (E.OK, E.ZERO_DISPARITY)).all() and (st == E.OK).sum() >= 16       # (a keypoint 7 px right of the winner has disparity 0)


NEAR_TIES = {"later_in_one_tile": (3, 19, 19), "later_across_tiles": (4, 36, 36), "earlier_in_one_tile": (3, 19, 3)}


@functools.lru_cache(maxsize=None)
def near_tie_scene(name):
    """96 x 64, the right image periodic in y with period 16 (a random texture), left = right.  NEAR_TIES[name] = (row of the first copy,
    row of the copy that holds the changed pixel, row the templates are cut from): ONE pixel, in the middle of the window (30, changed
    row), is raised by one grey level, so the windows at the two rows differ in that pixel alone and the templates equal one of them.
    With sum T^2 about 4e6 the two scores differ by about 1 / (2 sum T^2) ~ 1e-7 relative: the fp32 screen of the matrix-core form cannot
    tell them apart, the fp64 score must."""
    first, changed, cut = NEAR_TIES[name]
    w, h = 96, 64
    base = np.random.default_rng(73).integers(20, 231, (16, w)).astype(np.uint8)
    right = base[np.arange(h) % 16].copy()
    right[changed + 7, 37] += 1
    left = right.copy()
    xy = _keypoints([(px, cut) for px in (23, 30, 33, 37)], [(0.5, 0.0), (0.25, 0.5)])      # every window at these px holds column 37
    sc = dict(wh=(w, h), left=left, right=right, xy=xy, rows=(first, changed, cut))
    sc["oracle"] = E.stereo_match_pattern(PRM, BF_PATTERN, left, right, xy)
    return _freeze(sc)


def near_tie_holds(sc):
    """-> the largest relative gap.  From the oracle's score maps, per template: the two best DISTINCT scores s1 > s2 lie within 1e-5
    (relative) of each other at the same px, s1 (exactly 1.0) at the row the template is cut from and s2 first at the other row of the pair,
    in one 32-row tile or across two as the scene's name says"""
    maps = E.ScoreMaps(sc["left"], sc["right"])
    first, changed, cut = sc["rows"]
    other = changed if cut == first else first
    worst = 0.0
    for ox, oy in _cells(sc["xy"]):
        s = maps.map(ox, oy)
        v = np.unique(s)
        s1, s2 = v[-1], v[-2]
        gap = (s1 - s2) / s1
        assert s1 == 1.0 and 0 < gap < 1e-5, gap
        y1, x1 = [int(a[0]) for a in np.nonzero(s == s1)]
        y2, x2 = [int(a[0]) for a in np.nonzero(s == s2)]
        assert (x1, y1) == (ox, cut) and (x2, y2) == (ox, other), ((x1, y1), (x2, y2))
        assert (y1 // MF_TILE[1] == y2 // MF_TILE[1]) == (changed // MF_TILE[1] == first // MF_TILE[1])
        worst = max(worst, gap)
    assert np.all(sc["oracle"][1] == E.OK) and np.array_equal(sc["oracle"][3][:, 1], np.full(len(sc["xy"]), cut))
    return worst


# ---- nrs_init_stereo with three chunks of keypoints
@functools.lru_cache(maxsize=None)
def init_scene_three_chunks():
    """The 96 x 64 scene of tests/test_gpu_stereo_init.py (a band of disparity 0 above one of disparity 8, bf 400, z_min EXACTLY the depth of
    disparity 8.5) with 2093 keypoints: a few dozen template cells x sub-pixel fractions of 1 / 64 in x, which move the disparity and so the
    depth through the gate inside every cell.  In the lower band a fraction below 0.5 passes the gate, 0.5 lies on z_min (excluded), above
    it below z_min; the upper band's fractional keypoints lie far beyond z_max and its integer ones have disparity zero.  Two groups of cells
    (around x = 38 and x = 68) give two clusters of different size, three lone keypoints of a third cell are noise.  The scene's rejected
    kinds (the five boundary keypoints, the saturated template, zero disparity) are repeated a hundred times each, and everything is
    ordered by a seeded permutation."""
    p = S.make_stereo_pair((96, 64), 3, (0, 8), 40, row_pad=0)
    rng = np.random.default_rng(74)
    g1 = [(ox, oy) for ox in (30, 31, 32, 33) for oy in (32, 34, 36)]
    g2 = [(ox, oy) for ox in (60, 61, 62) for oy in (33, 35)]
    up = [(ox, oy) for ox in (30, 50) for oy in (2, 6, 10)]
    kinds = list(p["kind"])
    sat = p["xy"][kinds.index("saturated")]
    bounds = p["xy"][[i for i, k in enumerate(kinds) if k == "boundary"]]

    def draw(cells, count, fx_lo, fx_hi):
        c = np.array(cells)[rng.integers(0, len(cells), count)]
        return np.stack([c[:, 0] + 7 + rng.integers(fx_lo, fx_hi, count) / 64.0, c[:, 1] + 7 + rng.integers(0, 4, count) / 4.0], 1)

    parts = [draw(g1, 860, 0, 32), draw(g2, 500, 0, 32),                      # inside the gate: the two clusters
             draw(g1 + g2, 250, 33, 64), draw(g1 + g2, 30, 32, 33),           # below z_min; exactly on it
             draw(up, 150, 16, 64), draw(up, 100, 0, 1),                      # far beyond z_max; zero disparity
             np.tile(sat, (100, 1)) + np.stack([rng.integers(0, 4, 100) / 8.0, np.zeros(100)], 1),
             bounds[np.arange(100) % len(bounds)],
             np.array([(45 + 7 + f, 34 + 7) for f in (0.0, 0.1875, 0.375)])]   # noise: alone in x, 1 apart in z
    xy = np.concatenate(parts).astype(F32)
    xy = xy[rng.permutation(len(xy))]
    p = dict(wh=p["wh"], left=p["left"], right=p["right"], xy=xy)
    p["opts"] = dict(bf=BF_INIT, z_min=float(F32(BF_INIT) / F32(8.5)), z_max=60.0, eps=0.3, min_points=3)
    p["oracle"] = {nc: SO.init_stereo(PRM, p["left"], p["right"], xy, noise_competes=nc, **p["opts"]) for nc in (1, 0)}
    for o in p["oracle"].values():
        _freeze(o)
    return _freeze(p)


def init_three_chunks_holds(p):
    """what the scene is made for, from the oracle's result alone"""
    o = p["oracle"][1]
    n = len(p["xy"])
    assert 2 * 1024 < n <= 3 * 1024
    chunk = np.arange(n) // 1024
    for c in range(3):
        assert set(o["code"][chunk == c]) == {0, 1, 2, 3}, c
        assert {E.OUT_OF_BOUNDS, E.SATURATED, E.ZERO_DISPARITY}.issubset(set(o["match_status"][chunk == c])), c
    counts = (o["n_matched"], o["n_gated"], o["n_selected"])
    assert len(set(counts)) == 3 and all(v % 1024 for v in counts), counts
    assert o["n_clusters"] >= 2 and o["n_noise"] > 0 and o["verdict"] == 0
    assert set(chunk[o["selected"]]) == {0, 1, 2}
    # the select kernel loops over the GATED points in chunks of 1024: its second trip must hold selected points, and the rows of the
    # clustering (ceil(n / 64) words) must be wider than the words in use (ceil(n_gated / 64)), both large
    gated = np.nonzero(o["label"] != -2)[0]
    assert o["n_gated"] > 1024 and (o["label"][gated[1024:]] == 0).any() and (o["label"][gated[:1024]] == 0).any()
    assert (n + 63) // 64 > (o["n_gated"] + 63) // 64 > 16
    z = o["xyz"][:, 2]
    on_min = (o["match_status"] == E.OK) & (z == F32(p["opts"]["z_min"]))
    assert on_min.any() and np.all(o["code"][on_min] == 2)
    with np.errstate(invalid="ignore"):
        assert ((o["code"] == 2) & (z < F32(p["opts"]["z_min"]))).any() and ((o["code"] == 2) & (z > F32(p["opts"]["z_max"]))).any()
    o0 = p["oracle"][0]
    assert not np.array_equal(o0["label"], o["label"]) or o["n_noise"] < o["n_selected"]
    return counts
