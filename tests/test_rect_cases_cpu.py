"""CPU: every designed camera of tests/rect_cases.py shows, ON THE ORACLE ALONE (tests/rect_oracle.py), what it is made for -- so that the
GPU test, which holds the device to the oracle on the same cases, covers the identity, the blend, the rounding ties, every fraction index,
every way a pixel can lose taps to the border, the rational model and the non-finite rule -- and the new entry points are declared,
listed and exported."""
import inspect
import os
import re

import numpy as np
import pytest

import rect_cases as RC
import rect_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["nrs_front_rectify_configure", "nrs_front_rectify_maps", "nrs_front_process_stereo_raw"]
F32 = np.float32


def _fixed(name):
    return [RO.fix(mx, my) for mx, my in RC.maps(name)]


def test_identity_gives_the_input_back():
    c = RC.cases()["identity"]
    assert (c["dst_w"], c["dst_h"]) == (c["src_w"], c["src_h"])
    v, u = np.mgrid[0:c["dst_h"], 0:c["dst_w"]]
    for (mx, my), (ix, iy, fx, fy, finite) in zip(RC.maps("identity"), _fixed("identity")):
        assert np.array_equal(mx, u.astype(F32)) and np.array_equal(my, v.astype(F32))       # exactly: powers of two throughout
        assert finite.all() and not fx.any() and not fy.any() and np.array_equal(ix, u) and np.array_equal(iy, v)
    for ch in (1, 3, 4):
        for raw, rect in zip(RC.raw_pair("identity", ch), RC.rectified_pair("identity", ch)):
            assert np.array_equal(raw, rect)


def test_half_pixel_is_the_rounded_mean_of_two_neighbours():
    c = RC.cases()["half_pixel"]
    (lx, ly), (rx, ry) = RC.maps("half_pixel")
    v, u = np.mgrid[0:c["dst_h"], 0:c["dst_w"]]
    assert np.array_equal(lx, (u + 0.5).astype(F32)) and np.array_equal(ly, v.astype(F32))
    assert np.array_equal(rx, u.astype(F32)) and np.array_equal(ry, (v + 0.5).astype(F32))
    row = np.array([0, 255, 255, 1, 2, 4, 7, 250, 251, 3, 0, 0, 9, 128, 127, 64] * 4, np.int64)          # a hand-written row of 64
    src = np.tile(row.astype(np.uint8), (c["src_h"], 1))
    out = RO.remap(src, lx, ly)
    want = np.zeros(c["dst_w"], np.int64)
    want[:63] = (row[:-1] + row[1:] + 1) >> 1
    want[63] = (row[63] + 0 + 1) >> 1                               # the right neighbour is outside: 0
    assert want[0] == 128 and want[1] == 255 and want[3] == 2 and want[63] == 32 and not want[64:].any()
    assert np.array_equal(out[:c["src_h"]], np.tile(want, (c["src_h"], 1))) and not out[c["src_h"]:].any()
    col = np.tile(row[:c["src_h"], None].astype(np.uint8), (1, c["src_w"]))                                # ... and a column, for the right eye
    out = RO.remap(col, rx, ry)
    want = np.zeros(c["dst_h"], np.int64)
    want[:47] = (row[:47] + row[1:48] + 1) >> 1
    want[47] = (row[47] + 1) >> 1
    assert np.array_equal(out[:, :c["src_w"]], np.tile(want[:, None], (1, c["src_w"]))) and not out[:, c["src_w"]:].any()


def test_ties_occur_and_round_to_even():
    for (mx, my), (ix, iy, fx, fy, _), (want_fx, want_fy) in zip(RC.maps("ties"), _fixed("ties"), ((0, 2), (2, 0))):
        for m in (mx, my):
            t = (m * F32(32)).astype(F32).astype(np.float64)
            assert (np.abs(t - np.floor(t)) == 0.5).all()           # every product is an exact tie
        # 32 u + 0.5 -> 32 u (half up or away from zero: fraction 1), 32 u + 1.5 -> 32 u + 2 (truncation: fraction 1)
        assert (fx == want_fx).all() and (fy == want_fy).all()
        v, u = np.mgrid[0:mx.shape[0], 0:mx.shape[1]]
        assert np.array_equal(ix, u) and np.array_equal(iy, v)


@pytest.mark.parametrize("name", ["rot_dist", "border", "rational"])
def test_every_fraction_index_occurs_on_both_axes(name):
    for ix, iy, fx, fy, finite in _fixed(name):
        assert finite.all()
        assert set(np.unique(fx)) == set(range(32)) and set(np.unique(fy)) == set(range(32)), name


def test_rot_dist_is_a_rotation_with_distortion():
    c = RC.cases()["rot_dist"]
    for e in ("left", "right"):
        R = np.asarray(c[e]["R"])
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and abs(R[0, 1]) > 0.01 and np.count_nonzero(c[e]["dist"]) >= 4
        plain = RO.build_map(dict(c[e], dist=()), c["dst_w"], c["dst_h"])
        assert np.abs(plain[0] - RC.maps("rot_dist")[e == "right"][0]).max() > 1.0             # the distortion moves pixels by more than one


def test_border_leaves_the_source_on_all_four_sides():
    """A pixel's four taps form a 2 x 2 block and the source is a rectangle, so a pixel loses 0, 2 (an edge), 3 (a corner: ONE tap left
    inside) or 4 taps -- never one alone.  All four counts must occur, with both edge columns ix = -1 and ix = src_w - 1"""
    c = RC.cases()["border"]
    sw, sh = c["src_w"], c["src_h"]
    for (mx, my), (ix, iy, fx, fy, _) in zip(RC.maps("border"), _fixed("border")):
        assert ix.min() < -1 and ix.max() > sw and iy.min() < -1 and iy.max() > sh             # out on all four sides
        out = RO.taps_outside(mx, my, sw, sh)
        counts = np.bincount(out.ravel(), minlength=5)
        assert counts[1] == 0 and counts[2] > 0 and counts[3] > 0 and counts[4] > 0
        rows_in = (iy >= 0) & (iy < sh - 1)
        assert ((ix == -1) & rows_in).any() and ((ix == sw - 1) & rows_in).any()
        assert ((iy == -1) & (ix >= 0) & (ix < sw - 1)).any() and ((iy == sh - 1) & (ix >= 0) & (ix < sw - 1)).any()
        assert counts[0] >= out.size // 10                          # at least a tenth fully inside ...
    for ch in (1, 3):
        for rect in RC.rectified_pair("border", ch):
            assert (rect != 0).mean() > 0.5                         # ... so that an image of zeros cannot pass


def test_rational_model_has_its_denominator():
    c = RC.cases()["rational"]
    for e, m in zip(("left", "right"), RC.maps("rational")):
        d = np.asarray(c[e]["dist"])
        assert len(d) == 8 and np.all(d[5:] != 0)
        poly = RO.build_map(dict(c[e], dist=d[:5]), c["dst_w"], c["dst_h"])
        assert np.abs(poly[0] - m[0]).max() > 1.0 and np.abs(poly[1] - m[1]).max() > 0.25     # k4..k6 move pixels


def test_nonfinite_entries_give_zero():
    c = RC.cases()["nonfinite"]
    (lx, ly), (rx, ry) = RC.maps("nonfinite")
    assert not np.isfinite(lx[:, 64]).any() and np.isfinite(np.delete(lx, 64, 1)).all() and np.isfinite(np.delete(ly, 64, 1)[1:]).all()
    assert not np.isfinite(ry[32, 1:]).any() and np.isfinite(np.delete(ry, 32, 0)).all()
    white = np.full((c["src_h"], c["src_w"]), 255, np.uint8)
    for (mx, my), (ix, iy, fx, fy, finite) in zip(RC.maps("nonfinite"), _fixed("nonfinite")):
        bad = ~finite
        assert bad.any() and (ix[bad] == -32768).all() and (iy[bad] == -32768).all() and not fx[bad].any() and not fy[bad].any()
        out = RO.remap(white, mx, my)
        assert not out[bad].any() and (out == 255).mean() > 0.3
        assert ix.max() == 32767 or iy.max() == 32767 or ix.min() == -32768                    # the int16 saturation is reached next to the pole


def test_weights_sum_to_one():
    fy, fx = np.mgrid[0:32, 0:32]
    w = RO.weights(fx, fy)
    assert (sum(w) == 1 << 15).all() and all((x >= 0).all() for x in w)


def test_singular_and_inverse():
    det, inv = RO.inv3(RO.mul3([[2, 0, 3], [0, 4, 5], [0, 0, 1]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]]))
    assert det == 8.0 and inv == [0, 0.25, -1.25, -0.5, 0, 1.5, 0, 0, 1]
    assert RO.inv3([[1, 2, 3], [2, 4, 6], [0, 1, 0]]) == (0.0, None)
    with pytest.raises(ValueError):
        RO.eye_params(dict(K=np.eye(3), R=np.eye(3), P=np.zeros((3, 3))))


def test_new_symbols_are_declared_listed_and_exported(lib_built):
    nrs = lib_built
    lib = nrs.load_library()
    hdr = open(os.path.join(ROOT, "include", "nrs.h")).read()
    declared = set(re.findall(r"\b(nrs_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in nrs.SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name                   # the binding gives each of them its argument types
    assert "typedef struct { double K[9], dist[8], R[9], P[9]; } nrs_rect_eye;" in hdr
    import ctypes as C
    assert C.sizeof(nrs.RectEye) == 35 * 8 and nrs.RectEye.dist.offset == 72 and nrs.RectEye.P.offset == 208
    for cite in ("hamlyn.cc:194-198", "hamlyn.cc:226-229", "NRS_RECT_OWN_LAUNCH"):
        assert cite in hdr, cite
    assert lib.nrs_front_rectify_configure(None, 1, 1, 1, 1, None, None) == -1                # a null context fails cleanly, no device needed
    assert lib.nrs_front_rectify_maps(None, 0, None, None) == -1
    assert lib.nrs_front_process_stereo_raw(*([None] + [None, None, 1, 1, 1, 1, 1] + [None] * 8)) == -1
    for name in ("front_rectify_configure", "front_rectify_maps", "front_process_stereo_raw"):
        assert callable(getattr(nrs.Context, name)), name
    import nrs_frame_loop as FL
    p = inspect.signature(FL.GpuBackend.__init__).parameters
    assert "rectify" in p and p["rectify"].default is None
