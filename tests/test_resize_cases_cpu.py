"""CPU: every designed size of tests/resize_cases.py shows, ON THE ORACLE ALONE (tests/resize_oracle.py), what it is made for -- so that
the GPU test, which holds the device to the oracle on the same cases, covers the identity, the box branch and its rounding, both column
borders, the row border's asymmetry, the rounding ties and more than one workgroup in x -- and the new entry points are declared, listed
and exported."""
import inspect
import os
import re

import numpy as np
import pytest

import resize_cases as ZC
import resize_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["nrs_front_resize_configure", "nrs_front_resize_taps", "nrs_front_process_raw"]
TILE = 256                                                          # destination pixels of one workgroup (k_front_resize_gray)


def test_the_cases_are_the_stated_sizes_and_take_the_stated_branch():
    assert ZC.CASES["identity"] == (40, 30, 40, 30) and ZC.CASES["box_even"] == (64, 48, 32, 24) and ZC.CASES["odd_both"] == (37, 29, 18, 14)
    assert ZC.CASES["width_only_two"] == (66, 29, 33, 14) and ZC.CASES["upscale"] == (20, 12, 45, 31) and ZC.CASES["one_pixel"] == (1, 1, 5, 4)
    assert ZC.CASES["collapse"] == (2, 2, 1, 1) and ZC.CASES["wide"] == (531, 71, 265, 35) and ZC.CASES["wide_box"] == (530, 70, 265, 35)
    box = {n for n in ZC.NAMES if ZC.taps(n)["box"]}
    assert box == {"box_even", "collapse", "wide_box"}
    assert ZC.CASES["odd_both"][2:] == RO.half_size(37, 29)
    sw, sh, dw, dh = ZC.CASES["width_only_two"]
    assert sw == 2 * dw and sh != 2 * dh                            # the x-scale alone is exactly 2


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_identity_gives_the_input_back(ch):
    t = ZC.taps("identity")
    assert np.array_equal(t["sx"], np.arange(40)) and (t["ax"] == (2048, 0)).all()
    assert np.array_equal(t["sy"][:, 0], np.arange(30)) and (t["by"] == (2048, 0)).all()
    for kind in ZC.KINDS:
        assert np.array_equal(ZC.resized("identity", ch, kind), ZC.raw("identity", ch, kind)), kind


def test_box_rounds_with_plus_two():
    """the 0 / 255 checkerboard: every block sums to 510, (510 + 2) >> 2 = 128 where truncation gives 127; a block of (1, 1, 0, 0) sums to
    2 mod 4 and gives 1 where truncation gives 0"""
    for ch in (1, 3, 4):
        out = ZC.resized("box_even", ch, "extremes")
        assert out.shape[:2] == (24, 32) and (out == 128).all()
    img = np.zeros((48, 64), np.uint8)
    img[10, 20:22] = 1                                              # block (10, 5) of the output: 1 + 1 + 0 + 0
    img[13, 7] = 1                                                  # block (6, 3): a sum of 1 rounds down
    img[20:22, 30:32] = (3, 2), (2, 3)                              # block (10, 15): 10 = 2 mod 4 -> 3, truncation 2
    out = RO.resize(img, 32, 24)
    assert out[5, 10] == 1 and out[6, 3] == 0 and out[10, 15] == 3 and out.sum() == 4
    assert RO.resize(np.array([[255, 0], [0, 254]], np.uint8), 1, 1)[0, 0] == 127 and ZC.taps("collapse")["box"] == 1


@pytest.mark.parametrize("name", ["box_even", "collapse", "wide_box"])
def test_box_branch_against_the_general_branch(name):
    """The issue asked for a pixel on which the box branch and the general branch differ.  There is none: exactly halved, every fraction of
    the general rule is 0.5 exactly, its weights are (1024, 1024) on both axes, D_r >> 4 = 64 (s_r0 + s_r1) and (1024 * 64 (s_r0 + s_r1)) >> 16
    = s_r0 + s_r1 without a remainder, so the pixel is (s00 + s01 + s10 + s11 + 2) >> 2 -- the box.  What holds, and is asserted, is the
    opposite: the two branches give the same bytes on every image, the box branch only spares the tables (and stays the branch taken:
    test_the_cases_are_the_stated_sizes_and_take_the_stated_branch)"""
    sw, sh, dw, dh = ZC.CASES[name]
    t = ZC.taps(name)
    assert (t["ax"] == (1024, 1024)).all() and (t["by"] == (1024, 1024)).all()
    assert np.array_equal(t["sx"], 2 * np.arange(dw)) and np.array_equal(t["sy"], np.stack([2 * np.arange(dh), 2 * np.arange(dh) + 1], 1))
    for ch in (1, 3, 4):
        for kind in ZC.KINDS:
            img = ZC.raw(name, ch, kind)
            assert np.array_equal(RO.resize_box(img), RO.resize_general(img, dw, dh)), (ch, kind)


def test_odd_both_keeps_two_taps_in_the_last_column():
    sw, sh, dw, dh = ZC.CASES["odd_both"]
    t = ZC.taps("odd_both")
    assert t["box"] == 0 and t["sx"][-1] == sw - 2 and (t["ax"][-1] > 0).all() and t["sy"][-1].tolist() == [sh - 2, sh - 1] and (t["by"][-1] > 0).all()
    assert (t["ax"].sum(1) == 2048).all() and (t["by"].sum(1) == 2048).all()
    ramp = ZC.raw("odd_both", 1, "ramp")                            # the last output column does depend on the last-but-one and the last source column
    for col in (sw - 2, sw - 1):
        other = ramp.copy()
        other[:, col] ^= 0x80
        assert (RO.resize(other, dw, dh)[:, -1] != ZC.resized("odd_both", 1, "ramp")[:, -1]).any(), col


def test_width_only_two_is_the_general_branch():
    sw, sh, dw, dh = ZC.CASES["width_only_two"]
    t = ZC.taps("width_only_two")
    assert t["box"] == 0 and (t["ax"] == (1024, 1024)).all() and not (t["by"] == (1024, 1024)).all(1).any()
    out = ZC.resized("width_only_two", 3)
    assert out.shape == (dh, dw, 3) and np.array_equal(out, RO.resize_general(ZC.raw("width_only_two", 3), dw, dh))


def test_upscale_borders():
    """Columns: a tap left of the image is zeroed, one on the last source column has a single tap.  Rows: sy = -1 keeps its fraction and both
    rows clamp to row 0, so the row weights -- (628, 1420) at 12 -> 31; the issue's (1024, 1024) would need a scale of 0 -- fall on the same
    row twice and each product is truncated on its own: at least one byte of the top row differs from the single whole weight"""
    sw, sh, dw, dh = ZC.CASES["upscale"]
    t = ZC.taps("upscale")
    s, f = RO.raw_taps(sw, dw)
    assert s[0] == -1 and f[0] > 0 and t["sx"][0] == 0 and t["ax"][0].tolist() == [2048, 0]
    assert s[-1] == sw - 1 and f[-1] > 0 and t["sx"][-1] == sw - 1 and t["ax"][-1].tolist() == [2048, 0]
    inner = (s >= 0) & (s < sw - 1)
    assert inner.sum() > dw // 2 and (t["ax"][inner][:, 1] > 0).any()
    s, f = RO.raw_taps(sh, dh)
    assert s[0] == -1 and t["sy"][0].tolist() == [0, 0] and t["by"][0].tolist() == [628, 1420]
    assert s[-1] == sh - 1 and t["sy"][-1].tolist() == [sh - 1, sh - 1] and t["by"][-1].tolist() == [1420, 628]
    img = ZC.raw("upscale", 1)
    out = ZC.resized("upscale", 1)
    x0 = t["sx"].astype(np.int64)
    x1 = np.where(t["ax"][:, 1] != 0, x0 + 1, x0)
    for row, src_row in ((0, 0), (dh - 1, sh - 1)):
        d = img[src_row].astype(np.int64)[x0] * t["ax"][:, 0] + img[src_row].astype(np.int64)[x1] * t["ax"][:, 1]
        single = (((2048 * (d >> 4)) >> 16) + 2) >> 2               # one whole weight on that row
        assert (np.abs(out[row].astype(np.int64) - single) <= 1).all() and (out[row] != single).any(), row


def test_one_pixel_and_collapse():
    for ch in (1, 3, 4):
        src = ZC.raw("one_pixel", ch)
        out = ZC.resized("one_pixel", ch)
        assert out.shape[:2] == (4, 5)
        # columns take the pixel whole; rows split it over two weights on the same row, which may cost one grey level (never more)
        assert (np.abs(out.astype(int) - src.astype(int)) <= 1).all()
        c = ZC.raw("collapse", ch).astype(np.int64)
        assert np.array_equal(ZC.resized("collapse", ch).astype(np.int64).ravel(), ((c.reshape(4, -1).sum(0) + 2) >> 2))


def test_ties_round_half_to_even():
    sw, sh, dw, dh = ZC.CASES["ties"]
    s, f = RO.raw_taps(sw, dw)
    inner = (s >= 0) & (s < sw - 1)
    assert inner.sum() >= dw - 4
    for p in ((f.astype(np.float64) * 2048)[inner], ((1 - f.astype(np.float64)) * 2048)[inner]):
        assert (p - np.floor(p) == 0.5).all()                       # BOTH products of every inner column end in .5 ...
    ax = ZC.taps("ties")["ax"]
    assert (ax.sum(1) == 2048).all() and (ax[inner] % 2 == 0).all() and ax[1].tolist() == [1538, 510]      # ... half up would give odd 1539 + 511 = 2050


@pytest.mark.parametrize("name", ["wide", "wide_box"])
def test_wide_is_two_workgroups_and_a_ragged_one(name):
    dw = ZC.CASES[name][2]
    assert TILE < dw < 2 * TILE and dw % TILE != 0
    assert ZC.taps("wide")["box"] == 0 and ZC.taps("wide_box")["box"] == 1


def test_images_and_padding():
    for name in ZC.NAMES:
        for ch in (1, 3, 4):
            assert set(np.unique(ZC.raw(name, ch, "extremes"))) <= {0, 255}
            img = ZC.raw(name, ch)
            pad, stride = ZC.padded(img, ch, 5)
            assert stride == img.shape[1] * ch + 5 and (pad[:, -5:] == 0xEE).all()
            assert np.array_equal(pad[:, :stride - 5].reshape(img.shape), img)
    assert len(np.unique(ZC.raw("wide", 3, "ramp"))) == 256 and len(np.unique(ZC.raw("wide", 3))) == 256
    assert ZC.filters("collapse") == [("bright", 225)] and len(ZC.filters("box_even")) == 2


def test_half_size(lib_built):
    nrs = lib_built
    for fn in (nrs.half_size, RO.half_size):
        assert fn(1440, 1080) == (720, 540) and fn(1441, 1081) == (720, 540) and fn(1, 1) == (0, 0)
    # (0, 0) is refused: with a null context at the door, with a real one by the size check (tests/test_gpu_resize.py)
    assert nrs.load_library().nrs_front_resize_configure(None, 1, 1, 0, 0) == -1


def test_new_symbols_are_declared_listed_and_exported(lib_built):
    nrs = lib_built
    lib = nrs.load_library()
    hdr = open(os.path.join(ROOT, "include", "nrs.h")).read()
    declared = set(re.findall(r"\b(nrs_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in nrs.SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name                   # the binding gives each of them its argument types
    for cite in ("endomapper.cc:65-69", "NRS_RESIZE_OWN_LAUNCH"):
        assert cite in hdr, cite
    assert lib.nrs_front_resize_configure(None, 2, 2, 1, 1) == -1  # a null context fails cleanly, no device needed
    assert lib.nrs_front_resize_taps(None, None, None, None, None, None) == -1
    assert lib.nrs_front_process_raw(*([None] + [None, 1, 1, 1, 1] + [None] * 5)) == -1
    for name in ("front_resize_configure", "front_resize_taps", "front_process_raw"):
        assert callable(getattr(nrs.Context, name)), name
    import nrs_frame_loop as FL
    p = inspect.signature(FL.GpuBackend.__init__).parameters
    assert "resize" in p and p["resize"].default is None
