"""GPU: the image front end (include/nrs.h f5: grey conversion, CLAHE, the Masker's filter masks and the Global mask) against
tests/front_oracle.py, BYTE FOR BYTE on every output.  Sizes are the smallest that reach each branch: 64x48 (CLAHE tile 8x6, clip
floored to 1), 160x120 (tile 20x15, clip 3), 83x61 (padded on both axes), 72x50 (padded although the width is a multiple of 8),
9x7 (smaller than every structuring element), and one 640x480."""
import ctypes as C

import numpy as np
import pytest

import nrs
import front_cases as FC

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (160, 120), (83, 61), (72, 50), (9, 7), (640, 480)]
SETS = ["none", "endomapper", "hamlyn", "border_bright", "two_bright"]


@pytest.fixture(scope="module")
def fctx():
    c = nrs.Context()
    yield c
    c.close()


@pytest.mark.parametrize("wh", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fset", SETS)
def test_sizes_and_filter_sets(fctx, wh, fset):
    w, h = wh
    filters = FC.filter_sets(h, w)[fset]
    ch = (1, 3, 4)[(SIZES.index(wh) + SETS.index(fset)) % 3]
    img = FC.blobs(h, w, ch, 100 + w) if fset in ("endomapper", "two_bright") else FC.noise(h, w, ch, 7 + w)
    fctx.front_configure(filters)
    out = fctx.front_process(img)
    ref = FC.check_against_oracle(out, img, filters, (wh, fset, ch))
    if fset == "hamlyn":
        assert (ref["masks"][0] == 255).all()                  # v > 255 never fires


@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("kind", ["noise", "blobs", "black", "white"])
def test_images_and_channels(fctx, kind, ch):
    w, h = 160, 120
    img = {"noise": lambda: FC.noise(h, w, ch, 3), "blobs": lambda: FC.blobs(h, w, ch, 4),
           "black": lambda: FC.constant(h, w, ch, 0), "white": lambda: FC.constant(h, w, ch, 255)}[kind]()
    filters = [FC.border(h, w), ("bright", 225), ("predefined", FC.disk_mask(h, w))]
    fctx.front_configure(filters)
    out = fctx.front_process(img)
    ref = FC.check_against_oracle(out, img, filters, (kind, ch))
    if kind == "black":
        assert (ref["masks"][0] == 0).all() and (ref["global"] == 0).all()      # BorderFilter zeroes every black pixel
    if kind == "white":
        assert (ref["masks"][1] == 0).all()
    if kind == "blobs":
        assert (ref["global"] == 0).any() and (ref["global"] != 0).any()


@pytest.mark.parametrize("ch,stride", [(1, 96), (3, 83 * 3 + 7), (4, 83 * 4)])
def test_row_stride(fctx, ch, stride):
    w, h = 83, 61
    img = FC.blobs(h, w, ch, 21)
    raw = np.full((h, stride), 0xA5, np.uint8)                 # padding bytes that must not be read as pixels
    raw[:, :w * ch] = img.reshape(h, w * ch)
    filters = FC.filter_sets(h, w)["border_bright"]
    fctx.front_configure(filters)
    out = fctx.front_process(raw, stride=stride, width=w, channels=ch)
    FC.check_against_oracle(out, img, filters, (ch, stride))


def test_outputs_are_optional(fctx):
    w, h = 64, 48
    img = FC.noise(h, w, 3, 5)
    filters = FC.filter_sets(h, w)["border_bright"]
    fctx.front_configure(filters)
    full = fctx.front_process(img)
    assert fctx.front_process(img, outputs=False) == {}
    only = fctx.front_process(img, outputs=("global",))
    assert list(only) == ["global"] and np.array_equal(only["global"], full["global"])
    # one of the per-filter pointers null: the other is still written
    m1 = np.zeros((h, w), np.uint8)
    ptrs = (C.c_void_p * 2)(None, m1.ctypes.data)
    rc = fctx.lib.nrs_front_process(fctx.h, C.c_void_p(img.ctypes.data), C.c_int32(w), C.c_int32(h), C.c_int32(w * 3), C.c_int32(3),
                                    None, None, None, ptrs)
    assert rc == 0 and np.array_equal(m1, full["masks"][1])


def test_stateful_sequence(fctx):
    """three frames, a size change, a reconfiguration: nothing of an earlier frame or configuration leaks into a later one"""
    filters = [FC.border(120, 160), ("bright", 210)]
    fctx.front_configure(filters)
    for k in range(3):
        img = FC.blobs(120, 160, 3, 40 + k)
        FC.check_against_oracle(fctx.front_process(img), img, filters, ("frame", k))
    img = FC.blobs(61, 83, 1, 50)                              # smaller frame in the same (larger) buffers
    FC.check_against_oracle(fctx.front_process(img), img, filters, "size change")
    img = FC.noise(200, 320, 4, 51)                            # larger: buffers grow
    FC.check_against_oracle(fctx.front_process(img), img, filters, "size change 2")
    filters = [("bright", 128), ("predefined", FC.disk_mask(200, 320)), ("bright", 250)]
    fctx.front_configure(filters)
    FC.check_against_oracle(fctx.front_process(img), img, filters, "reconfigured")
    fctx.front_configure([])
    out = fctx.front_process(img)
    assert out["masks"] == [] and (out["global"] == 255).all()
    FC.check_against_oracle(out, img, [], "no filters")


def test_error_paths(fctx):
    INVALID = -1
    img = FC.noise(48, 64, 1, 1)
    fctx.front_configure([])

    def raw(w, h, stride, ch, data=img):
        return fctx.lib.nrs_front_process(fctx.h, C.c_void_p(data.ctypes.data), C.c_int32(w), C.c_int32(h), C.c_int32(stride), C.c_int32(ch),
                                          None, None, None, None)
    assert raw(0, 48, 64, 1) == INVALID and raw(64, 0, 64, 1) == INVALID
    assert raw(64, 48, 64, 2) == INVALID and raw(64, 48, 64, 0) == INVALID and raw(64, 48, 64, 5) == INVALID
    assert raw(64, 48, 63, 1) == INVALID                       # stride below the row
    assert fctx.lib.nrs_front_process(fctx.h, None, C.c_int32(64), C.c_int32(48), C.c_int32(64), C.c_int32(1), None, None, None, None) == INVALID
    with pytest.raises(nrs.NrsError) as ei:
        fctx.front_process(np.zeros((48, 64, 2), np.uint8))
    assert ei.value.code == INVALID
    # a PREDEFINED mask of another size
    fctx.front_configure([("predefined", FC.disk_mask(48, 60))])
    with pytest.raises(nrs.NrsError) as ei:
        fctx.front_process(img)
    assert ei.value.code == INVALID
    # BorderFilter: empty ROI, ROI leaving the image (negative margins are refused when configured)
    for rec in [("border", 24, 24, 0, 0, 0), ("border", 0, 0, 40, 24, 0), ("border", 20, 20, 50, 20, 0)]:
        fctx.front_configure([rec])
        with pytest.raises(nrs.NrsError) as ei:
            fctx.front_process(img)
        assert ei.value.code == INVALID, rec
    for rec in [("border", -1, 0, 0, 0, 0), ("border", 0, 0, 0, -3, 0)]:
        with pytest.raises(nrs.NrsError) as ei:
            fctx.front_configure([rec])
        assert ei.value.code == INVALID, rec
    # configuration: only the 8x8 grid is built; clip must be positive; at most NRS_FRONT_MAX_FILTERS filters; known kinds
    for kw in (dict(tiles=(4, 4)), dict(tiles=(8, 16)), dict(clahe_clip=0.0)):
        with pytest.raises(nrs.NrsError) as ei:
            fctx.front_configure([], **kw)
        assert ei.value.code == INVALID, kw
    with pytest.raises(nrs.NrsError) as ei:
        fctx.front_configure([("bright", 200)] * 9)
    assert ei.value.code == INVALID
    rec = (nrs.FrontFilter * 1)()
    rec[0].kind = 7
    assert fctx.lib.nrs_front_configure(fctx.h, C.c_int32(1), rec, C.c_float(3.0), C.c_int32(8), C.c_int32(8)) == INVALID
    assert fctx.lib.nrs_front_configure(fctx.h, C.c_int32(1), None, C.c_float(3.0), C.c_int32(8), C.c_int32(8)) == INVALID
    # and the context still works afterwards
    fctx.front_configure([("bright", 200)])
    FC.check_against_oracle(fctx.front_process(img), img, [("bright", 200)], "after errors")
