"""Designed sizes and images for the frame resize (include/nrs.h nrs_front_resize_configure / nrs_front_process_raw), shared by
tests/test_resize_cases_cpu.py -- which asserts ON THE ORACLE ALONE (tests/resize_oracle.py) that every case shows what it is made for --
and tests/test_gpu_resize.py, which holds the device to the oracle on all of them.  None of the sizes is a dataset's, but `odd_both` and
the 1440 x 1080 of the GPU test's resident case are halved the way apps/endomapper.cc:65-69 halves its frames."""
import functools

import numpy as np

import front_cases as FC
import resize_oracle as RO

# name -> (src_w, src_h, dst_w, dst_h)
CASES = {
    # scale 1: taps (x, 2048, 0), output == input
    "identity": (40, 30, 40, 30),
    # exactly halved: the box branch
    "box_even": (64, 48, 32, 24),
    # half_size of an odd frame: the general branch; the last destination column still has two taps
    "odd_both": (37, 29, 18, 14),
    # the x-scale is exactly 2, the y-scale is not: NOT the box branch
    "width_only_two": (66, 29, 33, 14),
    # up-scaling: column 0 has sx = -1 (zeroed), the last columns sit on the last source column with one tap, row 0 has sy = -1: both of
    # its weights fall on source row 0
    "upscale": (20, 12, 45, 31),
    "one_pixel": (1, 1, 5, 4),
    # the box branch at its smallest
    "collapse": (2, 2, 1, 1),
    # dst_w = 2048 and an odd src_w: every column fraction is an odd multiple of 1 / 4096, so BOTH products (1 - f) * 2048 and f * 2048 end
    # in .5 in every column and half-to-even decides a0 and a1
    "ties": (1023, 7, 2048, 5),
    # The kernel's workgroup is 256 consecutive destination pixels of one row (k_front_resize_gray, csrc/nrs_front.hip): 265 columns are two
    # workgroups in x, the second ragged with 9 pixels -- in the general branch ...
    "wide": (531, 71, 265, 35),
    # ... and in the box branch
    "wide_box": (530, 70, 265, 35),
}
NAMES = tuple(CASES)


def sizes(name):
    return CASES[name]


@functools.lru_cache(maxsize=None)
def taps(name):
    """the oracle's tables of a case: dict(sx, ax, sy, by, box), computed once"""
    sw, sh, dw, dh = CASES[name]
    sx, ax = RO.col_taps(sw, dw)
    sy, by = RO.row_taps(sh, dh)
    out = dict(sx=sx, ax=ax, sy=sy, by=by)
    for a in out.values():
        a.setflags(write=False)
    out["box"] = int(RO.is_box(sw, sh, dw, dh))
    return out


def _shape(h, w, ch):
    return (h, w) if ch == 1 else (h, w, ch)


def noise(name, ch):
    sw, sh = CASES[name][:2]
    return FC.noise(sh, sw, ch, 900 + sw + 7 * ch)


def ramp(name, ch):
    """a ramp in x and y, another slope per channel, wrapping at 256"""
    sw, sh = CASES[name][:2]
    y, x = np.mgrid[0:sh, 0:sw]
    img = np.stack([(x * (3 + c) + y * (5 + 2 * c) + 11 * c) & 255 for c in range(ch)], -1).astype(np.uint8)
    return np.ascontiguousarray(img.reshape(_shape(sh, sw, ch)))


def extremes(name, ch):
    """0 / 255 only: a one-pixel checkerboard, the channels in opposite phase"""
    sw, sh = CASES[name][:2]
    y, x = np.mgrid[0:sh, 0:sw]
    img = np.stack([(((x + y + c) & 1) * 255) for c in range(ch)], -1).astype(np.uint8)
    return np.ascontiguousarray(img.reshape(_shape(sh, sw, ch)))


KINDS = dict(noise=noise, ramp=ramp, extremes=extremes)


@functools.lru_cache(maxsize=None)
def raw(name, ch, kind="noise"):
    img = KINDS[kind](name, ch)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def resized(name, ch, kind="noise"):
    """the oracle's resize of raw(name, ch, kind)"""
    dw, dh = CASES[name][2:]
    out = RO.resize(raw(name, ch, kind), dw, dh)
    out.setflags(write=False)
    return out


def padded(img, ch, pad):
    """(h x stride raw bytes, stride): the rows of img followed by `pad` bytes of 0xEE that must never be read into the result"""
    h, w = img.shape[:2]
    out = np.full((h, w * ch + pad), 0xEE, np.uint8)
    out[:, :w * ch] = img.reshape(h, w * ch)
    return out, w * ch + pad


def filters(name):
    """the filter set of a case's front-end run: BrightFilter always, BorderFilter where the resized frame has room for its ROI"""
    dw, dh = CASES[name][2:]
    return [("bright", 225)] + ([FC.border(dh, dw)] if min(dw, dh) >= 8 else [])
