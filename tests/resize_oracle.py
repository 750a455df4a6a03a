"""CPU restatement of the frame resize (include/nrs.h nrs_front_resize_configure / nrs_front_process_raw; the cv::resize(INTER_LINEAR) of
reference apps/endomapper.cc:65-69), NumPy only.

Written from the definition in DESIGN.md 4 "Frame resize" -- OpenCV's 8-bit INTER_LINEAR conventions -- and shares nothing with the HIP
path (csrc/nrs_front.hip, csrc/nrs_resize_host.hpp).  The GPU tests compare the device with THIS file, tables and bytes, exactly.

    half_size        the app's newSize: Size(cols / 2.0f, rows / 2.0f)
    is_box           exactly halved in both directions: the 2 x 2 box branch
    raw_taps         first source index and fp32 fraction of every destination index of one axis, before any border rule
    weights          the two 11-bit weights of a fraction, each rounded half to even on its own
    col_taps         sx [dst_w], ax [dst_w, 2]: fraction zeroed left of the image and on its last column
    row_taps         sy [dst_h, 2] (clamped), by [dst_h, 2]: fraction kept
    resize_general / resize_box / resize
"""
import numpy as np

F32 = np.float32
ONE = 2048


def half_size(w, h):
    return int(F32(w) / F32(2)), int(F32(h) / F32(2))


def is_box(src_w, src_h, dst_w, dst_h):
    return src_w == 2 * dst_w and src_h == 2 * dst_h


def raw_taps(src, dst):
    """-> (s int64 [dst], f float32 [dst]): f = float32((d + 0.5) * scale - 0.5) with the product in float64, s = floor(f), f -= s in float32"""
    scale = 1.0 / (float(dst) / float(src))
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    return s, (f - s.astype(F32)).astype(F32)


def _sat16(v):
    return np.clip(v, -32768, 32767).astype(np.int16)


def weights(f):
    """[n, 2] int16: rint((1 - f) * 2048), rint(f * 2048), float32 throughout, numpy's rint rounds half to even"""
    f = np.asarray(f, F32)
    w0 = np.rint(((F32(1) - f).astype(F32) * F32(ONE)).astype(F32)).astype(np.int64)
    w1 = np.rint((f * F32(ONE)).astype(F32)).astype(np.int64)
    return np.stack([_sat16(w0), _sat16(w1)], -1)


def col_taps(src_w, dst_w):
    s, f = raw_taps(src_w, dst_w)
    left = s < 0
    s, f = np.where(left, 0, s), np.where(left, F32(0), f).astype(F32)
    right = s >= src_w - 1
    s, f = np.where(right, src_w - 1, s), np.where(right, F32(0), f).astype(F32)
    return s.astype(np.int32), weights(f)


def row_taps(src_h, dst_h):
    s, f = raw_taps(src_h, dst_h)
    sy = np.stack([np.clip(s, 0, src_h - 1), np.clip(s + 1, 0, src_h - 1)], -1).astype(np.int32)
    return sy, weights(f)


def _as3(img):
    img = np.asarray(img, np.uint8)
    return img[:, :, None] if img.ndim == 2 else img


def resize_general(img, dst_w, dst_h):
    """the general branch whatever the sizes (the box case included: tests compare the two branches)"""
    src = _as3(img).astype(np.int64)
    h, w = src.shape[:2]
    sx, ax = col_taps(w, dst_w)
    sy, by = row_taps(h, dst_h)
    x0 = sx.astype(np.int64)
    x1 = np.where(ax[:, 1] != 0, x0 + 1, x0)                        # a second tap of weight 0 is not read
    assert x1.max() < w
    a0, a1 = ax[:, 0].astype(np.int64)[None, :, None], ax[:, 1].astype(np.int64)[None, :, None]
    b0, b1 = by[:, 0].astype(np.int64)[:, None, None], by[:, 1].astype(np.int64)[:, None, None]
    d0 = src[sy[:, 0]][:, x0] * a0 + src[sy[:, 0]][:, x1] * a1
    d1 = src[sy[:, 1]][:, x0] * a0 + src[sy[:, 1]][:, x1] * a1
    assert np.abs(d0).max() < 2 ** 31 and np.abs(b0 * (d0 >> 4)).max() < 2 ** 31          # what the device holds in int32
    out = (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2
    out = np.clip(out, 0, 255).astype(np.uint8)
    return out[:, :, 0] if np.asarray(img).ndim == 2 else out


def resize_box(img):
    src = _as3(img).astype(np.int64)
    h, w = src.shape[:2]
    assert h % 2 == 0 and w % 2 == 0
    out = ((src[0::2, 0::2] + src[0::2, 1::2] + src[1::2, 0::2] + src[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    return out[:, :, 0] if np.asarray(img).ndim == 2 else out


def resize(img, dst_w, dst_h):
    """h x w or h x w x channels uint8 -> dst_h x dst_w (x channels), channel by channel"""
    h, w = np.asarray(img).shape[:2]
    return resize_box(img) if is_box(w, h, dst_w, dst_h) else resize_general(img, dst_w, dst_h)
