"""CPU restatement of the stereo rectification (include/nrs.h nrs_front_rectify_configure / nrs_front_process_stereo_raw), NumPy only.

Written from the definition in DESIGN.md 4 "Stereo rectification" -- what the reference's Hamlyn loader does with
cv::initUndistortRectifyMap once and cv::remap(INTER_LINEAR) per frame (modules/datasets/hamlyn.cc:194-229); parity with OpenCV is
unpinned, this file IS the definition's second statement -- and shares nothing with the HIP path.  The GPU tests compare the device
with THIS file: the fp32 maps bit for bit, the rectified bytes byte for byte.

    mul3 / inv3        P R and its inverse by cofactors, in Python floats (IEEE double), the order of DESIGN.md
    eye_params         the map's parameters of one eye record
    build_map          the fp32 maps of one eye
    fix                the fixed-point form of a map: ix, iy, fx, fy (and which entries are finite)
    weights            the four integer tap weights of a pixel
    remap              the rectified image
    taps_outside       how many of a pixel's four taps lie outside the source

An eye record is a dict(K=3x3, dist=up to 8 numbers k1 k2 p1 p2 k3 k4 k5 k6, R=3x3, P=3x3)."""
import numpy as np

F32 = np.float32
F64 = np.float64
TAB = 32
FIX_LIMIT = F32(2.0 ** 30)


def mul3(P, R):
    """M = P R, every entry (p0 r0 + p1 r1) + p2 r2"""
    P, R = [[float(v) for v in row] for row in np.asarray(P, F64).reshape(3, 3)], [[float(v) for v in row] for row in np.asarray(R, F64).reshape(3, 3)]
    return [[(P[i][0] * R[0][j] + P[i][1] * R[1][j]) + P[i][2] * R[2][j] for j in range(3)] for i in range(3)]


def inv3(m):
    """(det, inverse): cofactors written as (a b - c d), det along the first row from the left, the adjugate's entries divided by det"""
    (m0, m1, m2), (m3, m4, m5), (m6, m7, m8) = m
    c00, c01, c02 = m4 * m8 - m5 * m7, m5 * m6 - m3 * m8, m3 * m7 - m4 * m6
    det = (m0 * c00 + m1 * c01) + m2 * c02
    if det == 0.0 or not np.isfinite(det):
        return det, None
    inv = [c00 / det, (m2 * m7 - m1 * m8) / det, (m1 * m5 - m2 * m4) / det,
           c01 / det, (m0 * m8 - m2 * m6) / det, (m2 * m3 - m0 * m5) / det,
           c02 / det, (m1 * m6 - m0 * m7) / det, (m0 * m4 - m1 * m3) / det]
    return det, inv


def eye_params(eye):
    K = np.asarray(eye["K"], F64).reshape(3, 3)
    d = np.zeros(8, F64)
    dist = np.asarray(eye.get("dist", ()), F64).ravel()
    d[:len(dist)] = dist
    det, iR = inv3(mul3(eye["P"], eye["R"]))
    if iR is None:
        raise ValueError("det(P R) = %r" % det)
    return dict(iR=iR, fx=float(K[0, 0]), fy=float(K[1, 1]), cx=float(K[0, 2]), cy=float(K[1, 2]), d=[float(v) for v in d])


def build_map(eye, dst_w, dst_h):
    """-> (map_x, map_y), dst_h x dst_w float32: every pixel evaluated on its own, fp64, sums from the left, one rounding to fp32"""
    q = eye_params(eye)
    iR = [F64(v) for v in q["iR"]]
    k1, k2, p1, p2, k3, k4, k5, k6 = (F64(v) for v in q["d"])
    v, u = np.meshgrid(np.arange(dst_h, dtype=F64), np.arange(dst_w, dtype=F64), indexing="ij")
    with np.errstate(all="ignore"):
        X = (iR[0] * u + iR[1] * v) + iR[2]
        Y = (iR[3] * u + iR[4] * v) + iR[5]
        W = (iR[6] * u + iR[7] * v) + iR[8]
        x, y = X / W, Y / W
        x2, y2 = x * x, y * y
        r2 = x2 + y2
        xy2 = F64(2.0) * (x * y)
        kr = (F64(1.0) + ((k3 * r2 + k2) * r2 + k1) * r2) / (F64(1.0) + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = (x * kr + p1 * xy2) + p2 * (r2 + F64(2.0) * x2)
        yd = (y * kr + p1 * (r2 + F64(2.0) * y2)) + p2 * xy2
        mx = (F64(q["fx"]) * xd + F64(q["cx"])).astype(F32)
        my = (F64(q["fy"]) * yd + F64(q["cy"])).astype(F32)
    return mx, my


def _fix1(m):
    """rint(m * 32) of finite m: the product in fp32 (it may overflow to an infinity), brought into [-2^30, 2^30], rounded half to even"""
    with np.errstate(all="ignore"):
        t = (np.asarray(m, F32) * F32(TAB)).astype(F32)
    return np.rint(np.clip(t, -FIX_LIMIT, FIX_LIMIT)).astype(np.int64)


def fix(map_x, map_y):
    """-> ix, iy (int64, saturated to int16), fx, fy (0..31), finite (bool).  A non-finite entry is the tap (-32768, -32768), fraction 0"""
    map_x, map_y = np.asarray(map_x, F32), np.asarray(map_y, F32)
    finite = np.isfinite(map_x) & np.isfinite(map_y)
    sx, sy = _fix1(np.where(finite, map_x, F32(0))), _fix1(np.where(finite, map_y, F32(0)))
    ix, iy = np.clip(sx >> 5, -32768, 32767), np.clip(sy >> 5, -32768, 32767)          # arithmetic shifts: floor
    fx, fy = sx & (TAB - 1), sy & (TAB - 1)
    ix, iy = np.where(finite, ix, -32768), np.where(finite, iy, -32768)
    fx, fy = np.where(finite, fx, 0), np.where(finite, fy, 0)
    return ix, iy, fx, fy, finite


def weights(fx, fy):
    """the weights of taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1): integers, their sum is 2^15"""
    fx, fy = np.asarray(fx, np.int64), np.asarray(fy, np.int64)
    return (TAB - fx) * (TAB - fy) * 32, fx * (TAB - fy) * 32, (TAB - fx) * fy * 32, fx * fy * 32


def _tap(src, x, y):
    """src (h, w, ch) read at integer (x, y) arrays; 0 outside (BORDER_CONSTANT 0)"""
    h, w = src.shape[:2]
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    p = src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)].astype(np.int64)
    return np.where(inside[..., None], p, 0), inside


def remap(src, map_x, map_y):
    """src: h x w or h x w x ch uint8 -> the rectified image of the maps' shape (and channel count): (sum w_i p_i + 2^14) >> 15"""
    src = np.asarray(src, np.uint8)
    s3 = src[:, :, None] if src.ndim == 2 else src
    ix, iy, fx, fy, _ = fix(map_x, map_y)
    acc = np.zeros(ix.shape + (s3.shape[2],), np.int64)
    for wgt, (dx, dy) in zip(weights(fx, fy), ((0, 0), (1, 0), (0, 1), (1, 1))):
        p, _ = _tap(s3, ix + dx, iy + dy)
        acc += wgt[..., None] * p
    out = ((acc + (1 << 14)) >> 15).astype(np.uint8)
    return out[:, :, 0] if src.ndim == 2 else out


def taps_outside(map_x, map_y, src_w, src_h):
    """per destination pixel, how many of its four taps lie outside a src_w x src_h source (0, 2, 3 or 4: a rectangle never loses one tap alone)"""
    ix, iy, _, _, _ = fix(map_x, map_y)
    n = np.zeros(ix.shape, np.int64)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        x, y = ix + dx, iy + dy
        n += ~((x >= 0) & (x < src_w) & (y >= 0) & (y < src_h))
    return n


def rectify(src, eye, dst_w, dst_h):
    return remap(src, *build_map(eye, dst_w, dst_h))
