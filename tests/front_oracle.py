"""CPU restatement of the image front end (reference modules/SLAM/system.cc:113-201, modules/masking/*.cc), NumPy only.

Written from the definitions in DESIGN.md "f5" -- OpenCV's documented conventions for the integer steps, this project's own
definition for the Gaussian -- and shares nothing with the HIP path (csrc/nrs_front.hip).  The GPU tests compare the device
with THIS file, byte for byte.  Everything is plain loops over the (small) structuring elements, vectorised over the pixels.

    to_gray          cvtColor(RGB2GRAY), 8-bit fixed point
    ellipse_spans    getStructuringElement(MORPH_ELLIPSE): the row spans
    erode_rect / erode_ellipse    cv::erode, anchor ksize/2, outside pixels take no part
    gauss_weights / gaussian_blur the project's 11x11 sigma-5 blur (fp32, horizontal then vertical, one rounding)
    bright_filter / border_filter / predefined_prepare / global_mask      the Masker
    clahe_lut / clahe               createCLAHE(clip, 8x8)->apply
    front_process                   everything System::TrackImage does before the tracker
"""
import numpy as np

F32 = np.float32
BRIGHT, BORDER, PREDEFINED = 0, 1, 2


def reflect101(i, n):
    """BORDER_REFLECT_101 index (gfedcb|abcdefgh|gfedcba), any distance"""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def to_gray(img):
    """h x w (grey), h x w x 3 or h x w x 4, channel 0 = R: (R*9798 + G*19235 + B*3735 + 2^14) >> 15"""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img.copy()
    if img.shape[2] == 1:
        return img[:, :, 0].copy()
    r, g, b = (img[:, :, k].astype(np.int64) for k in range(3))
    return ((r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15).astype(np.uint8)


def ellipse_spans(cols, rows):
    """per row i of the element: (j1, j2), columns j1 <= j < j2 are set"""
    r, c = rows // 2, cols // 2
    spans = []
    for i in range(rows):
        dy = i - r
        if abs(dy) <= r:
            dx = int(np.rint(c * np.sqrt((r * r - dy * dy) / float(r * r))))
            spans.append((max(c - dx, 0), min(c + dx + 1, cols)))
        else:
            spans.append((0, 0))
    return spans


def _shifted(img, dy, dx):
    """img read at (y + dy, x + dx); 255 where that is outside (takes no part in a minimum)"""
    h, w = img.shape
    out = np.full((h, w), 255, np.uint8)
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = img[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def erode_rect(img, kw, kh):
    img = np.asarray(img, np.uint8)
    out = np.full(img.shape, 255, np.uint8)
    for i in range(kh):
        for j in range(kw):
            out = np.minimum(out, _shifted(img, i - kh // 2, j - kw // 2))
    return out


def erode_ellipse(img, k):
    img = np.asarray(img, np.uint8)
    out = np.full(img.shape, 255, np.uint8)
    for i, (j1, j2) in enumerate(ellipse_spans(k, k)):
        for j in range(j1, j2):
            out = np.minimum(out, _shifted(img, i - k // 2, j - k // 2))
    return out


def dilate_rect_reflect101(img, k):
    """k x k maximum, anchor k/2, outside pixels by reflect-101 (the support of the blur)"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    out = np.zeros((h, w), np.uint8)
    ys, xs = np.arange(h), np.arange(w)
    for i in range(k):
        for j in range(k):
            out = np.maximum(out, img[reflect101(ys + i - k // 2, h)][:, reflect101(xs + j - k // 2, w)])
    return out


def gauss_weights(k=11, sigma2x2=50.0):
    """g_i = float32(exp(-i^2 / 50)), i = -5..5; their float32 sum taken left to right; w_i = g_i / sum in float32"""
    g = [F32(np.exp(-float(i * i) / sigma2x2)) for i in range(-(k // 2), k // 2 + 1)]
    s = F32(0)
    for v in g:
        s = F32(s + v)
    return [F32(v / s) for v in g]


def gaussian_blur(img):
    """horizontal pass then vertical pass, float32, acc = acc + w_i * v for i = -5..5 in that order (separate multiply and
    add), reflect-101 borders, one rint + saturation at the end"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    wt = gauss_weights()
    ys, xs = np.arange(h), np.arange(w)
    src = img.astype(F32)
    tmp = np.zeros((h, w), F32)
    for i, wi in enumerate(wt):
        tmp = (tmp + (wi * src[:, reflect101(xs + i - 5, w)]).astype(F32)).astype(F32)
    out = np.zeros((h, w), F32)
    for i, wi in enumerate(wt):
        out = (out + (wi * tmp[reflect101(ys + i - 5, h), :]).astype(F32)).astype(F32)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def bright_threshold(gray, th):
    return np.where(np.asarray(gray, np.uint8) > th, 0, 255).astype(np.uint8)


def bright_filter(gray, th):
    return gaussian_blur(erode_ellipse(bright_threshold(gray, th), 11))


def border_roi(w, h, rb, re, cb, ce):
    """cv::Rect(cb, rb, w - ce - cb, h - re - rb); None when it is empty or leaves the image"""
    x, y, rw, rh = cb, rb, w - ce - cb, h - re - rb
    if x < 0 or y < 0 or rw <= 0 or rh <= 0 or x + rw > w or y + rh > h:
        return None
    return x, y, rw, rh


def border_filter(gray, rb, re, cb, ce):
    gray = np.asarray(gray, np.uint8)
    h, w = gray.shape
    x, y, rw, rh = border_roi(w, h, rb, re, cb, ce)
    m = np.zeros((h, w), np.uint8)
    m[y:y + rh, x:x + rw] = 255
    m[gray == 0] = 0
    return erode_rect(m, 21, 21)


def predefined_prepare(mask):
    return erode_ellipse(mask, 20)


def filter_masks(gray, filters):
    """filters: list of (BRIGHT, th) / (BORDER, rb, re, cb, ce, th) / (PREDEFINED, mask) -- the masks in that order"""
    out = []
    for f in filters:
        if f[0] == BRIGHT:
            out.append(bright_filter(gray, f[1]))
        elif f[0] == BORDER:
            out.append(border_filter(gray, f[1], f[2], f[3], f[4]))
        else:
            out.append(predefined_prepare(f[1]))
    return out


def global_mask(shape, masks):
    g = np.full(shape, 255, np.uint8)
    for m in masks:
        g = g & m
    return erode_rect(g, 10, 10)


# ---- CLAHE ---------------------------------------------------------------------------------------------------------------
def clahe_clip_limit(clip, tile_area):
    return max(1, int(F32(clip) * F32(tile_area) / F32(256)))


def clahe_redistribute(hist, clip):
    """cap the bins, hand the excess back: excess / 256 to every bin, the rest one by one to bins 0, step, 2 step, ..."""
    hist = np.asarray(hist, np.int64).copy()
    excess = int(np.maximum(hist - clip, 0).sum())
    hist = np.minimum(hist, clip)
    batch = excess // 256
    residual = excess - batch * 256
    hist += batch
    if residual != 0:
        step = max(256 // residual, 1)
        i = 0
        while i < 256 and residual > 0:
            hist[i] += 1
            i += step
            residual -= 1
    return hist


def clahe_lut(hist, clip, tile_area):
    hist = clahe_redistribute(hist, clip)
    scale = F32(255.0) / F32(tile_area)
    cs = np.cumsum(hist).astype(F32)
    return np.clip(np.rint((cs * scale).astype(F32)), 0, 255).astype(np.uint8)


def clahe_pad(gray, tiles_x=8, tiles_y=8):
    """both sizes multiples of the grid: as is.  Otherwise tiles - size % tiles more columns AND rows, reflect-101 (an axis that
    is already a multiple gets a whole extra `tiles` -- OpenCV's copyMakeBorder call does exactly that)"""
    h, w = gray.shape
    if w % tiles_x == 0 and h % tiles_y == 0:
        return gray
    pw, ph = w + tiles_x - w % tiles_x, h + tiles_y - h % tiles_y
    return gray[reflect101(np.arange(ph), h)][:, reflect101(np.arange(pw), w)]


def clahe_luts(gray, clip=3.0, tiles_x=8, tiles_y=8):
    ext = clahe_pad(np.asarray(gray, np.uint8), tiles_x, tiles_y)
    th, tw = ext.shape[0] // tiles_y, ext.shape[1] // tiles_x
    lim = clahe_clip_limit(clip, tw * th)
    luts = np.zeros((tiles_y, tiles_x, 256), np.uint8)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            t = ext[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
            luts[ty, tx] = clahe_lut(np.bincount(t.ravel(), minlength=256), lim, tw * th)
    return luts, tw, th


def clahe(gray, clip=3.0, tiles_x=8, tiles_y=8):
    gray = np.asarray(gray, np.uint8)
    h, w = gray.shape
    luts, tw, th = clahe_luts(gray, clip, tiles_x, tiles_y)
    lf = luts.astype(F32)
    inv_tw, inv_th = F32(1.0) / F32(tw), F32(1.0) / F32(th)
    txf = (np.arange(w).astype(F32) * inv_tw).astype(F32) - F32(0.5)
    tyf = (np.arange(h).astype(F32) * inv_th).astype(F32) - F32(0.5)
    tx1, ty1 = np.floor(txf).astype(np.int64), np.floor(tyf).astype(np.int64)
    xa, ya = (txf - tx1.astype(F32)).astype(F32), (tyf - ty1.astype(F32)).astype(F32)      # before the indices are clamped
    xa1, ya1 = (F32(1.0) - xa).astype(F32), (F32(1.0) - ya).astype(F32)
    tx2, ty2 = np.minimum(tx1 + 1, tiles_x - 1), np.minimum(ty1 + 1, tiles_y - 1)
    tx1, ty1 = np.maximum(tx1, 0), np.maximum(ty1, 0)
    Y1, Y2, YA, YA1 = ty1[:, None], ty2[:, None], ya[:, None], ya1[:, None]
    X1, X2, XA, XA1 = tx1[None, :], tx2[None, :], xa[None, :], xa1[None, :]
    v = gray.astype(np.int64)
    top = ((lf[Y1, X1, v] * XA1).astype(F32) + (lf[Y1, X2, v] * XA).astype(F32)).astype(F32)
    bot = ((lf[Y2, X1, v] * XA1).astype(F32) + (lf[Y2, X2, v] * XA).astype(F32)).astype(F32)
    res = ((top * YA1).astype(F32) + (bot * YA).astype(F32)).astype(F32)
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def front_process(img, filters, clip=3.0):
    """-> dict(gray, clahe, masks (configuration order), global)"""
    gray = to_gray(img)
    masks = filter_masks(gray, filters)
    return dict(gray=gray, clahe=clahe(gray, clip), masks=masks, **{"global": global_mask(gray.shape, masks)})
