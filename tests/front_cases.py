"""Inputs shared by the image front end's GPU tests (tests/test_gpu_front*.py): seeded frames, filter sets scaled to the frame, and
the conversion of one filter list into the two forms the tests need (nrs.Context.front_configure / tests/front_oracle.py)."""
import numpy as np

import front_oracle as FO


def noise(h, w, ch, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w) if ch == 1 else (h, w, ch)).astype(np.uint8)


def blobs(h, w, ch, seed):
    """mid-grey texture with saturated blobs, some of them cut by the image border, and a few exactly-zero pixels"""
    rng = np.random.default_rng(seed)
    g = rng.integers(60, 200, (h, w)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    r = max(2, min(h, w) // 6)
    for cy, cx in ((0, 0), (h - 1, w // 2), (h // 2, w - 1), (h // 3, w // 3)):
        g[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 255
    g[rng.uniform(size=(h, w)) < 0.002] = 0
    if ch == 1:
        return g
    img = np.repeat(g[:, :, None], ch, 2)
    img[:, :, 1] = np.where(g == 255, 255, rng.integers(0, 256, (h, w))).astype(np.uint8)      # channels differ off the blobs
    return np.ascontiguousarray(img)


def constant(h, w, ch, v):
    return np.full((h, w) if ch == 1 else (h, w, ch), v, np.uint8)


def disk_mask(h, w):
    """an endoscope-like predefined mask: 255 inside an ellipse that leaves the corners out"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((yy - (h - 1) / 2) / (0.55 * h)) ** 2 + ((xx - (w - 1) / 2) / (0.55 * w)) ** 2 <= 1.0, 255, 0).astype(np.uint8)


def border(h, w):
    """a BorderFilter line scaled to the frame (the reference's "20 20 50 20 0" at 640x480), never empty"""
    return ("border", max(1, h // 24), max(1, h // 24), max(1, w // 13), max(1, w // 32), 0)


def filter_sets(h, w):
    return {
        "none": [],
        "endomapper": [("bright", 225), ("predefined", disk_mask(h, w))],
        "hamlyn": [("bright", 255)],
        "border_bright": [border(h, w), ("bright", 200)],
        "two_bright": [("bright", 225), ("bright", 180)],
    }


def to_oracle(filters):
    out = []
    for f in filters:
        if f[0] == "bright":
            out.append((FO.BRIGHT, f[1]))
        elif f[0] == "border":
            out.append((FO.BORDER,) + tuple(f[1:6]))
        else:
            out.append((FO.PREDEFINED, f[1]))
    return out


def check_against_oracle(out, img, filters, tag=""):
    """every output of nrs_front_process against the NumPy restatement, byte for byte"""
    ref = FO.front_process(img, to_oracle(filters))
    for k in ("gray", "clahe", "global"):
        assert out[k].shape == ref[k].shape, (tag, k)
        bad = np.argwhere(out[k] != ref[k])
        assert len(bad) == 0, (tag, k, len(bad), bad[:4].tolist(), out[k][tuple(bad[0])], ref[k][tuple(bad[0])])
    assert len(out["masks"]) == len(ref["masks"]), tag
    for i, (a, b) in enumerate(zip(out["masks"], ref["masks"])):
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (tag, "mask", i, filters[i][0], len(bad), bad[:4].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])
    return ref
