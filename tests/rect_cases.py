"""Designed cameras for the stereo rectification (include/nrs.h nrs_front_rectify_configure / nrs_front_process_stereo_raw), shared by
tests/test_rect_cases_cpu.py -- which asserts ON THE ORACLE ALONE that every case shows what it is made for -- and tests/test_gpu_rect.py,
which holds the device to the oracle on all of them.  None of the numbers is a dataset's calibration.

Sizes follow tests/test_gpu_front_stereo.py: raw 64 x 48 -> rectified 70 x 52 (rectified != raw, and the CLAHE padding branch: 70 and 52 are
no multiples of 8) and raw 300 x 44 -> rectified 300 x 79 (the stretched shape of the Hamlyn loader, 720 x 288 -> 720 x 515; past one
256-thread block in x with w % 256 != 0).  The identity needs rectified == raw and stays at 64 x 48."""
import functools

import numpy as np

import front_cases as FC
import rect_oracle as RO

SMALL, WIDE = ((64, 48), (70, 52)), ((300, 44), (300, 79))


def cam(f, cx, cy, fy=None):
    return np.array([[f, 0.0, cx], [0.0, f if fy is None else fy, cy], [0.0, 0.0, 1.0]], np.float64)


def rot(rx, ry, rz):
    """Rz Ry Rx, radians"""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], np.float64)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], np.float64)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], np.float64)
    return Rz @ Ry @ Rx


def eye(K, P, R=None, dist=()):
    return dict(K=K, dist=np.asarray(dist, np.float64), R=np.eye(3) if R is None else R, P=P)


def _case(name, sizes, left, right):
    (sw, sh), (dw, dh) = sizes
    return dict(name=name, src_w=sw, src_h=sh, dst_w=dw, dst_h=dh, left=left, right=right)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case.  Powers of two in the first three make every step of the map exact: what they assert holds to the last bit"""
    out = [
        # 1: K = P, R = I, no distortion: map = (u, v) exactly, every fraction 0, output == input
        _case("identity", ((64, 48), (64, 48)), eye(cam(64, 32, 24), cam(64, 32, 24)), eye(cam(128, 16, 8), cam(128, 16, 8))),
        # 2: half a pixel in x (left) / in y (right): out = (a + b + 1) >> 1
        _case("half_pixel", SMALL, eye(cam(64, 32.5, 24), cam(64, 32, 24)), eye(cam(64, 32, 24.5), cam(64, 32, 24))),
        # 3: 1/64 and 3/64 pixel: map * 32 ends in .5 everywhere; half to even gives fractions 0 and 2 (half up: 1 and 2, truncation: 0 and 1)
        _case("ties", SMALL, eye(cam(64, 32 + 1 / 64, 24 + 3 / 64), cam(64, 32, 24)), eye(cam(64, 32 + 3 / 64, 24 + 1 / 64), cam(64, 32, 24))),
        # 4: rotation and distortion: every fraction index on both axes
        _case("rot_dist", SMALL, eye(cam(60, 31.3, 23.7, 61), cam(58, 34, 25), rot(0.02, -0.03, 0.05), (-0.25, 0.08, 0.002, -0.003, 0.01)),
              eye(cam(61, 32.4, 24.2, 60), cam(58, 35, 26), rot(-0.015, 0.02, -0.04), (-0.22, 0.06, -0.001, 0.002))),
        # 5: the rectified eye looks past the raw one on all four sides (x scaled by 1.1, y by 0.7 about the centre)
        _case("border", WIDE, eye(cam(110, 150, 22, 70), cam(100, 150, 39.5), rot(0, 0, 0.01), (-0.02, 0.004)),
              eye(cam(112, 149, 21.5, 72), cam(100, 150, 39.5), rot(0, 0, -0.01), (-0.02, 0.004))),
        # 6: the rational model: k4, k5, k6 non-zero
        _case("rational", WIDE, eye(cam(120, 148, 21, 90), cam(115, 150, 40), rot(0.01, 0.01, -0.02), (0.1, -0.02, 0.001, 0.0005, 0.003, 0.05, -0.01, 0.002)),
              eye(cam(118, 151, 22, 88), cam(115, 150, 40), rot(-0.01, 0.01, 0.02), (0.12, -0.03, -0.001, 0.0005, 0.002, 0.04, -0.02, 0.003))),
        # 7: P R = [1 0 0; 0 1 0; 1/64 0 1]: W = 1 - u / 64 is exactly 0 in column 64 (the right eye: 1 - v / 32, row 32): those entries are
        # not finite; before the pole the map runs through the raw eye, behind it the coordinates are negative
        _case("nonfinite", SMALL, eye(cam(0.5, 0, 0), np.array([[1, 0, 0], [0, 1, 0], [1 / 64, 0, 1]], np.float64)),
              eye(cam(0.5, 0, 0), np.array([[1, 0, 0], [0, 1, 0], [0, 1 / 32, 1]], np.float64))),
    ]
    return {c["name"]: c for c in out}


NAMES = ("identity", "half_pixel", "ties", "rot_dist", "border", "rational", "nonfinite")


@functools.lru_cache(maxsize=None)
def maps(name):
    """((map_x, map_y) left, (map_x, map_y) right) of the oracle, computed once"""
    c = cases()[name]
    out = tuple(RO.build_map(c[e], c["dst_w"], c["dst_h"]) for e in ("left", "right"))
    for m in out:
        for a in m:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def raw_pair(name, ch):
    """the raw eyes of a case: the blobs / noise frames of the front end's tests at the raw size"""
    c = cases()[name]
    w, h = c["src_w"], c["src_h"]
    left = FC.blobs(h, w, ch, 500 + w + ch)
    right = (FC.blobs(h, w, ch, 600 + w + ch) // 2 + FC.noise(h, w, ch, 700 + w + ch) // 2).astype(np.uint8)
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


@functools.lru_cache(maxsize=None)
def rectified_pair(name, ch):
    """the oracle's rectified eyes of raw_pair(name, ch)"""
    (ml, mr), (left, right) = maps(name), raw_pair(name, ch)
    out = RO.remap(left, *ml), RO.remap(right, *mr)
    for a in out:
        a.setflags(write=False)
    return out


def padded(img, ch, pad):
    """(h x stride raw bytes, stride): the rows of img followed by `pad` bytes of 0xEE"""
    h, w = img.shape[:2]
    raw = np.full((h, w * ch + pad), 0xEE, np.uint8)
    raw[:, :w * ch] = img.reshape(h, w * ch)
    return raw, w * ch + pad
