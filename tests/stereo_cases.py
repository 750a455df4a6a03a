"""Inputs shared by the tests of the resident stereo pair (tests/test_front_stereo_host_cpu.py, tests/test_gpu_front_stereo.py): each scene
is built once, with its oracle result, and handed out read-only.

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
