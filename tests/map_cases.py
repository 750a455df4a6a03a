"""The frame-mapping cases tests/test_map_oracle_cpu.py vets on the CPU and tests/test_gpu_map.py runs on the device.

A case = (flat temporal buffer, arguments, the restatement's result, its gate quantities).  The deformable leg of the restatement
(an LM in NumPy) is computed once per base buffer and shared: it depends on neither deform_mag, rad_per_pixel, index_snapshot nor
on which TRACKED ids are left as candidates (its neighbours are the TRACKED_WITH_3D ids).

What provokes which rigid code (include/nrs.h):
  1 close features      KB8 case: the 736 x 552 grid projects denser than 20 px near the border; dense case (spacing 13)
  2 rigidity            deform_mag of a snapshot inside the track above 0.004 (cases all_deforming, one_deforming, dead_band)
  4 parallax            the baseline of make_mapping_buffer puts only the longer tracks inside [10, 20] rad_per_pixel
  6 reprojection, prev. `bent`: a candidate whose oldest keypoint is moved 7 px across the epipolar line
  8 reprojection, cur.  `current_reproj`: two hand-made snapshots.  The mid-point splits the angular error evenly, so the pixel errors
                        differ only through 1 / cos^2 of the off-axis angle: the oldest (`current`) camera is turned 0.35 rad so that
                        it sees the point near its border, the newest sees it at the centre, and the oldest keypoint is moved 5 px
                        across the epipolar line -- 6.36 px^2 there against 4.70 px^2 in the newest camera, whose gate comes first.
                        The same buffer with the turn given to the newest camera instead gives 6 (`previous_reproj`): exchanging
                        the two cameras' gates, or their keypoints, fails one of the two.
  5 depth, previous     `previous_depth`: two hand-made snapshots whose cameras are turned far apart (about 0.7 and 2.6 rad) with a
                        baseline as long as the scene is deep; the mid-point lands behind the newest camera (z = -0.39).  Its
                        parallax there is 1.59 rad, so the case passes rad_per_pixel = 0.1057 (any finite value is accepted) to
                        put it inside the window.
  3 is never produced (TriangulateMidPoint returns no error).  7 is not provoked: it needs a positive depth and a reprojection
  error below 5.991 px^2 in the newest camera together with a negative depth in the oldest.  130 000 random two-view configurations
  (rotations up to 180 degrees in both cameras, baselines over four decades, rad_per_pixel set to parallax / 15 so that the window
  never decides) gave 5 in 4643 of 30 000, and 7 never.  That is a search, not a proof that 7 cannot occur."""
import functools

import numpy as np

import map_oracle as M
import nrs_synth as S

F32 = np.float32


def _copy(tb):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in tb.items()}


@functools.lru_cache(maxsize=None)
def base(name):
    if name == "f4":
        tb = S.make_mapping_buffer(4, 3)
    elif name == "f12":
        tb = S.make_mapping_buffer(12, 3)
    elif name == "f21_kb8":
        tb = S.make_mapping_buffer(21, 3, S.KB8, cand_frac=0.15)
    elif name == "dense":                                          # 1333 ids, > 1024 candidates, no deformable leg
        tb = S.make_mapping_buffer(4, 5, spacing=13.0, cand_frac=0.8)
    else:
        raise KeyError(name)
    return tb, M.deformable_leg(tb)


def _keep_candidates(tb, count):
    """leaves the first `count` TRACKED ids as candidates (the others become BAD: GetTriangulationCandidatesIds skips them)"""
    c = np.nonzero(tb["status"] == 1)[0]
    assert len(c) >= count
    tb["status"][c[count:]] = 3
    return tb


def _mid_snapshot_with_absentee(tb):
    """a snapshot in the middle that some candidate's track spans without having a keypoint there"""
    F = tb["n_frames"]
    for f in sorted(range(2, F - 2), key=lambda f: abs(f - F // 2)):
        for c in np.nonzero(tb["status"] == 1)[0]:
            tr = M.feature_track(tb, int(c))
            if tr[0] < f < tr[-1] and not tb["has_kp"][f, c]:
                return f
    return None


CASES = ["rigid_f4", "all_deforming", "one_deforming", "kb8_f21", "dead_band", "zero_zero", "count_0", "count_1", "count_64", "count_65",
         "count_1025", "index_snapshot", "nan", "bent", "current_reproj", "previous_reproj", "previous_depth"]


def _two_views(turn_oldest):
    """two snapshots, id 0 the candidate, id 1 a map point 60 px from it: the point X seen by a camera turned 0.35 rad about y (the
    oldest one, or the newest) and by an unturned one 15 rad_per_pixel of parallax away; the oldest keypoint moved 5 px in x"""
    prm = S.HAMLYN_PINHOLE
    rpp = float(1.0 / prm[0])
    q = np.array([0.0, np.sin(0.175), 0.0, np.cos(0.175)])
    c, s_ = np.cos(0.35), np.sin(0.35)
    R = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]])
    X, C = np.array([0.1, 0.05, 3.0]), np.array([0.0, 15 * rpp * 3.0, 0.0])

    def proj(p):
        return np.array([prm[0] * p[0] / p[2] + prm[2], prm[1] * p[1] / p[2] + prm[3]])
    if turn_oldest:                                                # oldest: turned, at the origin; newest: unturned, at C
        poses = [np.concatenate([q, np.zeros(3)]), np.concatenate([[0, 0, 0, 1], -C])]
        kp = [proj(R @ X), proj(X - C)]
    else:                                                          # oldest: unturned, at the origin; newest: turned, at C
        poses = [np.array([0, 0, 0, 1, 0, 0, 0.0]), np.concatenate([q, -R @ C])]
        kp = [proj(X), proj(R @ (X - C))]
    kp[0] = kp[0] + [5.0, 0.0]
    tb = dict(n_frames=2, poses=np.array(poses, F32), has_kp=np.ones((2, 2), bool), kp_xy=np.zeros((2, 2, 2), F32), has_lm=np.ones((2, 2), bool),
              lm_xyz=np.zeros((2, 2, 3), F32), status=np.array([1, 0], np.int32), model=S.PINHOLE, prm=prm, rad_per_pixel=rpp,
              deform_mag=np.array([0.001, 0.002], F32), touched=0)
    tb["kp_xy"][:, 0] = kp
    tb["kp_xy"][:, 1] = kp[1] + np.array([60.0, 0.0])
    return tb


def _behind_previous():
    """two snapshots (id 0 the candidate, id 1 a map point 60 px from it) whose mid-point lies behind the newest camera"""
    def unit(q):
        return np.asarray(q, np.float64) / np.linalg.norm(q)
    poses = [np.concatenate([unit([0.0011, 0.2552, -0.2342, 0.9381]), [-0.492, -0.62, 0.49]]),
             np.concatenate([unit([-0.3998, -0.8721, 0.0529, 0.2771]), [0.357, 0.105, -0.93]])]
    kp = [np.array([322.7, 263.5]), np.array([617.3, 368.8])]
    tb = dict(n_frames=2, poses=np.array(poses, F32), has_kp=np.ones((2, 2), bool), kp_xy=np.zeros((2, 2, 2), F32), has_lm=np.ones((2, 2), bool),
              lm_xyz=np.zeros((2, 2, 3), F32), status=np.array([1, 0], np.int32), model=S.PINHOLE, prm=S.HAMLYN_PINHOLE, rad_per_pixel=0.1057,
              deform_mag=np.array([0.001, 0.002], F32), touched=0)
    tb["kp_xy"][:, 0] = kp
    tb["kp_xy"][:, 1] = kp[1] + np.array([-60.0, 0.0])
    return tb


def _deformable_of(tb, c):
    """the deformable result of one candidate, when it reaches DeformableTriangulation (mapping.cc:90-115)"""
    if M.T.closest_map_points(tb, c) and len(M.feature_track(tb, c)) >= 5:
        return {c: M.T.deformable_triangulation(tb, c, tb["model"], tb["prm"], 5)}
    return {}


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(tb, deform_mag, rad_per_pixel, index_snapshot, ref, gates)"""
    index_snapshot, redo = -1, ()
    if name in ("current_reproj", "previous_reproj", "previous_depth"):
        tb = _behind_previous() if name == "previous_depth" else _two_views(name == "current_reproj")
        gates = []
        ref = M.landmark_triangulation(tb, tb["deform_mag"], tb["rad_per_pixel"], gates=gates, deformable={})
        return dict(tb=tb, deform_mag=tb["deform_mag"], rad_per_pixel=tb["rad_per_pixel"], index_snapshot=-1, ref=ref, gates=gates)
    if name in ("rigid_f4", "nan", "bent", "index_snapshot"):
        tb, dl = base("f4")
    elif name == "kb8_f21":
        tb, dl = base("f21_kb8")
    elif name == "count_1025":
        tb, dl = base("dense")
    else:
        tb, dl = base("f12")
    tb = _copy(tb)
    mag = tb["deform_mag"].copy()
    if name == "all_deforming":
        mag[:] = 0.006
    elif name == "one_deforming":
        f = _mid_snapshot_with_absentee(tb)
        if f is None:                                              # the generator drops no keypoint inside a track: make one absence
            f = tb["n_frames"] // 2
            c = [int(c) for c in np.nonzero(tb["status"] == 1)[0] if M.feature_track(tb, int(c))[0] < f][0]
            tb["has_kp"][f, c] = False
            redo = (c,)
        mag[f] = 0.006
        tb["deforming_snapshot"] = f
    elif name == "dead_band":
        pass                                                       # the 12-frame buffer as generated: 53 rigid against 63 deformable
    elif name == "zero_zero":
        mag[:] = 0.006                                             # no rigid success ...
        short = [int(c) for c in np.nonzero(tb["status"] == 1)[0] if len(M.feature_track(tb, int(c))) < 5]
        tb["status"][tb["status"] == 1] = 3
        tb["status"][short] = 1                                    # ... and only short tracks: no deformable success either
    elif name.startswith("count_"):
        _keep_candidates(tb, int(name[6:]))
    elif name == "index_snapshot":
        index_snapshot = 0                                         # the oldest snapshot: tracks that started later have no keypoint there
    elif name in ("nan", "bent"):
        ok = M.landmark_triangulation(tb, mag, tb["rad_per_pixel"], deformable=dl)
        c = int(ok["cand"][np.nonzero(ok["rigid_status"] == 0)[0][3]])
        f0, f1 = M.feature_track(tb, c)[0], M.feature_track(tb, c)[-1]
        if name == "nan":
            tb["kp_xy"][f0, c, 0] = np.nan
        else:
            tb["kp_xy"][f0, c, 1] += F32(7.0)
        tb["touched"] = c
        redo = (c,)
    if redo:
        dl = {k: v for k, v in dl.items() if k not in redo}
        for c in redo:
            dl.update(_deformable_of(tb, c))
    gates = []
    ref = M.landmark_triangulation(tb, mag, tb["rad_per_pixel"], index_snapshot=index_snapshot, gates=gates, deformable=dl)
    return dict(tb=tb, deform_mag=mag, rad_per_pixel=tb["rad_per_pixel"], index_snapshot=index_snapshot, ref=ref, gates=gates)
