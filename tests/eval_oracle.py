"""NumPy oracle of the evaluation (include/nrs.h "f7: evaluation"), written from the reference files and taking nothing from the library:

  stereo_match_pattern   modules/stereo/stereo_pattern_matching.cc:33-94 (matchTemplate TM_CCORR_NORMED restated with exact integer sums
                         and an fp64 score; OpenCV is not in the tree, so parity with cv::matchTemplate itself is not pinned)
  depth_ground_truth     modules/utilities/frame_evaluator.cc:265-278 with Interpolate of geometry_toolbox.h:47-60
  stereo_from_tracks     modules/stereo/stereo_lucas_kanade.cc:50-72
  eval_rmse              frame_evaluator.cc:54-226
  eval_frame             frame_evaluator.cc:35-52, 291-305

fp32 values are np.float32 operation by operation; sums are sequential fp64 accumulations rounded to fp32 once."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

F32 = np.float32
OK, OUT_OF_BOUNDS, SATURATED, LOW_CORRELATION, ZERO_DISPARITY, BAD_DEPTH, NOT_TRACKED, ROW_DIFFERENCE = range(8)
TRACKED = 1                                                       # utilities/landmark_status.h


def disparity_to_point(prm, bf, disp, u, v):
    prm = np.asarray(prm, F32)
    z = F32(bf) / F32(disp)
    return np.array([z * ((F32(u) - prm[2]) / prm[0]), z * ((F32(v) - prm[3]) / prm[1]), z], F32)


def search_dims(w, h):
    """width and height of matchTemplate's result: the search region (0, 0, w-3, 2*(int)((h-1)/2.f - 2)) minus the template"""
    return (w - 3) - 14, 2 * int(F32(h - 1) / F32(2) - F32(2)) - 14


def stereo_match_pattern_per_keypoint(prm, bf, left, right, xy):
    """the statement this module started with: one full correlation per keypoint.  tests/test_eval_oracle_cpu.py holds
    `stereo_match_pattern` (below) to it byte for byte"""
    left, right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
    h, w = right.shape
    Wr, Hr = search_dims(w, h)
    win = sliding_window_view(right[:Hr + 14, :Wr + 14].astype(np.int64), (15, 15))          # Hr x Wr x 15 x 15
    I2 = (win * win).sum((2, 3))
    xy = np.asarray(xy, F32).reshape(-1, 2)
    n = len(xy)
    xyz = np.full((n, 3), np.nan, F32)
    status = np.zeros(n, np.int32)
    score = np.full(n, np.nan, np.float64)
    match = np.full((n, 2), -1, np.int32)
    for i, (x, y) in enumerate(xy):
        if x < 0 or y < 0 or y > F32(h - 20) or x > F32(w - 20) or not (x == x and y == y):
            status[i] = OUT_OF_BOUNDS
            continue
        if F32(x - F32(7)) < 20 or F32(y - F32(7)) < 0 or F32(x + F32(7)) > w or F32(y + F32(7)) > h:
            status[i] = OUT_OF_BOUNDS
            continue
        ox, oy = int(F32(x - F32(7))), int(F32(y - F32(7)))
        T = left[oy:oy + 15, ox:ox + 15].astype(np.int64)
        if T.max() > 250:
            status[i] = SATURATED
            continue
        TI = (win * T).sum((2, 3))
        den = np.sqrt((T * T).sum().astype(np.float64) * I2.astype(np.float64))
        s = np.where(den > 0, TI.astype(np.float64) / np.where(den > 0, den, 1.0), 0.0)
        k = int(np.argmax(s))                                                              # first maximum in row-major order
        my, mx = divmod(k, Wr)
        score[i], match[i] = s[my, mx], (mx, my)
        if s[my, mx] < 0.99:
            status[i] = LOW_CORRELATION
            continue
        disp = np.abs(F32(mx + 7) - x)
        if disp == 0:
            status[i] = ZERO_DISPARITY
            continue
        xyz[i] = disparity_to_point(prm, bf, disp, x, y)
    return xyz, status, score, match


class ScoreMaps:
    """The fp64 TM_CCORR_NORMED map of a template cell: the 15 x 15 window of `left` whose top-left corner is (ox, oy) against every search
    position of `right`, [Hr, Wr].  A keypoint's result depends on the images and on its integer cell only, so `best` remembers the first
    maximum per cell; case builders read `map` to assert what a scene holds."""

    def __init__(self, left, right):
        self.left, right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
        self.h, self.w = right.shape
        self.Wr, self.Hr = search_dims(self.w, self.h)
        self.win = sliding_window_view(right[:self.Hr + 14, :self.Wr + 14].astype(np.int64), (15, 15))      # Hr x Wr x 15 x 15
        self.I2 = (self.win * self.win).sum((2, 3))
        self._best = {}

    def template(self, ox, oy):
        return self.left[oy:oy + 15, ox:ox + 15].astype(np.int64)

    def map(self, ox, oy):
        T = self.template(ox, oy)
        TI = (self.win * T).sum((2, 3))
        den = np.sqrt((T * T).sum().astype(np.float64) * self.I2.astype(np.float64))
        return np.where(den > 0, TI.astype(np.float64) / np.where(den > 0, den, 1.0), 0.0)

    def best(self, ox, oy):
        """-> (score, mx, my) of the first maximum in row-major order"""
        if (ox, oy) not in self._best:
            s = self.map(ox, oy)
            my, mx = divmod(int(np.argmax(s)), self.Wr)
            self._best[(ox, oy)] = (s[my, mx], mx, my)
        return self._best[(ox, oy)]


def stereo_match_pattern(prm, bf, left, right, xy):
    """stereo_match_pattern_per_keypoint with one correlation per template CELL of the call (ScoreMaps.best)"""
    maps = ScoreMaps(left, right)
    h, w = maps.h, maps.w
    xy = np.asarray(xy, F32).reshape(-1, 2)
    n = len(xy)
    xyz = np.full((n, 3), np.nan, F32)
    status = np.zeros(n, np.int32)
    score = np.full(n, np.nan, np.float64)
    match = np.full((n, 2), -1, np.int32)
    for i, (x, y) in enumerate(xy):
        if x < 0 or y < 0 or y > F32(h - 20) or x > F32(w - 20) or not (x == x and y == y):
            status[i] = OUT_OF_BOUNDS
            continue
        if F32(x - F32(7)) < 20 or F32(y - F32(7)) < 0 or F32(x + F32(7)) > w or F32(y + F32(7)) > h:
            status[i] = OUT_OF_BOUNDS
            continue
        ox, oy = int(F32(x - F32(7))), int(F32(y - F32(7)))
        if maps.template(ox, oy).max() > 250:
            status[i] = SATURATED
            continue
        s, mx, my = maps.best(ox, oy)
        score[i], match[i] = s, (mx, my)
        if s < 0.99:
            status[i] = LOW_CORRELATION
            continue
        disp = np.abs(F32(mx + 7) - x)
        if disp == 0:
            status[i] = ZERO_DISPARITY
            continue
        xyz[i] = disparity_to_point(prm, bf, disp, x, y)
    return xyz, status, score, match


def stereo_from_tracks(prm, bf, left_xy, right_xy, track_status):
    l, r = np.asarray(left_xy, F32).reshape(-1, 2), np.asarray(right_xy, F32).reshape(-1, 2)
    n = len(l)
    xyz, status = np.full((n, 3), np.nan, F32), np.zeros(n, np.int32)
    for i in range(n):
        if track_status[i] != TRACKED:
            status[i] = NOT_TRACKED
        elif float(np.abs(l[i, 1] - r[i, 1])) > 2.0:
            status[i] = ROW_DIFFERENCE
        else:
            disp = np.abs(l[i, 0] - r[i, 0])
            if not disp > 0:
                status[i] = ZERO_DISPARITY
            else:
                xyz[i] = disparity_to_point(prm, bf, disp, l[i, 0], l[i, 1])
    return xyz, status


def unproject_f32(model, prm, u, v):
    """CameraModel::Unproject (pin_hole.cc:33-38, kannala_brandt_8.cc:53-85) in float; sin / cos: the double function rounded to float"""
    prm = np.asarray(prm, F32)
    x, y = (F32(u) - prm[2]) / prm[0], (F32(v) - prm[3]) / prm[1]
    if model == 0:
        return np.array([x, y, 1], F32)
    theta_d = np.sqrt(x * x + y * y)
    th = F32(0)
    if theta_d > F32(1e-8):
        theta = theta_d
        for _ in range(10):
            t2 = theta * theta
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t4 * t4
            a, b, c, d = prm[4] * t2, prm[5] * t4, prm[6] * t6, prm[7] * t8
            fix = (theta * (F32(1) + a + b + c + d) - theta_d) / (F32(1) + F32(3) * a + F32(5) * b + F32(7) * c + F32(9) * d)
            theta = theta - fix
            if np.abs(fix) < F32(1e-6):
                break
        th = theta
    s, co = F32(np.sin(np.float64(th))), F32(np.cos(np.float64(th)))
    return np.array([s * x / theta_d, s * y / theta_d, co], F32)


def depth_ground_truth(model, prm, depth, xy):
    depth = np.asarray(depth, F32)
    h, w = depth.shape
    xy = np.asarray(xy, F32).reshape(-1, 2)
    gt, status = np.full((len(xy), 3), np.nan, F32), np.zeros(len(xy), np.int32)
    one = F32(1)
    with np.errstate(all="ignore"):
        for i, (x, y) in enumerate(xy):
            if not x >= 0 or not y >= 0 or x >= F32(w - 1) or y >= F32(h - 1):
                status[i] = OUT_OF_BOUNDS
                continue
            fx, xi = np.modf(x)
            fy, yi = np.modf(y)
            w00, w01, w10 = (one - fx) * (one - fy), (one - fx) * fy, fx * (one - fy)
            w11 = one - w00 - w01 - w10
            ix, iy = int(xi), int(yi)
            d = depth[iy, ix] * w00 + depth[iy, ix + 1] * w10 + depth[iy + 1, ix] * w01 + depth[iy + 1, ix + 1] * w11
            if not np.isfinite(d):
                status[i] = BAD_DEPTH
                continue
            ray = unproject_f32(model, prm, x, y)
            gt[i] = (ray / ray[2]) * d
    return gt, status


def _sum64(terms):
    acc = np.float64(0)
    for t in terms:
        acc = acc + np.float64(t)
    return F32(acc)


def eval_rmse(est_z, gt_z, gt_ok, align_scales=True, precomputed_depth=False):
    """-> (rmse, scale, (valid, kept, n_inliers), inlier mask over the inputs); rmse = scale = NaN where the reference is undefined"""
    est_z, gt_z, gt_ok = np.asarray(est_z, F32), np.asarray(gt_z, F32), np.asarray(gt_ok).astype(bool)
    n = len(est_z)
    inlier = np.zeros(n, bool)
    idx = np.nonzero(gt_ok)[0]
    nan = F32(np.nan)
    if len(idx) == 0:
        return nan, nan, (0, 0, 0), inlier
    est, gt = est_z[idx], gt_z[idx]
    errors = np.abs(est - gt)
    srt = np.sort(errors)
    q3, q1 = srt[int(F32(len(srt)) * F32(0.75))], srt[int(F32(len(srt)) * F32(0.25))]
    gate = q3 + F32(1.5) * (q3 - q1)
    bypass = bool(align_scales and precomputed_depth)
    keep = np.ones(len(est), bool) if bypass else errors <= gate
    idx, e, g = idx[keep], est[keep], gt[keep]
    n_depths = len(e)
    fraction = F32(0.95) if bypass else F32(0.9)
    n_inl = int(F32(n_depths) * fraction)
    counts = (len(est), n_depths, n_inl)
    if n_inl < 1:
        return nan, nan, counts, inlier
    if not align_scales:
        res = g - e
        sq = res * res
        th = np.sort(sq)[n_inl]
        pick = np.nonzero(sq < th)[0][:n_inl]
        inlier[idx[pick]] = True
        return F32(np.sqrt(_sum64(res[pick] * res[pick]) / F32(n_inl))), F32(1), counts, inlier
    s, rmse = F32(1), nan
    for _ in range(10):
        res = g - s * e
        sq = res * res
        th = np.sort(sq)[n_inl - 1]
        pick = np.nonzero(sq <= th)[0][:n_inl]
        H = _sum64(e[pick] * e[pick])
        G = _sum64((-res[pick]) * e[pick])
        s = F32(s + (-G / H))
        a = g[pick] - s * e[pick]
        rmse = F32(np.sqrt(_sum64(a * a) / F32(n_inl)))
    inlier[idx[pick]] = True
    return rmse, s, counts, inlier


def _rot(q):
    x, y, z, w = [F32(c) for c in q]
    one, two = F32(1), F32(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], F32)


def _act(R, t, X):
    X = np.asarray(X, F32).reshape(-1, 3)
    return np.stack([R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1] + R[r, 2] * X[:, 2] + t[r] for r in range(3)], 1).astype(F32)


def eval_frame(pose_qt, world_xyz, gt_xyz, gt_status, precomputed_depth):
    """-> (rmse, scale, counts, gt_world): camera-frame depth by the SE3f action, eval_rmse, then T^-1 * (gt / scale)"""
    qt = np.asarray(pose_qt, F32)
    R, t = _rot(qt[:4]), qt[4:]
    est = _act(R, t, world_xyz)[:, 2]
    gt_xyz = np.asarray(gt_xyz, F32).reshape(-1, 3)
    ok = np.asarray(gt_status) == OK
    rmse, scale, counts, _ = eval_rmse(est, gt_xyz[:, 2], ok, True, precomputed_depth)
    gw = np.full((len(est), 3), np.nan, F32)
    if np.isfinite(rmse) or counts[2] >= 1:
        Ri = _rot(np.array([-qt[0], -qt[1], -qt[2], qt[3]], F32))
        ti = -_act(Ri, np.zeros(3, F32), t)[0]
        with np.errstate(all="ignore"):
            gw[ok] = _act(Ri, ti, gt_xyz[ok] / scale)
    return rmse, scale, counts, gw
