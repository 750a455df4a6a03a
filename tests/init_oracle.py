"""NumPy restatement of the monocular map initialisation (TEST INFRASTRUCTURE ONLY) -- include/nrs.h "f6", DESIGN.md "f6".

Follows EssentialMatrixInitialization::Initialize (modules/tracking/essential_matrix_initialization.cc:47-410) stage by stage:
fp32 element by element where the device is fp32, np.linalg.svd in fp64 on the fp32 matrices where the device runs its fp64 Jacobi.
A second, independent fp64 method (np.linalg.eigh on A^T A) exists for the tolerance derivation of tests/test_gpu_init.py only.
The sampler is this project's own definition (the reference: cv::kmeans + srand(4) / random_shuffle; parity unpinned)."""
import numpy as np

from triang_oracle import project_pt, rays_parallax, se3_inverse, se3_mul_point, triangulate_mid_point, unproject_f32

F32 = np.float32
TRACKED = 1
HALF_PI_F32 = F32(np.pi / 2)
MASK64 = (1 << 64) - 1


def compute_max_tries(inlier_fraction=F32(0.8), success_likelihood=F32(0.95), min_sample_set_size=8):
    """ComputeMaxTries (:78-81): float arguments, std::log(float) over std::log(double), truncated"""
    num = np.log(F32(F32(1) - success_likelihood))
    den = np.log(1.0 - np.float64(inlier_fraction) ** min_sample_set_size)
    return int(np.float64(num) / den)


def _norm3(v):
    return F32(np.sqrt(F32(F32(v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])))


_RAYS = {}


def unit_ray(model, prm, xy):
    """Unproject(...).normalized() in fp32 (memoised: the stages unproject the same keypoints again, as the reference does)"""
    key = (model, np.asarray(prm, F32).tobytes(), F32(xy[0]).tobytes(), F32(xy[1]).tobytes())
    if key not in _RAYS:
        r = unproject_f32(model, prm, xy[0], xy[1])
        _RAYS[key] = (r / _norm3(r)).astype(F32)
    return _RAYS[key]


# ------------------------------------------------------------------------------------------------ stage 1
def compact_unproject(model, prm, ref_xy, cur_xy, status):
    """UnprojectTrackedFeatures (:83-103): (compact_map, reference rays, current rays)"""
    cmap = np.where(np.asarray(status) == TRACKED)[0].astype(np.int32)
    ref = np.array([unit_ray(model, prm, ref_xy[i]) for i in cmap], F32).reshape(-1, 3)
    cur = np.array([unit_ray(model, prm, cur_xy[i]) for i in cmap], F32).reshape(-1, 3)
    return cmap, ref, cur


# ------------------------------------------------------------------------------------------------ stage 2
def init_hash(seed, k):
    z = (seed + (k + 1) * 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def _d2(pts, c):
    dx, dy = (pts[:, 0] - c[0]).astype(F32), (pts[:, 1] - c[1]).astype(F32)
    return (dx * dx + dy * dy).astype(F32)


def sampler(pts, n_hyp, seed):
    """(labels, centres fp32 [8,2], samples [n_hyp,8]) over the compact reference keypoints pts (fp32 [nc,2])"""
    pts = np.asarray(pts, F32)
    nc = len(pts)
    cen = np.zeros((8, 2), F32)
    cen[0] = pts[0]
    mind = _d2(pts, cen[0])
    for k in range(1, 8):
        pick = int(np.argmax(mind))                          # first maximum = lowest index
        cen[k] = pts[pick]
        mind = np.minimum(mind, _d2(pts, cen[k]))
    labels = np.zeros(nc, np.int32)
    for _ in range(10):
        d = np.stack([_d2(pts, cen[c]) for c in range(8)], 1)
        labels = np.argmin(d, axis=1).astype(np.int32)       # first minimum = lowest cluster
        new = cen.copy()
        for c in range(8):
            m = labels == c
            if m.any():
                sx, sy = 0.0, 0.0
                for p in pts[m]:                             # fp64 sums, sequential (they are exact for pixel coordinates: DESIGN.md)
                    sx += float(p[0])
                    sy += float(p[1])
                new[c] = (F32(sx / int(m.sum())), F32(sy / int(m.sum())))
        ddx, ddy = (new[:, 0] - cen[:, 0]).astype(F32), (new[:, 1] - cen[:, 1]).astype(F32)
        moved = bool(np.any((ddx * ddx + ddy * ddy).astype(F32) > F32(1.0)))
        cen = new
        if not moved:
            break
    members = [np.where(labels == c)[0] for c in range(8)]
    samples = np.zeros((n_hyp, 8), np.int32)
    for h in range(n_hyp):
        for c in range(8):
            hs = init_hash(seed, 8 * h + c)
            samples[h, c] = members[c][hs % len(members[c])] if len(members[c]) else hs % nc
    return labels, cen, samples


# ------------------------------------------------------------------------------------------------ stage 3
def build_A(ref_s, cur_s):
    """:183-188, fp32"""
    A = np.zeros((8, 9), F32)
    for i in range(8):
        for k in range(3):
            A[i, 3 * k:3 * k + 3] = (ref_s[i] * cur_s[i, k]).astype(F32)
    return A


def _force_essential(E0):
    U, _, Vt = np.linalg.svd(E0.astype(np.float64))
    return (-(U @ np.diag([1.0, 1.0, 0.0]) @ Vt)).astype(F32)


def compute_E(ref_s, cur_s):
    """ComputeE (:180-206): null vector and 3 x 3 SVD in fp64 from the fp32 matrices, each rounded to fp32"""
    A = build_A(ref_s, cur_s).astype(np.float64)
    v = np.linalg.svd(A, full_matrices=True)[2][8]
    return _force_essential(v.astype(F32).reshape(3, 3))


def compute_E_eigh(ref_s, cur_s):
    """the same by another fp64 route: the eigenvector of A^T A of the smallest eigenvalue; U diag(1,1,0) V^T = E0 (E0^T E0)^-1/2 on the top-2 space"""
    A = build_A(ref_s, cur_s).astype(np.float64)
    w, Q = np.linalg.eigh(A.T @ A)
    E0 = Q[:, 0].astype(F32).reshape(3, 3).astype(np.float64)
    w3, V = np.linalg.eigh(E0.T @ E0)                        # ascending: columns 1, 2 span the top-2 right space
    Ef = sum(np.outer(E0 @ V[:, j], V[:, j]) / np.sqrt(w3[j]) for j in (1, 2))
    return (-Ef).astype(F32)


def align_sign(E, ref):
    """the sign of E is free: the one closer to ref"""
    return E if np.sum((E - ref) ** 2) <= np.sum((E + ref) ** 2) else -E


# ------------------------------------------------------------------------------------------------ stage 4
def score(E, ref_rays, cur_rays, n_matches, threshold):
    """ComputeScoreAndInliers (:236-256): (mask, fp64 angular error per point) -- the mask in fp32 in the device's order"""
    E = np.asarray(E, F32)
    r, c = ref_rays[:n_matches], cur_rays[:n_matches]
    v = np.stack([((E[i, 0] * r[:, 0]).astype(F32) + (E[i, 1] * r[:, 1]).astype(F32)).astype(F32) + (E[i, 2] * r[:, 2]).astype(F32) for i in range(3)], 1).astype(F32)

    def unit(a):
        nn = np.sqrt((((a[:, 0] * a[:, 0]).astype(F32) + (a[:, 1] * a[:, 1]).astype(F32)).astype(F32) + (a[:, 2] * a[:, 2]).astype(F32)).astype(F32)).astype(F32)
        return (a / nn[:, None]).astype(F32)
    v, cn = unit(v), unit(c)
    dot = (((v[:, 0] * cn[:, 0]).astype(F32) + (v[:, 1] * cn[:, 1]).astype(F32)).astype(F32) + (v[:, 2] * cn[:, 2]).astype(F32)).astype(F32)
    with np.errstate(invalid="ignore"):
        ac = np.arccos(dot.astype(np.float64)).astype(F32)
        mask = np.abs((HALF_PI_F32 - ac).astype(F32)) < F32(threshold)
    # the same quantity in fp64 from the same fp32 inputs (the excusal band of the GPU test is measured on it)
    v64 = r.astype(np.float64) @ E.astype(np.float64).T
    v64 /= np.linalg.norm(v64, axis=1, keepdims=True)
    c64 = c.astype(np.float64) / np.linalg.norm(c.astype(np.float64), axis=1, keepdims=True)
    err64 = np.abs(np.pi / 2 - np.arccos(np.clip(np.sum(v64 * c64, 1), -1, 1)))
    return mask, err64


# ------------------------------------------------------------------------------------------------ stage 5
def _R_to_quat64(R):
    """Eigen's matrix -> quaternion (the cases of csrc/nrs_device.hpp R_to_quat), fp64, then normalised with qw >= 0"""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    if q[3] < 0:
        q = -q
    return q / np.sqrt(np.sum(q * q))


def decompose(E):
    """DecomposeEssentialMatrix (:303-318) in fp64, rounded: (R_1, R_2, t) with t's largest component positive (lowest index on ties)"""
    U, _, Vt = np.linalg.svd(np.asarray(E, F32).astype(np.float64))
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1 = U @ W.T @ Vt
    if np.linalg.det(R1) < 0:
        R1 = -R1
    R2 = U @ W @ Vt
    if np.linalg.det(R2) < 0:
        R2 = -R2
    t = U[:, 2] / np.linalg.norm(U[:, 2])
    km = int(np.argmax(np.abs(t)))
    if t[km] < 0:
        t = -t
    return R1.astype(F32), R2.astype(F32), t.astype(F32)


def cameras(E, model, prm, ref_xy, cur_xy, inlier, kp_of):
    """ReconstructCameras (:284-318): camera_transform_world as (q fp32 [4], t fp32 [3]); kp_of[idx] = the keypoint read for flag idx"""
    R1, R2, t = decompose(E)
    tr1, tr2 = F32(F32(R1[0, 0] + R1[1, 1]) + R1[2, 2]), F32(F32(R2[0, 0] + R2[1, 1]) + R2[2, 2])
    R = R2 if tr2 > tr1 else R1
    away = 0
    for idx in np.where(inlier)[0]:
        kp = kp_of[idx]
        r1, r2 = unit_ray(model, prm, ref_xy[kp]), unit_ray(model, prm, cur_xy[kp])
        d = [F32(F32(F32(F32(R[i, 0] * r1[0] + R[i, 1] * r1[1]) + R[i, 2] * r1[2]) - r2[i]) * F32(r2[i] - t[i])) for i in range(3)]
        s = F32(F32(d[0] + d[1]) + d[2])
        away += int(s > 0) - int(s < 0)
    if away < 0:
        t = (-t).astype(F32)
    q = _R_to_quat64(R.astype(np.float64)).astype(F32)
    return q, t


# ------------------------------------------------------------------------------------------------ stage 6
def points(model, prm, ref_xy, cur_xy, q, t, inlier, kp_of, n, radians_per_pixel, min_triangulated=100, max_low_parallax=F32(0.25), xyz64=None):
    """ReconstructPoints (:320-410): (xyz [n,3], code [n], counters [8], verdict, gate margins)"""
    T = np.concatenate([q, t]).astype(F32)
    I = np.array([0, 0, 0, 1, 0, 0, 0], F32)
    wtc = se3_inverse(T)[4:]
    xyz, code = np.zeros((n, 3), F32), np.ones(n, np.int32)
    cnt = np.zeros(8, np.int64)
    margins = np.full(n, np.inf)                             # smallest relative distance to a gate the point was tested against
    gate_par = F32(F32(radians_per_pixel) * F32(5))

    def near(val, gate):
        return abs(float(val) - float(gate)) / max(abs(float(gate)), 1e-30)
    for idx in np.where(inlier)[0]:
        kp = kp_of[idx]
        cnt[0] += 1
        r1, r2 = unit_ray(model, prm, ref_xy[kp]), unit_ray(model, prm, cur_xy[kp])
        X = triangulate_mid_point(r1, r2, I, T)
        par = rays_parallax(X, (X - wtc).astype(F32))
        m = near(par, gate_par)
        c = 0
        if par < gate_par:
            c = 2
        elif X[2] < F32(0):
            c = 3
        else:
            m = min(m, abs(float(X[2])) / max(float(_norm3(X)), 1e-30))
            uv = project_pt(model, prm, X)
            ex, ey = F32(ref_xy[kp][0]) - uv[0], F32(ref_xy[kp][1]) - uv[1]
            e1 = F32(ex * ex + ey * ey)
            m = min(m, near(e1, 5.991))
            if float(e1) > 5.991:
                c = 4
            else:
                pc = se3_mul_point(T, X)
                m = min(m, abs(float(pc[2])) / max(float(_norm3(pc)), 1e-30))
                if pc[2] < F32(0):
                    c = 5
                else:
                    uv = project_pt(model, prm, pc)
                    ex, ey = F32(cur_xy[kp][0]) - uv[0], F32(cur_xy[kp][1]) - uv[1]
                    e2 = F32(ex * ex + ey * ey)
                    m = min(m, near(e2, 5.991))
                    if float(e2) > 5.991:
                        c = 6
        margins[kp] = m
        code[kp] = c
        cnt[c if c else 1] += 1
        if c == 0:
            xyz[kp] = X
    # counters: N, n_triangulated, n_parallax, n_depth_1, n_reprojection_error_1, n_depth_2, n_reprojection_error_2, n_triangulation_error
    counters = np.array([cnt[0], cnt[1], cnt[2], cnt[3], cnt[4], cnt[5], cnt[6], 0], np.int32)
    verdict = 0
    if counters[1] < min_triangulated:
        verdict = 2
    elif float(counters[2]) > float(counters[0]) * float(F32(max_low_parallax)):
        verdict = 3
    return xyz, code, counters, verdict, margins


def triangulate64(ref_xy_kp, cur_xy_kp, model, prm, q, t):
    """the mid-point of one keypoint pair in fp64 (from the fp32 rays): the yardstick of the xyz tolerance"""
    r1 = unit_ray(model, prm, ref_xy_kp).astype(np.float64)
    r2 = unit_ray(model, prm, cur_xy_kp).astype(np.float64)
    f0, f1 = r1 / np.linalg.norm(r1), r2 / np.linalg.norm(r2)
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    Rf0 = R @ f0
    p, qq, r = np.cross(Rf0, f1), np.cross(Rf0, t), np.cross(f1, t)
    nq, nr, npp = np.linalg.norm(qq), np.linalg.norm(r), np.linalg.norm(p)
    x1 = nq / (nq + nr) * (t + nr / npp * (Rf0 + f1))
    return R.T @ (x1 - t)


# ------------------------------------------------------------------------------------------------ the whole call
def kp_table(cmap, n_matches, compact_indexing):
    """which keypoint ReconstructEnvironment / ReconstructPoints read for inlier flag idx: idx itself as the reference writes it
    (:266-267, :331-338), compact_map[idx] with compact_indexing"""
    return np.asarray(cmap[:n_matches]) if compact_indexing else np.arange(n_matches)


def initialize(model, prm, ref_xy, cur_xy, status, n_matches, n_hypotheses=0, epipolar_threshold=F32(0.005), radians_per_pixel=F32(0.0025),
               min_triangulated=100, max_low_parallax=F32(0.25), compact_indexing=0, seed=4, samples=None):
    """EssentialMatrixInitialization::Initialize: dict with the fields of nrs.Context.init_essential"""
    ref_xy, cur_xy = np.asarray(ref_xy, F32), np.asarray(cur_xy, F32)
    n = len(status)
    nh = n_hypotheses if n_hypotheses else compute_max_tries()
    if n_matches < 8:
        return dict(verdict=1, code=np.ones(n, np.int32), xyz=np.zeros((n, 3), F32))
    cmap, ref_rays, cur_rays = compact_unproject(model, prm, ref_xy, cur_xy, status)
    out = dict(n_compact=len(cmap), cmap=cmap, ref_rays=ref_rays, cur_rays=cur_rays)
    if samples is None:
        out["labels"], out["centres"], samples = sampler(ref_xy[cmap], nh, seed)
    samples = np.asarray(samples).reshape(nh, 8)
    hyp_E = np.array([compute_E(ref_rays[s], cur_rays[s]) for s in samples], F32)
    masks = [score(E, ref_rays, cur_rays, n_matches, epipolar_threshold)[0] for E in hyp_E]
    hyp_score = np.array([int(m.sum()) for m in masks], np.int32)
    best = int(np.argmax(hyp_score))                         # first maximum = lowest h
    kp_of = kp_table(cmap, n_matches, compact_indexing)
    q, t = cameras(hyp_E[best], model, prm, ref_xy, cur_xy, masks[best], kp_of)
    xyz, code, counters, verdict, margins = points(model, prm, ref_xy, cur_xy, q, t, masks[best], kp_of, n, radians_per_pixel, min_triangulated,
                                                   max_low_parallax)
    out.update(samples=samples, hyp_E=hyp_E, hyp_score=hyp_score, best_hypothesis=best, score=int(hyp_score[best]), E=hyp_E[best],
               inlier=masks[best], pose_q=q, pose_t=t, xyz=xyz, code=code, counters=counters, verdict=verdict, margins=margins)
    return out
