// f7, the host half of the evaluation: the trimmed RMSE of FrameEvaluator, the disparity-to-3D step of the stereo matchers and the SE3f
// pieces nrs_eval_frame needs.  Plain C++ (no HIP): nrs_eval.hip includes it for the library, host/eval_check.cpp for a stand-alone
// sanitizer build.  fp32 expressions are written one operation per statement where the order matters; the file is compiled with
// contraction off (pragma below), so no a*b+c becomes an FMA.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include "../../include/nrs.h"

#pragma STDC FP_CONTRACT OFF

namespace nrs_eval {

// fp64 accumulation in index order, rounded to fp32 once (DESIGN.md 4 "Evaluation": the stated replacement of Eigen's vectorised order)
struct Sum64 {
    double s = 0.0;
    void add(float v) { s += (double)v; }
    float value() const { return (float)s; }
};

// stereo_pattern_matching.cc:87-92 / stereo_lucas_kanade.cc:57-64 on a disparity: baseline/disp, times ((u - cx) / fx), ((v - cy) / fy)
inline void disparity_to_point(const float* prm, float bf, float disp, float u, float v, float* o) {
#pragma clang fp contract(off)
    const float z = bf / disp;
    const float rx = (u - prm[2]) / prm[0];
    const float ry = (v - prm[3]) / prm[1];
    o[0] = z * rx;
    o[1] = z * ry;
    o[2] = z;
}

inline int stereo_from_tracks(const nrs_camera* cam, float bf, int32_t n, const float* lxy, const float* rxy, const int32_t* st, float* xyz,
                              int32_t* status) {
    if (!cam || n < 0 || (n > 0 && (!lxy || !rxy || !st || !xyz || !status))) return NRS_ERR_INVALID;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int i = 0; i < n; ++i) {
        float* o = xyz + 3 * (size_t)i;
        o[0] = o[1] = o[2] = nan;
        if (st[i] != NRS_TRACKED) { status[i] = NRS_EVAL_NOT_TRACKED; continue; }
        const float dif_in_rows = std::fabs(lxy[2 * i + 1] - rxy[2 * i + 1]);
        if ((double)dif_in_rows > 2.0) { status[i] = NRS_EVAL_ROW_DIFFERENCE; continue; }
        const float disp = std::fabs(lxy[2 * i] - rxy[2 * i]);
        if (!(disp > 0.f)) { status[i] = NRS_EVAL_ZERO_DISPARITY; continue; }      // (a NaN disparity lands here too: the reference CHECKs)
        disparity_to_point(cam->params, bf, disp, lxy[2 * i], lxy[2 * i + 1], o);
        status[i] = NRS_EVAL_OK;
    }
    return NRS_OK;
}

// ---- SE3f as py/nrs_frame_loop.py writes it: rotation matrix of the quaternion in float, rows summed left to right
struct Rt { float R[9], t[3]; };
inline void quat_R(const float* q, float* R) {
#pragma clang fp contract(off)
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, xw = x * w, yw = y * w, zw = z * w;
    R[0] = 1.f - 2.f * (yy + zz); R[1] = 2.f * (xy - zw);       R[2] = 2.f * (xz + yw);
    R[3] = 2.f * (xy + zw);       R[4] = 1.f - 2.f * (xx + zz); R[5] = 2.f * (yz - xw);
    R[6] = 2.f * (xz - yw);       R[7] = 2.f * (yz + xw);       R[8] = 1.f - 2.f * (xx + yy);
}
inline float row_act(const float* Rr, float t, const float* X) {
#pragma clang fp contract(off)
    const float a = Rr[0] * X[0];
    const float b = Rr[1] * X[1];
    const float c = Rr[2] * X[2];
    float s = a + b;
    s = s + c;
    return s + t;
}
inline Rt se3f(const float* qt) {
    Rt T;
    quat_R(qt, T.R);
    T.t[0] = qt[4]; T.t[1] = qt[5]; T.t[2] = qt[6];
    return T;
}
// T * X, z only: FrameEvaluator::TransformPointCloud (frame_evaluator.cc:228-236) keeps the depth alone
inline float se3f_act_z(const Rt& T, const float* X) { return row_act(T.R + 6, T.t[2], X); }
inline void se3f_act(const Rt& T, const float* X, float* o) {
    for (int r = 0; r < 3; ++r) o[r] = row_act(T.R + 3 * r, T.t[r], X);
}
// inverse: conjugate quaternion, t' = -(R' t) with the rows of R' summed left to right
inline Rt se3f_inv(const float* qt) {
    const float qi[4] = {-qt[0], -qt[1], -qt[2], qt[3]};
    Rt T;
    quat_R(qi, T.R);
    for (int r = 0; r < 3; ++r) T.t[r] = -row_act(T.R + 3 * r, 0.f, qt + 4);
    return T;
}

// ---- the trimmed RMSE (frame_evaluator.cc:54-226)
inline int eval_rmse(int32_t n, const float* est_z, const float* gt_z, const uint8_t* gt_ok, int32_t align_scales, int32_t precomputed_depth,
                     float* rmse, float* scale, int32_t* counts, uint8_t* inlier) {
#pragma clang fp contract(off)
    const float nan = std::numeric_limits<float>::quiet_NaN();
    if (rmse) *rmse = nan;
    if (scale) *scale = nan;
    if (counts) counts[0] = counts[1] = counts[2] = 0;
    if (n < 0 || !rmse || !scale || !counts || (n > 0 && (!est_z || !gt_z || !gt_ok))) return NRS_ERR_INVALID;
    if (inlier) std::fill(inlier, inlier + n, (uint8_t)0);
    std::vector<int> id;                       // index in the caller's arrays
    std::vector<float> est, gt;
    for (int i = 0; i < n; ++i)
        if (gt_ok[i]) { id.push_back(i); est.push_back(est_z[i]); gt.push_back(gt_z[i]); }
    counts[0] = (int)est.size();
    if (est.empty()) return NRS_ERR_INVALID;
    // inter-quartile gate
    std::vector<float> errors(est.size());
    for (size_t i = 0; i < est.size(); ++i) errors[i] = std::fabs(est[i] - gt[i]);
    std::vector<float> sorted = errors;
    std::sort(sorted.begin(), sorted.end());
    const float q3 = sorted[(int)((float)sorted.size() * 0.75f)], q1 = sorted[(int)((float)sorted.size() * 0.25f)];
    const float iqr = q3 - q1;
    const float th_ = 1.5f * iqr;
    const float gate = q3 + th_;
    const bool bypass = align_scales && precomputed_depth;          // the unaligned form has no bypass (:95)
    std::vector<int> kid;
    std::vector<float> e, g;
    for (size_t i = 0; i < est.size(); ++i)
        if (bypass || errors[i] <= gate) { kid.push_back(id[i]); e.push_back(est[i]); g.push_back(gt[i]); }
    const int n_depths = (int)e.size();
    counts[1] = n_depths;
    const float fraction = (align_scales && precomputed_depth) ? 0.95f : 0.9f;
    const int n_inliers = (int)((float)n_depths * fraction);
    counts[2] = n_inliers;
    if (n_inliers < 1) return NRS_ERR_INVALID;
    std::vector<float> res(n_depths), sq(n_depths), ss(n_depths);
    std::vector<int> pick(n_inliers);
    if (!align_scales) {
        for (int i = 0; i < n_depths; ++i) { res[i] = g[i] - e[i]; sq[i] = res[i] * res[i]; }
        ss = sq;
        std::sort(ss.begin(), ss.end());
        const float th = ss[n_inliers];                              // (its own off-by-one, :119; n_inliers < n_depths always)
        Sum64 acc;
        int cur = 0;
        for (int i = 0; i < n_depths && cur < n_inliers; ++i)
            if (sq[i] < th) { acc.add(res[i] * res[i]); if (inlier) inlier[kid[i]] = 1; ++cur; }   // missing residuals count as 0
        *rmse = std::sqrt(acc.value() / (float)n_inliers);
        *scale = 1.f;
        return NRS_OK;
    }
    float s = 1.f, out = nan;
    for (int it = 0; it < 10; ++it) {
        for (int i = 0; i < n_depths; ++i) {
            const float se = s * e[i];
            res[i] = g[i] - se;
            sq[i] = res[i] * res[i];
        }
        ss = sq;
        std::sort(ss.begin(), ss.end());
        const float th = ss[n_inliers - 1];
        int cur = 0;
        for (int i = 0; i < n_depths && cur < n_inliers; ++i)
            if (sq[i] <= th) pick[cur++] = i;                        // ties beyond n_inliers: the first n_inliers in index order
        Sum64 H, G;
        for (int k = 0; k < cur; ++k) {
            const int i = pick[k];
            H.add(e[i] * e[i]);
            const float nr = -res[i];
            G.add(nr * e[i]);
        }
        const float delta = -G.value() / H.value();
        s = s + delta;
        Sum64 A;
        for (int k = 0; k < cur; ++k) {
            const int i = pick[k];
            const float se = s * e[i];
            const float a = g[i] - se;
            A.add(a * a);
        }
        out = std::sqrt(A.value() / (float)n_inliers);
        if (inlier && it == 9)
            for (int k = 0; k < cur; ++k) inlier[kid[pick[k]]] = 1;
    }
    *rmse = out;
    *scale = s;
    return NRS_OK;
}

}  // namespace nrs_eval
