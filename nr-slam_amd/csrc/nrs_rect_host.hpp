// Host half of the stereo rectification (nrs_front.hip; include/nrs.h nrs_front_rectify_configure / nrs_front_process_stereo_raw, DESIGN.md 4
// "Stereo rectification") in plain C++: the refusals with their texts, P R and its inverse, the map of one destination pixel, the
// fixed-point tap rule and the blend of one pixel.  The three per-pixel bodies are the ones the kernels run: there is one definition.
// No HIP here: host/rect_check.cpp runs it under AddressSanitizer + UBSan (`make rect_check`).  tests/rect_oracle.py restates all of it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "../../include/nrs.h"

#ifdef __HIPCC__
#define NRS_RECT_HD __host__ __device__
#else
#define NRS_RECT_HD
#endif

namespace nrs {

constexpr int RECT_MAX_SIZE = 16384;             // either side of the raw or of the rectified eye (an index then fits the int16 of a tap)
constexpr int RECT_TAB = 32, RECT_TAB_BITS = 5;  // OpenCV's INTER_TAB_SIZE: fractions in 1/32 pixel
constexpr int RECT_ONE_BITS = 15;                // its INTER_REMAP_COEF_BITS: the four weights of a pixel sum to 2^15
constexpr float RECT_FIX_LIMIT = 1073741824.f;   // 2^30: the product map * 32 is brought into [-2^30, 2^30] before it is rounded to an integer

// the refusals' texts: formats here, so that the stand-alone program and the library print the same words
constexpr const char* RECT_MSG_NULL = "%s: null eye record";
constexpr const char* RECT_MSG_SIZE = "%s: %s size %d x %d (1 .. %d each)";
constexpr const char* RECT_MSG_FINITE = "%s: %s eye: %s[%d] is not finite";
constexpr const char* RECT_MSG_DET = "%s: %s eye: det(P R) is %g, the map has no inverse";
constexpr const char* RECT_MSG_NONE = "%s: no rectification has been configured (nrs_front_rectify_configure)";
constexpr const char* RECT_MSG_RAW = "%s: the raw eyes are %d x %d, the configured ones %d x %d";
constexpr const char* RECT_MSG_EYE = "%s: eye = %d (0: left, 1: right)";

// what the map of one eye needs: (P R)^-1 row-major, K's four entries, the eight distortion coefficients k1 k2 p1 p2 k3 k4 k5 k6
struct RectEye { double iR[9], fx, fy, cx, cy, d[8]; };

// M = P R: every entry the sum over k = 0, 1, 2 from the left, (p0 r0 + p1 r1) + p2 r2
inline void rect_mul3(const double* P, const double* R, double* M) {
#pragma clang fp contract(off)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[3 * i + j] = (P[3 * i] * R[j] + P[3 * i + 1] * R[3 + j]) + P[3 * i + 2] * R[6 + j];
}

// M^-1 by cofactors: c_ij = the 2 x 2 minor written as (a b - c d), det = (m00 c00 + m01 c01) + m02 c02 along the first row, every entry
// of the adjugate divided by det.  -> det (the inverse is written only when it is non-zero and finite)
inline double rect_inv3(const double* m, double* inv) {
#pragma clang fp contract(off)
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = (m[0] * c00 + m[1] * c01) + m[2] * c02;
    if (!(det != 0.0) || !std::isfinite(det)) return det;
    inv[0] = c00 / det;                         inv[1] = (m[2] * m[7] - m[1] * m[8]) / det; inv[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    inv[3] = c01 / det;                         inv[4] = (m[0] * m[8] - m[2] * m[6]) / det; inv[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    inv[6] = c02 / det;                         inv[7] = (m[1] * m[6] - m[0] * m[7]) / det; inv[8] = (m[0] * m[4] - m[1] * m[3]) / det;
    return det;
}

inline bool rect_size_ok(int w, int h) { return w >= 1 && h >= 1 && w <= RECT_MAX_SIZE && h <= RECT_MAX_SIZE; }

// nrs_front_rectify_configure's checks; on success out[0] / out[1] hold the left / right eye's map parameters.  0, or -1 with the
// message in msg (NRS_ERR_INVALID)
inline int rect_check_configure(int src_w, int src_h, int dst_w, int dst_h, const nrs_rect_eye* left, const nrs_rect_eye* right, RectEye* out,
                                char* msg, size_t msg_len) {
    const char* who = "nrs_front_rectify_configure";
    if (!left || !right) { snprintf(msg, msg_len, RECT_MSG_NULL, who); return -1; }
    if (!rect_size_ok(src_w, src_h)) { snprintf(msg, msg_len, RECT_MSG_SIZE, who, "raw", src_w, src_h, RECT_MAX_SIZE); return -1; }
    if (!rect_size_ok(dst_w, dst_h)) { snprintf(msg, msg_len, RECT_MSG_SIZE, who, "rectified", dst_w, dst_h, RECT_MAX_SIZE); return -1; }
    for (int e = 0; e < 2; ++e) {
        const nrs_rect_eye* q = e ? right : left;
        const char* eye = e ? "right" : "left";
        for (int i = 0; i < 9; ++i) {
            if (!std::isfinite(q->K[i])) { snprintf(msg, msg_len, RECT_MSG_FINITE, who, eye, "K", i); return -1; }
            if (!std::isfinite(q->R[i])) { snprintf(msg, msg_len, RECT_MSG_FINITE, who, eye, "R", i); return -1; }
            if (!std::isfinite(q->P[i])) { snprintf(msg, msg_len, RECT_MSG_FINITE, who, eye, "P", i); return -1; }
        }
        for (int i = 0; i < 8; ++i)
            if (!std::isfinite(q->dist[i])) { snprintf(msg, msg_len, RECT_MSG_FINITE, who, eye, "dist", i); return -1; }
        double M[9];
        rect_mul3(q->P, q->R, M);
        RectEye& o = out[e];
        const double det = rect_inv3(M, o.iR);
        if (!(det != 0.0) || !std::isfinite(det)) { snprintf(msg, msg_len, RECT_MSG_DET, who, eye, det); return -1; }
        o.fx = q->K[0]; o.fy = q->K[4]; o.cx = q->K[2]; o.cy = q->K[5];
        for (int i = 0; i < 8; ++i) o.d[i] = q->dist[i];
    }
    return 0;
}

// nrs_front_process_stereo_raw's own checks: 0, -1 (NRS_ERR_INVALID) or -2 (NRS_ERR_STATE), the message in msg
inline int rect_check_raw(bool configured, int cfg_w, int cfg_h, int src_w, int src_h, char* msg, size_t msg_len) {
    const char* who = "nrs_front_process_stereo_raw";
    if (!configured) { snprintf(msg, msg_len, RECT_MSG_NONE, who); return -2; }
    if (src_w != cfg_w || src_h != cfg_h) { snprintf(msg, msg_len, RECT_MSG_RAW, who, src_w, src_h, cfg_w, cfg_h); return -1; }
    return 0;
}

// ---- the map of destination pixel (u, v): fp64, contraction off, every sum from the left ---------------------------------------
NRS_RECT_HD inline void rect_map_px(const RectEye& e, int u, int v, float* map_x, float* map_y) {
#pragma clang fp contract(off)
    const double du = (double)u, dv = (double)v;
    const double X = (e.iR[0] * du + e.iR[1] * dv) + e.iR[2];
    const double Y = (e.iR[3] * du + e.iR[4] * dv) + e.iR[5];
    const double W = (e.iR[6] * du + e.iR[7] * dv) + e.iR[8];
    const double x = X / W, y = Y / W;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * (x * y);
    const double k1 = e.d[0], k2 = e.d[1], p1 = e.d[2], p2 = e.d[3], k3 = e.d[4], k4 = e.d[5], k5 = e.d[6], k6 = e.d[7];
    const double kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2);
    const double xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2);
    const double yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2;
    *map_x = (float)(e.fx * xd + e.cx);
    *map_y = (float)(e.fy * yd + e.cy);
}

// ---- the fixed-point form of a map entry: what the remap reads, 8 bytes a pixel -------------------------------------------------
// ix, iy: the top-left tap, saturated to int16; frac = fy * 32 + fx, the 10-bit index of the pixel's four weights.  A non-finite entry is
// stored as the tap (-32768, -32768): all four taps lie outside every source, the pixel is 0
struct RectTap { int16_t ix, iy; uint16_t frac, pad; };
static_assert(sizeof(RectTap) == 8, "a tap is one 8-byte load");

NRS_RECT_HD inline int rect_fix1(float m) {       // rint(m * 32): fp32 product, brought into [-2^30, 2^30], rounded half to even
#pragma clang fp contract(off)
    float t = m * (float)RECT_TAB;
    t = t < -RECT_FIX_LIMIT ? -RECT_FIX_LIMIT : (t > RECT_FIX_LIMIT ? RECT_FIX_LIMIT : t);
    return (int)rintf(t);
}
NRS_RECT_HD inline int rect_sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

NRS_RECT_HD inline RectTap rect_fix(float map_x, float map_y) {
    RectTap t;
    t.pad = 0;
    if (!(fabsf(map_x) <= 3.402823466e38f) || !(fabsf(map_y) <= 3.402823466e38f)) {      // NaN or an infinity
        t.ix = t.iy = -32768; t.frac = 0;
        return t;
    }
    const int sx = rect_fix1(map_x), sy = rect_fix1(map_y);
    t.ix = (int16_t)rect_sat16(sx >> RECT_TAB_BITS);                                     // arithmetic shifts: floor
    t.iy = (int16_t)rect_sat16(sy >> RECT_TAB_BITS);
    t.frac = (uint16_t)((sy & (RECT_TAB - 1)) * RECT_TAB + (sx & (RECT_TAB - 1)));
    return t;
}

// the weights of taps (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1): exact integers, their sum is 2^15
NRS_RECT_HD inline void rect_weights(int frac, int* w) {
    const int fx = frac & (RECT_TAB - 1), fy = frac >> RECT_TAB_BITS;
    w[0] = (RECT_TAB - fx) * (RECT_TAB - fy) * 32;
    w[1] = fx * (RECT_TAB - fy) * 32;
    w[2] = (RECT_TAB - fx) * fy * 32;
    w[3] = fx * fy * 32;
}

// One rectified pixel, CH interleaved channels, from a sw x sh source with a row stride in bytes: out[c] = (sum_i w_i p_i + 2^14) >> 15, a
// tap outside the source contributes 0 (BORDER_CONSTANT 0)
template <int CH>
NRS_RECT_HD inline void rect_sample_px(const uint8_t* __restrict__ src, int stride, int sw, int sh, RectTap t, int* out) {
    int w[4];
    rect_weights(t.frac, w);
    const int x0 = t.ix, y0 = t.iy, x1 = x0 + 1, y1 = y0 + 1;
    const bool inx0 = x0 >= 0 && x0 < sw, inx1 = x1 >= 0 && x1 < sw, iny0 = y0 >= 0 && y0 < sh, iny1 = y1 >= 0 && y1 < sh;
    const uint8_t* r0 = src + (ptrdiff_t)(iny0 ? y0 : 0) * stride;
    const uint8_t* r1 = src + (ptrdiff_t)(iny1 ? y1 : 0) * stride;
    const ptrdiff_t o0 = (ptrdiff_t)(inx0 ? x0 : 0) * CH, o1 = (ptrdiff_t)(inx1 ? x1 : 0) * CH;      // (an outside tap reads pixel 0 and is weighted 0)
    if (!(inx0 && iny0)) w[0] = 0;
    if (!(inx1 && iny0)) w[1] = 0;
    if (!(inx0 && iny1)) w[2] = 0;
    if (!(inx1 && iny1)) w[3] = 0;
    for (int c = 0; c < CH; ++c)
        out[c] = (w[0] * r0[o0 + c] + w[1] * r0[o1 + c] + w[2] * r1[o0 + c] + w[3] * r1[o1 + c] + (1 << (RECT_ONE_BITS - 1))) >> RECT_ONE_BITS;
}

}  // namespace nrs
