// Host half of the frame resize (nrs_front.hip; include/nrs.h nrs_front_resize_configure / nrs_front_process_raw, DESIGN.md 4 "Frame
// resize") in plain C++: the refusals with their texts, the test for the 2 x 2 box branch, the tap tables of the general branch and the two
// pixel bodies.  The pixel bodies are the ones the kernel runs and the tables are computed here and uploaded: there is one definition.
// No HIP here: host/resize_check.cpp runs it under AddressSanitizer + UBSan (`make resize_check`).  tests/resize_oracle.py restates all of it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#ifdef __HIPCC__
#define NRS_RESIZE_HD __host__ __device__
#else
#define NRS_RESIZE_HD
#endif

namespace nrs {

constexpr int RESIZE_MAX_SIZE = 16384;           // either side of the raw or of the resized frame
constexpr int RESIZE_COEF_BITS = 11;             // OpenCV's INTER_RESIZE_COEF_BITS: the two weights of an axis sum to 2^11

// the refusals' texts: formats here, so that the stand-alone program and the library print the same words
constexpr const char* RESIZE_MSG_SIZE = "%s: %s size %d x %d (1 .. %d each)";
constexpr const char* RESIZE_MSG_NONE = "%s: no resize has been configured (nrs_front_resize_configure)";
constexpr const char* RESIZE_MSG_RAW = "%s: the raw frame is %d x %d, the configured one %d x %d";

inline bool resize_size_ok(int w, int h) { return w >= 1 && h >= 1 && w <= RESIZE_MAX_SIZE && h <= RESIZE_MAX_SIZE; }

// nrs_front_resize_configure's checks: 0, or -1 with the message in msg (NRS_ERR_INVALID)
inline int resize_check_configure(int src_w, int src_h, int dst_w, int dst_h, char* msg, size_t msg_len) {
    const char* who = "nrs_front_resize_configure";
    if (!resize_size_ok(src_w, src_h)) { snprintf(msg, msg_len, RESIZE_MSG_SIZE, who, "raw", src_w, src_h, RESIZE_MAX_SIZE); return -1; }
    if (!resize_size_ok(dst_w, dst_h)) { snprintf(msg, msg_len, RESIZE_MSG_SIZE, who, "resized", dst_w, dst_h, RESIZE_MAX_SIZE); return -1; }
    return 0;
}

// nrs_front_process_raw's own checks: 0, -1 (NRS_ERR_INVALID) or -2 (NRS_ERR_STATE), the message in msg
inline int resize_check_raw(bool configured, int cfg_w, int cfg_h, int src_w, int src_h, char* msg, size_t msg_len) {
    const char* who = "nrs_front_process_raw";
    if (!configured) { snprintf(msg, msg_len, RESIZE_MSG_NONE, who); return -2; }
    if (src_w != cfg_w || src_h != cfg_h) { snprintf(msg, msg_len, RESIZE_MSG_RAW, who, src_w, src_h, cfg_w, cfg_h); return -1; }
    return 0;
}

// the box branch: exactly half in both directions (what apps/endomapper.cc:65-69 asks for whenever both sizes are even)
inline bool resize_is_box(int src_w, int src_h, int dst_w, int dst_h) { return src_w == 2 * dst_w && src_h == 2 * dst_h; }

// ---- the taps of one axis ------------------------------------------------------------------------------------------------------
// destination index d of an axis dst <- src: the first source index and the fraction, before any border rule.  The product in double, one
// rounding to fp32, the floor of that, the difference in fp32
inline void resize_tap(int d, int dst, int src, int* s, float* f) {
#pragma clang fp contract(off)
    const double scale = 1.0 / ((double)dst / src);
    const float v = (float)(((double)d + 0.5) * scale - 0.5);
    const int i = (int)floorf(v);
    *s = i;
    *f = v - (float)i;
}

inline int resize_sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// the two fixed-point weights of a fraction: rounded half to even (the default rounding mode), each on its own
inline void resize_weights(float f, int16_t* w) {
#pragma clang fp contract(off)
    const float one = (float)(1 << RESIZE_COEF_BITS);
    w[0] = (int16_t)resize_sat16((int)rintf((1.f - f) * one));
    w[1] = (int16_t)resize_sat16((int)rintf(f * one));
}

// Both tables.  Columns: sx [dst_w], ax [dst_w][2]; a tap left of the image or on its last column has its fraction ZEROED, so that the
// second tap carries no weight and is never read.  Rows: sy [dst_h][2], by [dst_h][2]; the fraction stays and the two rows are clamped
// into the image instead -- at the border both weights then fall on one row, each truncated on its own, which is not one whole weight
inline void resize_build_taps(int src_w, int src_h, int dst_w, int dst_h, int32_t* sx, int16_t* ax, int32_t* sy, int16_t* by) {
    for (int d = 0; d < dst_w; ++d) {
        int s;
        float f;
        resize_tap(d, dst_w, src_w, &s, &f);
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= src_w - 1) { s = src_w - 1; f = 0.f; }
        sx[d] = s;
        resize_weights(f, ax + 2 * d);
    }
    for (int d = 0; d < dst_h; ++d) {
        int s;
        float f;
        resize_tap(d, dst_h, src_h, &s, &f);
        sy[2 * d] = s < 0 ? 0 : (s > src_h - 1 ? src_h - 1 : s);
        sy[2 * d + 1] = s + 1 < 0 ? 0 : (s + 1 > src_h - 1 ? src_h - 1 : s + 1);
        resize_weights(f, by + 2 * d);
    }
}

// ---- the pixel bodies ----------------------------------------------------------------------------------------------------------
NRS_RESIZE_HD inline int resize_sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// general branch, one channel: rows r = 0, 1 give D_r = S[r][sx] a0 + S[r][sx + 1] a1; the pixel is
// (((b0 (D_0 >> 4)) >> 16) + ((b1 (D_1 >> 4)) >> 16) + 2) >> 2.  int32 throughout (|D| <= 255 * 2^11, the products stay below 2^27)
NRS_RESIZE_HD inline int resize_blend(int s00, int s01, int s10, int s11, int a0, int a1, int b0, int b1) {
    const int d0 = s00 * a0 + s01 * a1, d1 = s10 * a0 + s11 * a1;
    return resize_sat8((((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2);
}

// box branch, one channel: the rounded mean of the 2 x 2 block
NRS_RESIZE_HD inline int resize_box(int s00, int s01, int s10, int s11) { return (s00 + s01 + s10 + s11 + 2) >> 2; }

// One resized pixel of the general branch, CH interleaved channels, from a source with a row stride in bytes: column tap x0 with weights
// a0, a1, rows y0, y1 (clamped already) with weights b0, b1.  A second column tap of weight 0 is the first one again: it is not read
template <int CH>
NRS_RESIZE_HD inline void resize_sample_px(const uint8_t* __restrict__ src, int stride, int x0, int a0, int a1, int y0, int y1, int b0, int b1,
                                           int* out) {
    const uint8_t* r0 = src + (ptrdiff_t)y0 * stride;
    const uint8_t* r1 = src + (ptrdiff_t)y1 * stride;
    const ptrdiff_t o0 = (ptrdiff_t)x0 * CH, o1 = (ptrdiff_t)(a1 ? x0 + 1 : x0) * CH;
    for (int c = 0; c < CH; ++c) out[c] = resize_blend(r0[o0 + c], r0[o1 + c], r1[o0 + c], r1[o1 + c], a0, a1, b0, b1);
}

// One resized pixel (x, y) of the box branch: source pixels (2x, 2y) .. (2x + 1, 2y + 1)
template <int CH>
NRS_RESIZE_HD inline void resize_box_px(const uint8_t* __restrict__ src, int stride, int x, int y, int* out) {
    const uint8_t* r0 = src + (ptrdiff_t)(2 * y) * stride + (ptrdiff_t)(2 * x) * CH;
    const uint8_t* r1 = r0 + stride;
    for (int c = 0; c < CH; ++c) out[c] = resize_box(r0[c], r0[CH + c], r1[c], r1[CH + c]);
}

}  // namespace nrs
