// Host half of f8, nrs_dbscan3d and nrs_init_stereo (nrs_sinit.hip), in plain C++: the argument checks with their texts, the layout of the
// packed result, its unpacking with the header's sanity test, the verdict and the median depth.  No HIP here: host/sinit_check.cpp runs it
// under AddressSanitizer + UBSan (`make sinit_check`).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "../../include/nrs.h"

namespace nrs {

constexpr int SINIT_MAX = NRS_DBSCAN_MAX_POINTS;   // an adjacency row is n bits: 16384 points are 32 MiB of rows
constexpr int SINIT_HDR = 8;                       // words of the packed header: n_matched, n_gated, n_clusters, n_noise, n_selected, size of label 0, 2 spare

// 0, or -1 with the message in msg (NRS_ERR_INVALID)
inline int dbscan_check_args(int n, const void* xyz, double eps, int min_points, const void* label, const void* counts, char* msg, size_t msg_len) {
    if (n < 0 || n > SINIT_MAX) { snprintf(msg, msg_len, "nrs_dbscan3d: n = %d (0 .. %d)", n, SINIT_MAX); return -1; }
    if (!counts || (n > 0 && (!xyz || !label))) { snprintf(msg, msg_len, "nrs_dbscan3d: null pointer"); return -1; }
    if (!std::isfinite(eps) || !(eps > 0.0)) { snprintf(msg, msg_len, "nrs_dbscan3d: eps = %g is not a positive finite number", eps); return -1; }
    if (min_points < 1) { snprintf(msg, msg_len, "nrs_dbscan3d: min_points = %d (at least 1)", min_points); return -1; }
    return 0;
}

inline void sinit_options_init(nrs_init_stereo_options* o) {
    memset(o, 0, sizeof *o);
    o->struct_size = (uint32_t)sizeof *o;
    o->bf = 3886.37f;                              // stereo_pattern_matching's baseline_ as tracking.cc:226 passes it
    o->z_min = 35.5f; o->z_max = 70.5f;            // tracking.cc:229-233
    o->eps = 2.5; o->min_points = 5;               // tracking.cc:250
    o->noise_competes = 1;
}

// the checks of nrs_init_stereo that are its own (the matcher's follow): 0, or -1 with the message in msg
inline int sinit_check_args(const nrs_init_stereo_options* opt, const nrs_init_stereo_result* out, int n, char* msg, size_t msg_len) {
    if (!opt || !out) { snprintf(msg, msg_len, "nrs_init_stereo: null pointer"); return -1; }
    if (opt->struct_size != sizeof(nrs_init_stereo_options)) {
        snprintf(msg, msg_len, "nrs_init_stereo: options struct_size %u, this library's is %zu", opt->struct_size, sizeof(nrs_init_stereo_options));
        return -1;
    }
    if (out->struct_size != sizeof(nrs_init_stereo_result)) {
        snprintf(msg, msg_len, "nrs_init_stereo: result struct_size %u, this library's is %zu", out->struct_size, sizeof(nrs_init_stereo_result));
        return -1;
    }
    if (n > SINIT_MAX) { snprintf(msg, msg_len, "nrs_init_stereo: n = %d keypoints (at most %d)", n, SINIT_MAX); return -1; }
    if (!std::isfinite(opt->eps) || !(opt->eps > 0.0)) { snprintf(msg, msg_len, "nrs_init_stereo: eps = %g is not a positive finite number", opt->eps); return -1; }
    if (opt->min_points < 1) { snprintf(msg, msg_len, "nrs_init_stereo: min_points = %d (at least 1)", opt->min_points); return -1; }
    if (!(opt->z_min < opt->z_max)) { snprintf(msg, msg_len, "nrs_init_stereo: the depth gate (%g, %g) is empty", (double)opt->z_min, (double)opt->z_max); return -1; }
    return 0;
}

// The upload, in bytes: left[w h] packed | right[w h] packed | xy[2n] f32, each piece on a 256-byte boundary
struct SinitUpload {
    size_t w, h, n, left, right, xy, bytes;
    SinitUpload(size_t w_, size_t h_, size_t n_) : w(w_), h(h_), n(n_) {
        const size_t img = (w * h + 255) / 256 * 256;
        left = 0; right = img; xy = 2 * img; bytes = xy + 8 * n;
    }
};

// fills the upload (buf: SinitUpload::bytes bytes; the gaps behind the images are zeroed); strides in bytes, at least w
inline void sinit_pack_upload(const SinitUpload& U, const uint8_t* left, size_t stride_l, const uint8_t* right, size_t stride_r, const float* xy, char* buf) {
    for (size_t y = 0; y < U.h; ++y) {
        memcpy(buf + U.left + y * U.w, left + y * stride_l, U.w);
        memcpy(buf + U.right + y * U.w, right + y * stride_r, U.w);
    }
    const size_t img = U.w * U.h;
    memset(buf + U.left + img, 0, U.right - img);
    memset(buf + U.right + img, 0, U.xy - U.right - img);
    if (U.n) memcpy(buf + U.xy, xy, 8 * U.n);
}

// The packed result, in 4-byte words, for n keypoints:
//   header | xyz[3n] f32 | match_status[n] | code[n] | raw_label[n] | label[n] | selected[n] | selected_xyz[3n] f32
struct SinitLayout {
    size_t xyz, status, code, raw, label, selected, sel_xyz, words;
    explicit SinitLayout(size_t n) {
        xyz = SINIT_HDR; status = xyz + 3 * n; code = status + n; raw = code + n; label = raw + n; selected = label + n; sel_xyz = selected + n;
        words = sel_xyz + 3 * n;
    }
};

// nth_element at n / 2 of the selected depths (tracking.cc:239-248); NaN for an empty selection.  z: every third float from z0
inline float sinit_median_depth(const float* sel_xyz, int n_selected) {
    if (n_selected <= 0) return std::numeric_limits<float>::quiet_NaN();
    std::vector<float> z((size_t)n_selected);
    for (int i = 0; i < n_selected; ++i) z[(size_t)i] = sel_xyz[3 * (size_t)i + 2];
    std::nth_element(z.begin(), z.begin() + n_selected / 2, z.end());
    return z[(size_t)(n_selected / 2)];
}

// the scalars of a result for n = 0 keypoints or before anything ran: nothing matched, nothing gated -> verdict 1
inline void sinit_clear(nrs_init_stereo_result* o) {
    o->verdict = 1;
    o->n_matched = o->n_gated = o->n_clusters = o->n_noise = o->n_selected = 0;
    o->median_depth = std::numeric_limits<float>::quiet_NaN();
}

// 0, or -1 when the header contradicts itself or n (a device-side fault: nothing is copied)
inline int sinit_unpack(const int32_t* packed, int n, nrs_init_stereo_result* o) {
    const SinitLayout L((size_t)n);
    const int n_matched = packed[0], n_gated = packed[1], n_clusters = packed[2], n_noise = packed[3], n_selected = packed[4];
    if (n_matched < 0 || n_matched > n || n_gated < 0 || n_gated > n_matched || n_clusters < 0 || n_clusters > n_gated || n_noise < 0 ||
        n_noise > n_gated || n_selected < 0 || n_selected > n_gated || packed[5] != n_selected)      // (words 4 and 5: the selection's length and the size of label 0, counted apart)
        return -1;
    o->n_matched = n_matched; o->n_gated = n_gated; o->n_clusters = n_clusters; o->n_noise = n_noise; o->n_selected = n_selected;
    o->verdict = n_gated == 0 ? 1 : 0;
    const float* pf = reinterpret_cast<const float*>(packed);
    o->median_depth = sinit_median_depth(pf + L.sel_xyz, n_selected);
    const size_t m = (size_t)n, s = (size_t)n_selected;
    if (m) {
        if (o->xyz) memcpy(o->xyz, packed + L.xyz, 12 * m);
        if (o->match_status) memcpy(o->match_status, packed + L.status, 4 * m);
        if (o->code) memcpy(o->code, packed + L.code, 4 * m);
        if (o->raw_label) memcpy(o->raw_label, packed + L.raw, 4 * m);
        if (o->label) memcpy(o->label, packed + L.label, 4 * m);
    }
    if (s) {
        if (o->selected) memcpy(o->selected, packed + L.selected, 4 * s);
        if (o->selected_xyz) memcpy(o->selected_xyz, packed + L.sel_xyz, 12 * s);
    }
    return 0;
}

}  // namespace nrs
