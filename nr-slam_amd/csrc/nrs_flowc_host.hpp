// Host half of the flow-track clustering, nrs_dbscan_nd and nrs_flow_tracks_cluster (nrs_sinit.hip; include/nrs.h "f6", DESIGN.md 4
// "Flow-track clustering"), in plain C++: the argument checks with their texts, the eps rule, the dimension and length arithmetic, the
// layout of the clustering's rows (shared with f8) and of a call's scratch.  No HIP here: host/flowc_check.cpp runs it under
// AddressSanitizer + UBSan (`make flowc_check`).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "../../include/nrs.h"

namespace nrs {

constexpr int FLOWC_MAX_POINTS = NRS_DBSCAN_MAX_POINTS;
constexpr int FLOWC_MAX_DIM = NRS_DBSCAN_MAX_DIM;
constexpr int FLOWC_MIN_LENGTH = 2, FLOWC_MAX_LENGTH = FLOWC_MAX_DIM / 2 + 1;       // keypoints of a track: 2 .. 33
constexpr int FLOWC_MIN_POINTS = 10;                                                // monocular_map_initializer.cc:213
constexpr int FLOWC_TILE = 64;                                                      // candidate points of an LDS tile = bits of an adjacency word
constexpr int FLOWC_TILE_STRIDE = FLOWC_TILE + 1;                                   // floats between two coordinates of the dimension-major tile (odd)

// the refusals' texts: formats here, so that the stand-alone program and the library print the same words
constexpr const char* FLOWC_MSG_N = "%s: n = %d (0 .. %d)";
constexpr const char* FLOWC_MSG_DIM = "%s: dim = %d (1 .. %d)";
constexpr const char* FLOWC_MSG_LENGTH = "%s: length = %d keypoints (2 .. %d)";
constexpr const char* FLOWC_MSG_NULL = "%s: null pointer";
constexpr const char* FLOWC_MSG_EPS = "%s: eps = %g is not a positive finite number";
constexpr const char* FLOWC_MSG_MIN_POINTS = "%s: min_points = %d (at least 1)";

// coordinates of a track's point: one (dx, dy) per step between consecutive keypoints (:191-211)
inline int flowc_dim(int length) { return 2 * (length - 1); }
// eps = 0.1 * dim, stored in a float by the reference (:212) and widened again for the comparison
inline double flowc_eps(int dim) { return (double)(float)(0.1 * (double)dim); }

// 0, or -1 with the message in msg (NRS_ERR_INVALID).  A refusal reads no array
inline int dbscan_nd_check_args(int n, int dim, const void* data, double eps, int min_points, const void* label, const void* counts, char* msg,
                                size_t msg_len) {
    const char* who = "nrs_dbscan_nd";
    if (n < 0 || n > FLOWC_MAX_POINTS) { snprintf(msg, msg_len, FLOWC_MSG_N, who, n, FLOWC_MAX_POINTS); return -1; }
    if (dim < 1 || dim > FLOWC_MAX_DIM) { snprintf(msg, msg_len, FLOWC_MSG_DIM, who, dim, FLOWC_MAX_DIM); return -1; }
    if (!counts || (n > 0 && (!data || !label))) { snprintf(msg, msg_len, FLOWC_MSG_NULL, who); return -1; }
    if (!std::isfinite(eps) || !(eps > 0.0)) { snprintf(msg, msg_len, FLOWC_MSG_EPS, who, eps); return -1; }
    if (min_points < 1) { snprintf(msg, msg_len, FLOWC_MSG_MIN_POINTS, who, min_points); return -1; }
    return 0;
}

// flows_out is optional; eps and min_points are the rule's own
inline int flow_tracks_check_args(int n_tracks, int length, const void* tracks_xy, const void* label, const void* counts, char* msg, size_t msg_len) {
    const char* who = "nrs_flow_tracks_cluster";
    if (n_tracks < 0 || n_tracks > FLOWC_MAX_POINTS) { snprintf(msg, msg_len, FLOWC_MSG_N, who, n_tracks, FLOWC_MAX_POINTS); return -1; }
    if (length < FLOWC_MIN_LENGTH || length > FLOWC_MAX_LENGTH) { snprintf(msg, msg_len, FLOWC_MSG_LENGTH, who, length, FLOWC_MAX_LENGTH); return -1; }
    if (!counts || (n_tracks > 0 && (!tracks_xy || !label))) { snprintf(msg, msg_len, FLOWC_MSG_NULL, who); return -1; }
    return 0;
}

inline size_t flowc_padded(size_t bytes) { return (bytes + 255) / 256 * 256; }

// The clustering's device arrays for up to cap points, in bytes from the start of the piece, each on a 256-byte boundary: the adjacency rows
// (cap rows of W 64-bit words), the core mask, core flag / component label / raw label of a root by point, class sizes and ranks (noise
// first).  nrs_dbscan3d, nrs_init_stereo and the calls here carve the same piece: the rows do not know the points' dimension
struct DbRowsLayout {
    size_t W, adj, coremask, core, lab, rawid, size, rank, bytes;
    explicit DbRowsLayout(size_t cap) {
        W = (cap + 63) / 64;
        adj = 0;
        coremask = adj + flowc_padded(8 * cap * W);
        core = coremask + flowc_padded(8 * (size_t)(FLOWC_MAX_POINTS / 64));
        lab = core + flowc_padded(4 * cap);
        rawid = lab + flowc_padded(4 * cap);
        size = rawid + flowc_padded(4 * cap);
        rank = size + flowc_padded(4 * (cap + 1));
        bytes = rank + flowc_padded(4 * (cap + 1));
    }
};

// A call's scratch, in bytes: the ONE upload (the point count in a 256-byte header, then the caller's floats: n x dim coordinates, or
// n x length x 2 keypoints), the ONE download (counts[4] | label[n] | flows[n x dim], the last for tracks only), then the rows.  The
// clustering reads its points from the upload (nrs_dbscan_nd) or from the flows inside the download (nrs_flow_tracks_cluster)
struct FlowcScratch {
    size_t n, dim, in_floats, up_bytes, out_words, flows_word, m, in, out, rows, bytes;
    FlowcScratch(size_t n_, size_t dim_, size_t length /* 0: points, not tracks */) : n(n_), dim(dim_) {
        in_floats = length ? n * length * 2 : n * dim;
        up_bytes = 256 + 4 * in_floats;
        flows_word = 4 + n;
        out_words = flows_word + (length ? n * dim : 0);
        m = 0; in = 256;
        out = flowc_padded(up_bytes);
        rows = out + flowc_padded(4 * out_words);
        bytes = rows + DbRowsLayout(n).bytes;
    }
};

// queries a wave of k_db_neigh_nd carries (a workgroup of four waves owns four times as many): more reuse of a tile at the sizes that fill
// the chip anyway, more workgroups below (DESIGN.md 4 "Flow-track clustering")
inline int flowc_queries_per_wave(int n) { return n <= 1024 ? 1 : (n <= 4096 ? 2 : 4); }

}  // namespace nrs
