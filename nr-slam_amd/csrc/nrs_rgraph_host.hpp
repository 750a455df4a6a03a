// Host half of the device-resident RegularizationGraph (nrs_rgraph.hip) in plain C++: the layout of a GetEdges block, what fits a
// row's sort buffer in LDS and what each of the two passes stages, the form an update takes, when GetEdges scans full-matrix mirrors,
// the scratch plan of the device walk, the argument checks with their texts, and min_weight / the far-distance bound from sigma.
// No HIP here: host/rgraph_check.cpp runs it under AddressSanitizer + UBSan (`make rgraph_check`).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "nrs_rgraph.hpp"

#ifdef __HIPCC__
#define NRS_RG_HD __host__ __device__
#else
#define NRS_RG_HD
#endif

namespace nrs {

// InterpolationWeight (utilities/geometry_toolbox.cc:26-28): float argument, exp evaluated in double and rounded to float (the
// definition shared with the oracle and nrs_track.hip, DESIGN.md "weights").  The one definition of the graph: host and kernels.
NRS_RG_HD inline float rg_weight(float d, float sigma) {
#pragma clang fp contract(off)
    const float arg = -(d * d) / (2.0f * sigma * sigma);
    return (float)exp((double)arg);
}
// regularization_graph.cc:29 / SetSigma :33-36 (float * double literal -> float argument)
inline float rg_min_weight(float sigma) { return rg_weight((float)((double)sigma * 1.5), sigma); }
// beyond 1.5 sigma (1 + 1e-4) a weight is below min_weight for sure; inside, the exact value decides (k_rg_get_edges)
inline float rg_far_distance(float sigma) { return (float)((double)sigma * 1.5 * (1.0 + 1e-4)); }

// ---- one GetEdges block, on the device and in the pinned staging area alike, in 4-byte words from its start:
// count[n_ids] | col | status | weight | first distance (each n_ids x cap_per_point) | overflow word
struct RgListLayout {
    int n_ids, stride;
    size_t col, status, w, d0, overflow;
    RgListLayout(int n_ids_, int cap_per_point) : n_ids(n_ids_), stride(cap_per_point) {
        const size_t no = (size_t)n_ids * (size_t)cap_per_point;
        col = (size_t)n_ids; status = col + no; w = col + 2 * no; d0 = col + 3 * no; overflow = col + 4 * no;
    }
    size_t list_bytes() const { return 4 * overflow; }             // what a caller reads
    size_t bytes() const { return 4 * (overflow + 1); }            // ... and the overflow word behind it
    RgDeviceLists view(const void* base) const {
        const int* b = static_cast<const int*>(base);
        return RgDeviceLists{n_ids, stride, b, b + col, b + status, reinterpret_cast<const float*>(b + w), reinterpret_cast<const float*>(b + d0)};
    }
};

// ---- the sort buffer of a row lives in LDS: 8 bytes per staged candidate (a power of two of them) next to 4 KB of histogram and
// 512 bytes of slack
constexpr int RG_SLACK = 1024;   // candidates staged beyond out_cap (the population of the bin the cut falls into)
inline size_t rg_cand_limit(size_t lds_bytes) {
    size_t m = 512;
    while (8 * (m << 1) + 4096 + 512 <= lds_bytes) m <<= 1;
    return m;
}
// what a row stages in the selecting pass: the prefix and one histogram bin's population, never more than the row has
inline int rg_first_pass_cands(int cap, int cap_per_point) { return (int)std::min<int64_t>(cap, (int64_t)cap_per_point + RG_SLACK); }
// pass 0: the selecting form; pass 1: every survivor of a row staged (many equal distances overflowed a bin)
struct RgPass { int cand_cap; size_t pad, lds_bytes; };            // candidates a row may stage; the power of two >= 512 the long-list sort runs over; dynamic LDS
inline RgPass rg_pass_plan(int pass, int cap, int cap_per_point, size_t cand_limit) {
    RgPass p;
    p.cand_cap = pass == 0 ? rg_first_pass_cands(cap, cap_per_point) : (int)std::min<size_t>({(size_t)cap, (size_t)12000, cand_limit});
    p.pad = 512;
    while (p.pad < (size_t)p.cand_cap) p.pad <<= 1;
    p.lds_bytes = 8 * p.pad;
    return p;
}
// rg_max_cap_per_point; `lowered`: NRS_RG_MAX_CAP gives a lower limit (so that the tests reach the callers' "ran off at the limit" refusal)
inline int rg_cap_limit(int cap, size_t cand_limit, bool lowered, int lower) {
    int lim = std::min(cap, (int)cand_limit - RG_SLACK);
    if (lowered) lim = std::max(1, std::min(lim, lower));
    return lim;
}

// ---- UpdateVertex of a list: the one-pass form over the stored triangle when a large part of the points is listed, each once
// (slot[v] = place of v in the list, -1: not listed); the per-vertex form otherwise.  The ids have passed rg_check_ids.
inline bool rg_update_one_pass(int cap, int n_ids, const int32_t* ids, std::vector<int>& slot) {
    if ((size_t)n_ids * 4 < (size_t)cap) return false;
    slot.assign((size_t)cap, -1);
    for (int a = 0; a < n_ids; ++a) {
        if (slot[ids[a]] >= 0) return false;
        slot[ids[a]] = a;
    }
    return true;
}

// ---- GetEdges of many rows of a graph that is not small scans full symmetric copies of status and longest distance (k_rg_mirror);
// no_mirror: the NRS_RG_NO_MIRROR switch
inline bool rg_use_mirror(int n_ids, int cap, bool no_mirror) { return (int64_t)n_ids * 8 >= cap && cap >= 512 && !no_mirror; }

// ---- the device walk's scratch (rg_walk), bytes from the start of its buffer, each part 256-byte aligned.  [lost, lost + zero_bytes)
// is cleared in one fill before the passes: the lost flags and the change counters (one per pass and one for the final pass).
constexpr int RG_WALK_MAX = 11;          // connections a walk accepts (OPT:252-279)
constexpr int RG_WALK_PASSES = 96;
struct RgWalkPlan {
    size_t code, node, acc, n_acc, w, d0, ended, lost, changed, total, zero_bytes;
    RgWalkPlan(size_t n_map, size_t n) {
        auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
        code = 0;
        node = code + al(4 * n_map);
        acc = node + al(n);
        n_acc = acc + al(4 * RG_WALK_MAX * n);
        w = n_acc + al(4 * n);
        d0 = w + al(4 * RG_WALK_MAX * n);
        ended = d0 + al(4 * RG_WALK_MAX * n);
        lost = ended + al(n);
        changed = lost + al(n_map);
        total = changed + al(4 * (RG_WALK_PASSES + 1));
        zero_bytes = changed - lost + 4 * (RG_WALK_PASSES + 1);
    }
};

// ---- argument checks: 0, or -1 with the refusal in msg (NRS_ERR_INVALID)
inline int rg_check_ids(int cap, int n, const int32_t* ids, const char* what, char* msg, size_t msg_len) {
    if (n < 0 || (n > 0 && !ids)) { snprintf(msg, msg_len, "%s: null / negative id list", what); return -1; }
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= cap) { snprintf(msg, msg_len, "%s: point index %d outside [0, %d)", what, ids[i], cap); return -1; }
    return 0;
}
constexpr int RG_MAX_CAPACITY = 200000;
inline int rg_check_create(int capacity, float sigma, float stretch_th, char* msg, size_t msg_len) {
    if (capacity <= 1 || capacity > RG_MAX_CAPACITY || !(sigma > 0) || !(stretch_th > 0)) { snprintf(msg, msg_len, "nrs_rgraph_create: bad argument"); return -1; }
    return 0;
}
inline int rg_check_resize(int cap, int new_capacity, char* msg, size_t msg_len) {
    if (new_capacity < cap) { snprintf(msg, msg_len, "nrs_rgraph_resize: capacity %d is below the graph's %d", new_capacity, cap); return -1; }
    if (new_capacity <= 1 || new_capacity > RG_MAX_CAPACITY) {
        snprintf(msg, msg_len, "nrs_rgraph_resize: capacity %d is past the limit of %d points (nrs_rgraph_create: bad argument)", new_capacity, RG_MAX_CAPACITY);
        return -1;
    }
    return 0;
}
// GetEdges behind every entry point.  ids_on_device: the caller's kernels made the ids and `ids` is not read
inline int rg_check_get_edges(int cap, int n_ids, const int32_t* ids, bool ids_on_device, int cap_per_point, char* msg, size_t msg_len) {
    if (ids_on_device) {
        if (n_ids <= 0 || n_ids > cap) { snprintf(msg, msg_len, "GetEdges: %d device-side ids for %d points", n_ids, cap); return -1; }
    } else if (rg_check_ids(cap, n_ids, ids, "GetEdges", msg, msg_len) != 0) return -1;
    if (cap_per_point <= 0) { snprintf(msg, msg_len, "GetEdges: cap_per_point must be positive"); return -1; }
    return 0;
}
inline int rg_check_fits_lds(int cap, int cap_per_point, size_t cand_limit, int lds_bytes, char* msg, size_t msg_len) {
    if ((size_t)rg_first_pass_cands(cap, cap_per_point) > cand_limit) {
        snprintf(msg, msg_len, "GetEdges: cap_per_point %d needs more than the %zu candidates per row that fit this device's %d bytes of LDS", cap_per_point,
                 cand_limit, lds_bytes);
        return -1;
    }
    return 0;
}
// nrs_rgraph_get_edges' own arguments, ahead of the above
inline int rg_check_get_edges_abi(int n_ids, int cap_per_point, bool outputs, char* msg, size_t msg_len) {
    if (cap_per_point <= 0 || (n_ids > 0 && !outputs)) { snprintf(msg, msg_len, "nrs_rgraph_get_edges: bad argument"); return -1; }
    return 0;
}

}  // namespace nrs
