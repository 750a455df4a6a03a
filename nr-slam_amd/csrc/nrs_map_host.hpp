// Host half of nrs_map_frame (nrs_map.hip) in plain C++: the argument checks, the candidate count, the layout of the packed
// result and its unpacking.  No HIP here: host/map_check.cpp runs it under AddressSanitizer + UBSan (`make map_check`).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace nrs {

constexpr int MAP_MAXF = 21;     // snapshots of a TemporalBuffer: InsertSnapshotFromFrame pops when size() > 20, then inserts
constexpr int MAP_HDR = 8;       // words of the packed header: n_cand, n_rigid, n_deformable, mode, n_accepted, 3 spare
enum { MAP_MODE_NONE = 0, MAP_MODE_RIGID = 1, MAP_MODE_DEFORMABLE = 2 };

struct MapIn {
    const void* cam; int cam_model;
    int n_frames, n_ids;
    const float* poses; const uint8_t* has_kp; const float* kp_xy; const uint8_t* has_lm; const float* lm_xyz;
    const int32_t* last_status; const float* deform_mag;
    float rad_per_pixel, rigidity_th;
    int index_snapshot;
    const void* outs[10];        // every output pointer of the call
};

// 0, or -1 with the message in msg: the conditions of nrs_triangulate_batch (a candidate = an id whose last status is TRACKED (1)
// must have a keypoint in the last snapshot), plus the inputs that are new here.  *n_cand = GetTriangulationCandidatesIds().size().
inline int map_check_args(const MapIn& a, int* n_cand, char* msg, size_t msg_len) {
    *n_cand = 0;
    bool null_out = false;
    for (const void* o : a.outs) null_out = null_out || !o;
    if (!a.cam || a.n_frames < 1 || a.n_frames > MAP_MAXF || a.n_ids <= 0 || !a.poses || !a.has_kp || !a.kp_xy || !a.has_lm || !a.lm_xyz ||
        !a.last_status || !a.deform_mag || null_out) {
        snprintf(msg, msg_len, "nrs_map_frame: bad argument (at most %d buffered frames)", MAP_MAXF);
        return -1;
    }
    if (a.cam_model != 0 && a.cam_model != 1) { snprintf(msg, msg_len, "unknown camera model %d", a.cam_model); return -1; }
    if (!std::isfinite(a.rad_per_pixel) || !std::isfinite(a.rigidity_th)) {
        snprintf(msg, msg_len, "nrs_map_frame: rad_per_pixel / rigidity_th must be finite");
        return -1;
    }
    if (a.index_snapshot < -1 || a.index_snapshot >= a.n_frames) {
        snprintf(msg, msg_len, "nrs_map_frame: index_snapshot %d outside [-1, %d)", a.index_snapshot, a.n_frames);
        return -1;
    }
    const uint8_t* last = a.has_kp + (size_t)(a.n_frames - 1) * a.n_ids;
    for (int i = 0; i < a.n_ids; ++i)
        if (a.last_status[i] == 1) {
            if (!last[i]) { snprintf(msg, msg_len, "candidate %d has no keypoint in the last snapshot", i); return -1; }
            ++*n_cand;
        }
    return 0;
}

// The packed result, in 4-byte words, for n candidates: header | cand_id[n] | rigid_status[n] | deform_status[n] | rigid_xyz[3n] |
// deform_xyz[3n] | accepted_id[n] | accepted_xyz[3n]
struct MapLayout {
    size_t cand, r_st, d_st, r_xyz, d_xyz, a_id, a_xyz, words;
    explicit MapLayout(size_t n) {
        cand = MAP_HDR; r_st = cand + n; d_st = r_st + n; r_xyz = d_st + n; d_xyz = r_xyz + 3 * n; a_id = d_xyz + 3 * n; a_xyz = a_id + n;
        words = a_xyz + 3 * n;
    }
};

struct MapOut {
    int32_t* n_cand; int32_t* cand_ids; int32_t* rigid_status; float* rigid_xyz; int32_t* deform_status; float* deform_xyz;
    int32_t* counts;             // n_rigid, n_deformable, mode
    int32_t* n_accepted; int32_t* accepted_ids; float* accepted_xyz;
};

// 0, or -1 when the header contradicts the host's count (a device-side fault: nothing is copied)
inline int map_unpack(const int32_t* packed, int n_cand, const MapOut& o) {
    const MapLayout L((size_t)n_cand);
    const int n_acc = packed[4];
    if (packed[0] != n_cand || n_acc < 0 || n_acc > n_cand || packed[3] < MAP_MODE_NONE || packed[3] > MAP_MODE_DEFORMABLE) return -1;
    const size_t n = (size_t)n_cand;
    *o.n_cand = n_cand;
    o.counts[0] = packed[1]; o.counts[1] = packed[2]; o.counts[2] = packed[3];
    *o.n_accepted = n_acc;
    if (n) {
        memcpy(o.cand_ids, packed + L.cand, 4 * n);
        memcpy(o.rigid_status, packed + L.r_st, 4 * n);
        memcpy(o.deform_status, packed + L.d_st, 4 * n);
        memcpy(o.rigid_xyz, packed + L.r_xyz, 12 * n);
        memcpy(o.deform_xyz, packed + L.d_xyz, 12 * n);
    }
    if (n_acc) {
        memcpy(o.accepted_ids, packed + L.a_id, 4 * (size_t)n_acc);
        memcpy(o.accepted_xyz, packed + L.a_xyz, 12 * (size_t)n_acc);
    }
    return 0;
}

}  // namespace nrs
