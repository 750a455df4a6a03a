// Host half of nrs_point_reuse (nrs_klt.hip) in plain C++: the argument checks with their texts, the rotation of the pose in the
// frame loop's float32 form, the lost-id flags, the upload and packed-result layouts and the unpacking.  No HIP here:
// host/reuse_check.cpp runs it under AddressSanitizer + UBSan (`make reuse_check`).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace nrs {

constexpr int REUSE_MAX_MAP = 1 << 20;   // the archive is dense by key and a candidate's key is its map index (nrs_klt_archive_templates)
constexpr int REUSE_HDR = 4;             // words of the packed header: n_cand, n_reused, n_new, 1 spare

struct ReuseArgs {
    const void* cam; int cam_model;
    const float* pose_qt;
    int w, h;
    int n_map; const float* map_pos; const int32_t* frame_slot;
    int n_slots; const int32_t* slot_status;
    int n_lost; const int32_t* lost_ids;
    const void* outs[8];         // every output pointer of the call
};

// 0, or -1 with the message in msg (NRS_ERR_INVALID)
inline int reuse_check_args(const ReuseArgs& a, char* msg, size_t msg_len) {
    bool null_out = false;
    for (const void* o : a.outs) null_out = null_out || !o;
    if (!a.cam || !a.pose_qt || null_out) { snprintf(msg, msg_len, "nrs_point_reuse: null pointer"); return -1; }
    if (a.cam_model != 0 && a.cam_model != 1) { snprintf(msg, msg_len, "unknown camera model %d", a.cam_model); return -1; }
    if (a.n_map < 0 || a.n_slots < 0 || a.n_lost < 0 || a.w <= 0 || a.h <= 0) {
        snprintf(msg, msg_len, "nrs_point_reuse: negative count or empty image (n_map %d, n_slots %d, n_lost %d, %d x %d)", a.n_map, a.n_slots, a.n_lost, a.w, a.h);
        return -1;
    }
    if (a.n_map >= REUSE_MAX_MAP) {
        snprintf(msg, msg_len, "nrs_point_reuse: n_map %d is not below %d (a candidate's archive key is its map index: keys below %d)", a.n_map, REUSE_MAX_MAP, REUSE_MAX_MAP);
        return -1;
    }
    if ((a.n_map > 0 && (!a.map_pos || !a.frame_slot)) || (a.n_slots > 0 && !a.slot_status) || (a.n_lost > 0 && !a.lost_ids)) {
        snprintf(msg, msg_len, "nrs_point_reuse: null pointer");
        return -1;
    }
    for (int i = 0; i < a.n_map; ++i)
        if (a.frame_slot[i] >= a.n_slots) { snprintf(msg, msg_len, "nrs_point_reuse: frame_slot[%d] = %d, the frame has %d slots", i, a.frame_slot[i], a.n_slots); return -1; }
    for (int i = 0; i < a.n_lost; ++i)
        if (a.lost_ids[i] < 0 || a.lost_ids[i] >= a.n_map) { snprintf(msg, msg_len, "nrs_point_reuse: lost id %d outside the map (%d points)", a.lost_ids[i], a.n_map); return -1; }
    return 0;
}

// R of a unit quaternion (x y z w), row-major, every entry the float32 expression of nrs_frame_loop.se3f_act (no contraction)
inline void reuse_rotation(const float* q, float* R) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.f - 2.f * (y * y + z * z); R[1] = 2.f * (x * y - z * w);       R[2] = 2.f * (x * z + y * w);
    R[3] = 2.f * (x * y + z * w);       R[4] = 1.f - 2.f * (x * x + z * z); R[5] = 2.f * (y * z - x * w);
    R[6] = 2.f * (x * z - y * w);       R[7] = 2.f * (y * z + x * w);       R[8] = 1.f - 2.f * (x * x + y * y);
}

// The upload, in bytes: map_pos[3 n_map] f32 | frame_slot[n_map] i32 | slot_status[n_slots] i32 | lost[n_map] u8 (1 = listed lost)
struct ReuseUpload {
    size_t pos, slot, status, lost, bytes;
    ReuseUpload(size_t n_map, size_t n_slots) {
        pos = 0; slot = pos + 12 * n_map; status = slot + 4 * n_map; lost = status + 4 * n_slots; bytes = lost + n_map;
    }
};

// fills the whole upload (buf: ReuseUpload::bytes bytes); the arguments have passed reuse_check_args
inline void reuse_pack_upload(const ReuseArgs& a, char* buf) {
    const ReuseUpload U((size_t)a.n_map, (size_t)a.n_slots);
    if (a.n_map) { memcpy(buf + U.pos, a.map_pos, 12 * (size_t)a.n_map); memcpy(buf + U.slot, a.frame_slot, 4 * (size_t)a.n_map); }
    if (a.n_slots) memcpy(buf + U.status, a.slot_status, 4 * (size_t)a.n_slots);
    if (a.n_map) memset(buf + U.lost, 0, (size_t)a.n_map);
    for (int i = 0; i < a.n_lost; ++i) buf[U.lost + (size_t)a.lost_ids[i]] = 1;
}

// The device scratch, in 4-byte words, for a map of n points: header | cand_id[n] | seed_xy[2n] | xy[2n] | status[n] | new_key[n]
struct ReuseScratch {
    size_t cand, seed, xy, status, new_key, words;
    explicit ReuseScratch(size_t n) {
        cand = REUSE_HDR; seed = cand + n; xy = seed + 2 * n; status = xy + 2 * n; new_key = status + n; words = new_key + n;
    }
};

// The packed result, in 4-byte words, for n candidates: header | cand_id[n] | seed_xy[2n] | xy[2n] | status[n] | accepted[n]
struct ReuseLayout {
    size_t cand, seed, xy, status, accepted, words;
    explicit ReuseLayout(size_t n) {
        cand = REUSE_HDR; seed = cand + n; xy = seed + 2 * n; status = xy + 2 * n; accepted = status + n; words = accepted + n;
    }
};

struct ReuseOut {
    int32_t* n_cand; int32_t* cand_id; float* seed_xy; float* xy; int32_t* status; int32_t* accepted; int32_t* n_reused; int32_t* n_new;
};

// 0, or -1 when the header contradicts the host's count (a device-side fault: nothing is copied)
inline int reuse_unpack(const int32_t* packed, int n_cand, const ReuseOut& o) {
    const ReuseLayout L((size_t)n_cand);
    const int n_reused = packed[1], n_new = packed[2];
    if (packed[0] != n_cand || n_reused < 0 || n_reused > n_cand || n_new < 0 || n_new > n_reused) return -1;
    const size_t n = (size_t)n_cand;
    *o.n_cand = n_cand; *o.n_reused = n_reused; *o.n_new = n_new;
    if (n) {
        memcpy(o.cand_id, packed + L.cand, 4 * n);
        memcpy(o.seed_xy, packed + L.seed, 8 * n);
        memcpy(o.xy, packed + L.xy, 8 * n);
        memcpy(o.status, packed + L.status, 4 * n);
        memcpy(o.accepted, packed + L.accepted, 4 * n);
    }
    return 0;
}

}  // namespace nrs
