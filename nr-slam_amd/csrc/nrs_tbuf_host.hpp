// Host half of the resident TemporalBuffer (nrs_tbuf.hip; reference modules/map/temporal_buffer.cc:28-74) in plain C++: the ring of
// snapshots with the reference's pop rule, the argument checks with their texts, the filter of InsertSnapshotFromFrame, the packing of a
// snapshot into its one upload, the per-id reference counts (so the number of distinct ids is known without asking the device), the id
// span and the layout of the dense tables the device rebuilds per mapping call.  No HIP here: host/tbuf_check.cpp runs it under
// AddressSanitizer + UBSan (`make tbuf_check`).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <unordered_map>
#include <vector>
#include "nrs_map_host.hpp"

namespace nrs {

// The device addresses a row through its keypoint id: presence and row number are tables over [lowest id, highest id] of the held
// snapshots.  Ids are handed out in ascending order and a snapshot lives for 21 frames, so the span is a few thousand in practice;
// beyond TBUF_MAX_SPAN ids (16 MB of table) nrs_tbuf_insert refuses.
constexpr int64_t TBUF_MAX_SPAN = 1 << 22;
constexpr int TBUF_HEAD = 8;          // words in front of a slot's entries: pose (qx qy qz qw tx ty tz), deformation_magnitud
constexpr int TBUF_ENTRY = 7;         // words per entry: id | flags | x y | X Y Z, stored as sections id[m] flags[m] xy[2m] xyz[3m]
constexpr int TBUF_MIN_CAP = 256;     // entries of a slot at creation; doubled until a snapshot fits
constexpr uint32_t TBUF_HAS_LM = 0x100;   // flags = LandmarkStatus | TBUF_HAS_LM

inline size_t tb_slot_words(int cap) { return (size_t)TBUF_HEAD + (size_t)TBUF_ENTRY * (size_t)cap; }
inline bool tb_kept(int32_t status) { return status == 0 || status == 1; }   // GetKeypointsWithStatus({TRACKED_WITH_3D, TRACKED})

struct TbSnap {
    std::vector<int32_t> ids;         // the kept ids, in the frame's order (what the slot holds)
    int n_cand = 0;                   // kept entries whose status is TRACKED: GetTriangulationCandidatesIds().size() while this is the last
    int32_t id_lo = 0, id_hi = -1;    // lowest / highest kept id (id_hi < id_lo: none kept)
    float pose[7] = {0, 0, 0, 1, 0, 0, 0}, mag = 0.f;
    int slot = 0;                     // where its block lies on the device
};

struct TbufHost {
    int max_size = 20;                // TemporalBuffer::Options::max_buffer_size
    int cap = TBUF_MIN_CAP;           // entries per slot
    std::vector<TbSnap> snaps;        // oldest first, at most max_size + 1
    std::vector<int> free_slots;      // slots no snapshot lies in
    std::unordered_map<int32_t, int32_t> ref;   // id -> number of held snapshots with that id
    int n_slots() const { return max_size + 1; }
    int n_ids() const { return (int)ref.size(); }
    int n_candidates() const { return snaps.empty() ? 0 : snaps.back().n_cand; }
};

inline int tb_check_create(int max_buffer_size, char* msg, size_t msg_len) {
    if (max_buffer_size < 1 || max_buffer_size + 1 > MAP_MAXF) {
        snprintf(msg, msg_len, "nrs_tbuf_create: max_buffer_size %d outside [1, %d]", max_buffer_size, MAP_MAXF - 1);
        return -1;
    }
    return 0;
}

inline void tb_reset(TbufHost& h, int max_buffer_size) {
    h.max_size = max_buffer_size;
    h.snaps.clear();
    h.ref.clear();
    h.free_slots.clear();
    for (int s = h.n_slots() - 1; s >= 0; --s) h.free_slots.push_back(s);
}

struct TbInsertIn {
    int n;
    const int32_t* kp_id; const float* kp_xy; const float* lm_xyz; const int32_t* status; const uint8_t* has_lm; const float* pose_qt;
    float deform_mag;
};

// what an insert will do, decided before anything changes
struct TbPlan {
    int m = 0, n_cand = 0;            // kept entries, candidates among them
    int32_t id_lo = 0, id_hi = -1;
    bool pops = false;                // the oldest snapshot leaves first (size() > max_buffer_size)
    int slot = 0;                     // where the new block goes
    int new_cap = 0;                  // entries per slot afterwards (> cap: the slots are re-allocated first)
};

// 0, or -1 with the message in msg (the buffer is untouched either way).  `seen` is scratch.
inline int tb_plan_insert(const TbufHost& h, const TbInsertIn& a, TbPlan* p, std::vector<uint64_t>& seen, char* msg, size_t msg_len) {
    *p = TbPlan();
    if (a.n < 0 || !a.pose_qt || (a.n > 0 && (!a.kp_id || !a.kp_xy || !a.lm_xyz || !a.status))) {
        snprintf(msg, msg_len, "nrs_tbuf_insert: bad argument (null array with n = %d)", a.n);
        return -1;
    }
    bool any = false;
    for (int i = 0; i < a.n; ++i) {
        if (!tb_kept(a.status[i])) continue;
        const int32_t id = a.kp_id[i];
        if (id < 0) { snprintf(msg, msg_len, "nrs_tbuf_insert: negative keypoint id %d at slot %d", id, i); return -1; }
        if (!any || id < p->id_lo) p->id_lo = id;
        if (!any || id > p->id_hi) p->id_hi = id;
        any = true;
        ++p->m;
        p->n_cand += a.status[i] == 1;
    }
    // the span of the buffer as it will stand: without the snapshot that is popped, with the new one
    p->pops = (int)h.snaps.size() > h.max_size;
    int64_t lo = 0, hi = -1;
    bool held = false;
    auto widen = [&](int32_t a_lo, int32_t a_hi) {
        if (a_hi < a_lo) return;
        if (!held || a_lo < lo) lo = a_lo;
        if (!held || a_hi > hi) hi = a_hi;
        held = true;
    };
    for (size_t s = p->pops ? 1 : 0; s < h.snaps.size(); ++s) widen(h.snaps[s].id_lo, h.snaps[s].id_hi);
    if (any) widen(p->id_lo, p->id_hi);
    if (held && hi - lo + 1 > TBUF_MAX_SPAN) {
        snprintf(msg, msg_len, "nrs_tbuf_insert: the held ids would span [%lld, %lld]: more than the limit of %lld ids", (long long)lo, (long long)hi,
                 (long long)TBUF_MAX_SPAN);
        return -1;
    }
    if (any) {                                                     // two kept entries with one id: the reference's map would silently overwrite
        const size_t span = (size_t)((int64_t)p->id_hi - p->id_lo + 1);
        seen.assign((span + 63) / 64, 0);
        for (int i = 0; i < a.n; ++i) {
            if (!tb_kept(a.status[i])) continue;
            const size_t k = (size_t)(a.kp_id[i] - p->id_lo);
            if (seen[k >> 6] >> (k & 63) & 1) {
                snprintf(msg, msg_len, "nrs_tbuf_insert: duplicate keypoint id %d among the kept entries (second at slot %d)", a.kp_id[i], i);
                return -1;
            }
            seen[k >> 6] |= 1ull << (k & 63);
        }
    }
    p->slot = p->pops ? h.snaps.front().slot : (h.free_slots.empty() ? -1 : h.free_slots.back());
    if (p->slot < 0) { snprintf(msg, msg_len, "nrs_tbuf_insert: no free slot (internal)"); return -1; }
    p->new_cap = h.cap;
    while (p->new_cap < p->m) p->new_cap *= 2;
    return 0;
}

// the snapshot as its one upload: TBUF_HEAD + TBUF_ENTRY * m words
inline void tb_pack(const TbInsertIn& a, const TbPlan& p, uint32_t* dst) {
    float head[TBUF_HEAD];
    for (int k = 0; k < 7; ++k) head[k] = a.pose_qt[k];
    head[7] = a.deform_mag;
    memcpy(dst, head, sizeof(head));
    const size_t m = (size_t)p.m;
    uint32_t* id = dst + TBUF_HEAD;
    uint32_t* fl = id + m;
    uint32_t* xy = fl + m;
    uint32_t* xyz = xy + 2 * m;
    size_t j = 0;
    for (int i = 0; i < a.n; ++i) {
        if (!tb_kept(a.status[i])) continue;
        id[j] = (uint32_t)a.kp_id[i];
        fl[j] = (uint32_t)a.status[i] | ((!a.has_lm || a.has_lm[i]) ? TBUF_HAS_LM : 0u);
        memcpy(xy + 2 * j, a.kp_xy + 2 * (size_t)i, 8);
        memcpy(xyz + 3 * j, a.lm_xyz + 3 * (size_t)i, 12);
        ++j;
    }
}

// InsertSnapshotFromFrame's bookkeeping (temporal_buffer.cc:49-55): pop the oldest when size() > max, then insert
inline void tb_commit(TbufHost& h, const TbInsertIn& a, const TbPlan& p) {
    if (p.pops) {
        for (int32_t id : h.snaps.front().ids) {
            auto it = h.ref.find(id);
            if (it != h.ref.end() && --it->second == 0) h.ref.erase(it);
        }
        h.snaps.erase(h.snaps.begin());
    } else {
        h.free_slots.pop_back();
    }
    h.cap = p.new_cap;
    h.snaps.emplace_back();
    TbSnap& s = h.snaps.back();
    s.ids.reserve((size_t)p.m);
    for (int i = 0; i < a.n; ++i)
        if (tb_kept(a.status[i])) { s.ids.push_back(a.kp_id[i]); ++h.ref[a.kp_id[i]]; }
    s.n_cand = p.n_cand; s.id_lo = p.id_lo; s.id_hi = p.id_hi; s.slot = p.slot;
    for (int k = 0; k < 7; ++k) s.pose[k] = a.pose_qt[k];
    s.mag = a.deform_mag;
}

// [lo, hi] over the held snapshots; false when no snapshot holds an id
inline bool tb_span(const TbufHost& h, int32_t* lo, int32_t* hi) {
    bool held = false;
    for (const TbSnap& s : h.snaps) {
        if (s.id_hi < s.id_lo) continue;
        if (!held || s.id_lo < *lo) *lo = s.id_lo;
        if (!held || s.id_hi > *hi) *hi = s.id_hi;
        held = true;
    }
    return held;
}

// The dense tables the device rebuilds, in bytes from the start of the work buffer, each 256-byte aligned.  [0, zero_end) is cleared
// in one fill before the scatter: the presence / row table and everything that lies under a flag.
struct TbLayout {
    size_t row, has_kp, has_lm, kp_xy, lm_xyz, zero_end, status, row_id, poses, mag, bytes;
    TbLayout(size_t F, size_t n, size_t span) {
        auto al = [](size_t b) { return (b + 255) / 256 * 256; };
        row = 0;
        has_kp = al(4 * span);
        has_lm = has_kp + al(F * n);
        kp_xy = has_lm + al(F * n);
        lm_xyz = kp_xy + al(8 * F * n);
        zero_end = lm_xyz + al(12 * F * n);
        status = zero_end;
        row_id = status + al(4 * n);
        poses = row_id + al(4 * n);
        mag = poses + al(28 * F);
        bytes = mag + al(4 * F);
    }
};

// the checks of nrs_map_frame_tbuf that need no device; 0, or -1 (*state: the refusal is NRS_ERR_STATE, not NRS_ERR_INVALID)
inline int tb_check_map(const TbufHost& h, const void* cam, int cam_model, float rad_per_pixel, float rigidity_th, int index_snapshot,
                        const void* const outs[10], bool* state, char* msg, size_t msg_len) {
    *state = false;
    bool null_out = false;
    for (int i = 0; i < 10; ++i) null_out = null_out || !outs[i];
    if (!cam || null_out) { snprintf(msg, msg_len, "nrs_map_frame_tbuf: bad argument (null camera or output)"); return -1; }
    if (cam_model != 0 && cam_model != 1) { snprintf(msg, msg_len, "unknown camera model %d", cam_model); return -1; }
    if (!std::isfinite(rad_per_pixel) || !std::isfinite(rigidity_th)) {
        snprintf(msg, msg_len, "nrs_map_frame_tbuf: rad_per_pixel / rigidity_th must be finite");
        return -1;
    }
    if (h.snaps.empty()) { *state = true; snprintf(msg, msg_len, "nrs_map_frame_tbuf: the buffer holds no snapshot"); return -1; }
    if (index_snapshot < -1 || index_snapshot >= (int)h.snaps.size()) {
        snprintf(msg, msg_len, "nrs_map_frame_tbuf: index_snapshot %d outside [-1, %d)", index_snapshot, (int)h.snaps.size());
        return -1;
    }
    return 0;
}

}  // namespace nrs
