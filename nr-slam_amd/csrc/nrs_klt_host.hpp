// Host half of the tracker's template stores (nrs_klt.hip) in plain C++: what one template entry holds in each of its arrays, the rule
// by which a store grows, and the argument checks of nrs_klt_archive_templates with their texts and its "last occurrence of a key
// stands" list.  No HIP here: host/klt_check.cpp runs it under AddressSanitizer + UBSan (`make klt_check`).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace nrs {

constexpr int KW = 21, KA = KW * KW;               // the reference's 21 x 21 window (SLAM/system.cc:78) and its pixel count

// A template entry is `levels` levels of four arrays, level-major inside the entry, entries back to back: the window's intensities x 32
// (i16), its derivative pairs (i16, i16), meanI and meanI2 (f32, f32) and the valid byte.
constexpr int KLT_ARRAYS = 4;
constexpr size_t KLT_LEVEL_ELEMS[KLT_ARRAYS] = {(size_t)KA, (size_t)KA, 2, 1};      // elements per level: grey, gradient pairs, means, valid
constexpr size_t KLT_ELEM_BYTES[KLT_ARRAYS] = {2, 4, 4, 1};
inline size_t klt_entry_bytes(int array, int levels) { return KLT_LEVEL_ELEMS[array] * KLT_ELEM_BYTES[array] * (size_t)levels; }
// ... and a fifth, one item per entry whatever the level count: the tracker's reference point (x, y as f32) or the archive's "has" byte
constexpr size_t KLT_XY_BYTES = 8, KLT_HAS_BYTES = 1;

// capacity a store is given when `want` entries no longer fit: half as much again, never below 256
inline int klt_grow_capacity(int want) { return std::max(want + want / 2, 256); }

// The archive is DENSE by key (a map point id indexes its slot: no lookup on the device): KA x levels x 6 bytes per key, so the key range is bounded --
// 2^20 map points = 2.9 GB at 5 levels; the reference's maps hold thousands (include/nrs.h nrs_klt_archive_templates)
constexpr int NRS_KLT_ARCHIVE_MAX_KEY = 1 << 20;

// The checks of nrs_klt_archive_templates in their order.  0 (kmax: the largest key, -1 for an empty list, which asks for no tracker
// state); -1 with the message in msg (NRS_ERR_INVALID); -2 with the message in msg (NRS_ERR_STATE).  n_stored: templates the tracker holds
inline int klt_archive_check(int n, const int32_t* slots, const int32_t* keys, bool has_state, int n_stored, int* kmax, char* msg, size_t msg_len) {
    *kmax = -1;
    if (n < 0 || (n > 0 && (!slots || !keys))) { snprintf(msg, msg_len, "nrs_klt_archive_templates: bad argument"); return -1; }
    if (n == 0) return 0;
    if (!has_state) { snprintf(msg, msg_len, "nrs_klt_archive_templates: no tracker state"); return -2; }
    for (int i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= n_stored) { snprintf(msg, msg_len, "nrs_klt_archive_templates: slot %d out of range", slots[i]); return -1; }
        if (keys[i] < 0 || keys[i] >= NRS_KLT_ARCHIVE_MAX_KEY) {
            snprintf(msg, msg_len, "nrs_klt_archive_templates: key %d out of range (the archive is dense by key: keys below %d)", keys[i], NRS_KLT_ARCHIVE_MAX_KEY);
            return -1;
        }
        *kmax = std::max(*kmax, keys[i]);
    }
    return 0;
}

// a key listed more than once: its LAST occurrence stands (the copies run side by side: two of them must not share a destination).  The
// lists have passed klt_archive_check, kmax is its; the survivors keep their order
inline void klt_archive_last_stands(int n, const int32_t* slots, const int32_t* keys, int kmax, std::vector<int>& u_slot, std::vector<int>& u_key) {
    u_slot.clear(); u_key.clear();
    std::vector<int> last((size_t)kmax + 1, -1);
    for (int i = 0; i < n; ++i) last[keys[i]] = i;
    for (int i = 0; i < n; ++i) if (last[keys[i]] == i) { u_slot.push_back(slots[i]); u_key.push_back(keys[i]); }
}

}  // namespace nrs
