// Stand-alone check of the host half of the resident TemporalBuffer (csrc/nrs_tbuf_host.hpp) under AddressSanitizer + UBSan:
// `make tbuf_check` (builds and runs it).  No HIP, no library: hand-made frames, every array exactly as long as the interface says, the
// ring held against a brute-force restatement of temporal_buffer.cc:28-74 (a list of id sets).
#include <algorithm>
#include <cstdio>
#include <set>
#include <vector>
#include "../csrc/nrs_tbuf_host.hpp"

using namespace nrs;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

struct Frame {
    std::vector<int32_t> id, status;
    std::vector<float> xy, xyz;
    std::vector<uint8_t> has_lm;
    float pose[7], mag;
    TbInsertIn in(bool flags = false) const {
        return TbInsertIn{(int)id.size(), id.data(), xy.data(), xyz.data(), status.data(), flags ? has_lm.data() : nullptr, pose, mag};
    }
};

// frame t: n slots, ids first .. first + n - 1 in a rotated order, statuses cycling 0 .. 5
static Frame make_frame(int t, int n, int first) {
    Frame f;
    for (int i = 0; i < n; ++i) {
        const int k = (i * 11 + t) % n;                            // (a permutation: no n used here is a multiple of 11)
        f.id.push_back(first + k);
        f.status.push_back((k + t) % 6);
        f.xy.push_back(10.f * t + k); f.xy.push_back(-1.f * k);
        f.xyz.push_back(0.5f * k); f.xyz.push_back(1.f * t); f.xyz.push_back(3.f);
        f.has_lm.push_back((uint8_t)(k % 3 != 0));
    }
    for (int k = 0; k < 7; ++k) f.pose[k] = 0.1f * k + t;
    f.mag = 0.001f * t;
    return f;
}

static bool insert(TbufHost& h, const Frame& f, std::vector<uint32_t>* block = nullptr, char* msg_out = nullptr, bool flags = false) {
    std::vector<uint64_t> seen;
    char msg[256] = "";
    TbPlan p;
    const TbInsertIn in = f.in(flags);
    const int rc = tb_plan_insert(h, in, &p, seen, msg, sizeof msg);
    if (msg_out) memcpy(msg_out, msg, sizeof msg);
    if (rc != 0) return false;
    std::vector<uint32_t> b((size_t)TBUF_HEAD + (size_t)TBUF_ENTRY * (size_t)p.m);   // exactly the upload's length
    tb_pack(in, p, b.data());
    if (block) *block = b;
    tb_commit(h, in, p);
    return true;
}

int main() {
    char msg[256];
    // ---- create
    CHECK(tb_check_create(20, msg, sizeof msg) == 0 && tb_check_create(1, msg, sizeof msg) == 0);
    CHECK(tb_check_create(0, msg, sizeof msg) != 0 && strstr(msg, "outside [1, 20]"));
    CHECK(tb_check_create(21, msg, sizeof msg) != 0);

    // ---- the pop rule, the reference counts and the span over 45 inserts, against a list of id sets
    {
        TbufHost h;
        tb_reset(h, 20);
        std::vector<std::set<int32_t>> ref;
        std::vector<int> ref_cand;
        for (int t = 0; t < 45; ++t) {
            const Frame f = make_frame(t, 70, 40 * t);             // a sliding window: ids enter and leave
            std::vector<uint32_t> block;
            CHECK(insert(h, f, &block, nullptr, true));
            std::set<int32_t> kept;
            int nc = 0;
            for (size_t i = 0; i < f.id.size(); ++i)
                if (f.status[i] == 0 || f.status[i] == 1) { kept.insert(f.id[i]); nc += f.status[i] == 1; }
            if ((int)ref.size() > 20) { ref.erase(ref.begin()); ref_cand.erase(ref_cand.begin()); }
            ref.push_back(kept); ref_cand.push_back(nc);
            const int want = t < 21 ? t + 1 : 21;                  // 1 .. 21, then 21 -> (pop) 20 -> (insert) 21 inside every call
            CHECK((int)h.snaps.size() == want && ref.size() == h.snaps.size());
            std::set<int32_t> all;
            for (const auto& s : ref) all.insert(s.begin(), s.end());
            CHECK(h.n_ids() == (int)all.size() && h.n_candidates() == nc);
            int32_t lo = 0, hi = -1;
            CHECK(tb_span(h, &lo, &hi) && lo == *all.begin() && hi == *all.rbegin());
            for (int32_t id : all) {
                int cnt = 0;
                for (const auto& s : ref) cnt += (int)s.count(id);
                CHECK(h.ref.at(id) == cnt);
            }
            // the slots in use are distinct and inside the ring
            std::set<int> slots;
            for (const TbSnap& s : h.snaps) { slots.insert(s.slot); CHECK(s.slot >= 0 && s.slot < h.n_slots()); }
            CHECK(slots.size() == h.snaps.size() && slots.size() + h.free_slots.size() == (size_t)h.n_slots());
            // the block: head, then the kept entries in the frame's order
            const size_t m = kept.size();
            CHECK(block.size() == TBUF_HEAD + TBUF_ENTRY * m && h.snaps.back().ids.size() == m);
            float head[8];
            memcpy(head, block.data(), 32);
            CHECK(head[0] == f.pose[0] && head[6] == f.pose[6] && head[7] == f.mag);
            size_t j = 0;
            for (size_t i = 0; i < f.id.size(); ++i) {
                if (f.status[i] > 1) continue;
                CHECK(block[TBUF_HEAD + j] == (uint32_t)f.id[i] && h.snaps.back().ids[j] == f.id[i]);
                CHECK(block[TBUF_HEAD + m + j] == ((uint32_t)f.status[i] | (f.has_lm[i] ? TBUF_HAS_LM : 0u)));
                CHECK(memcmp(&block[TBUF_HEAD + 2 * m + 2 * j], &f.xy[2 * i], 8) == 0 && memcmp(&block[TBUF_HEAD + 4 * m + 3 * j], &f.xyz[3 * i], 12) == 0);
                ++j;
            }
            CHECK(j == m);
        }
        // has_lm == null: every kept entry carries the flag
        std::vector<uint32_t> block;
        const Frame f = make_frame(45, 9, 5000);
        CHECK(insert(h, f, &block));
        const size_t m = (block.size() - TBUF_HEAD) / TBUF_ENTRY;
        for (size_t j = 0; j < m; ++j) CHECK(block[TBUF_HEAD + m + j] & TBUF_HAS_LM);
        // clear: nothing held, every slot free, the slots' size kept
        const int cap = h.cap;
        tb_reset(h, h.max_size);
        int32_t lo, hi;
        CHECK(h.snaps.empty() && h.n_ids() == 0 && h.n_candidates() == 0 && !tb_span(h, &lo, &hi) && (int)h.free_slots.size() == 21 && h.cap == cap);
    }

    // ---- a small ring: max = 2 goes 1, 2, 3 and stays there (3 -> 2 -> 3 inside a call)
    {
        TbufHost h;
        tb_reset(h, 2);
        const int want[] = {1, 2, 3, 3, 3, 3};
        for (int t = 0; t < 6; ++t) { CHECK(insert(h, make_frame(t, 12, 3 * t))); CHECK((int)h.snaps.size() == want[t]); }
    }

    // ---- every refusal leaves the buffer as it was
    {
        TbufHost h;
        tb_reset(h, 20);
        CHECK(insert(h, make_frame(0, 30, 100)));
        const int n_ids = h.n_ids(), n_cand = h.n_candidates();
        auto unchanged = [&]() { return h.snaps.size() == 1 && h.n_ids() == n_ids && h.n_candidates() == n_cand && h.free_slots.size() == 20; };
        Frame f = make_frame(1, 30, 100);
        // a duplicate among the kept entries
        f.status[3] = 0; f.status[9] = 1; f.id[9] = f.id[3];
        CHECK(!insert(h, f, nullptr, msg) && strstr(msg, "duplicate keypoint id") && unchanged());
        // ... among dropped entries it is not looked at
        f.status[9] = 4;
        CHECK(insert(h, f) && h.snaps.size() == 2);
        tb_reset(h, 20);
        CHECK(insert(h, make_frame(0, 30, 100)));
        // a negative id: refused when kept, ignored when dropped
        f = make_frame(1, 30, 100);
        f.status[5] = 1; f.id[5] = -7;
        CHECK(!insert(h, f, nullptr, msg) && strstr(msg, "negative keypoint id -7") && unchanged());
        f.status[5] = 2;
        CHECK(insert(h, f));
        tb_reset(h, 20);
        CHECK(insert(h, make_frame(0, 30, 100)));
        // the span: inside one frame, and against the held snapshots
        f = make_frame(1, 30, 100);
        f.status[0] = 0; f.id[0] = 100 + (int32_t)TBUF_MAX_SPAN + 40;
        CHECK(!insert(h, f, nullptr, msg) && strstr(msg, "more than the limit of 4194304 ids") && unchanged());
        f = make_frame(1, 4, 100 + (int32_t)TBUF_MAX_SPAN);
        f.status.assign(4, 0);
        CHECK(!insert(h, f, nullptr, msg) && strstr(msg, "limit") && unchanged());
        f = make_frame(1, 4, 100 + (int32_t)TBUF_MAX_SPAN - 4);   // the last id that fits: span == limit
        f.status.assign(4, 0);
        CHECK(insert(h, f));
        int32_t lo = 0, hi = -1;
        CHECK(tb_span(h, &lo, &hi) && (int64_t)hi - lo + 1 == TBUF_MAX_SPAN);
        // a far frame is accepted once the near ones have left: max = 1 pops the near one first
        TbufHost g;
        tb_reset(g, 1);
        CHECK(insert(g, make_frame(0, 6, 0)) && insert(g, make_frame(1, 6, 3)));
        f = make_frame(2, 6, 2 * (int32_t)TBUF_MAX_SPAN);
        f.status.assign(6, 1);
        CHECK(!insert(g, f, nullptr, msg) && g.snaps.size() == 2);   // pops frame 0, frame 1 stays: too wide
        // the largest id there is
        f = make_frame(1, 2, 2147483646);
        f.status.assign(2, 0);
        TbufHost top;
        tb_reset(top, 20);
        CHECK(insert(top, f) && tb_span(top, &lo, &hi) && hi == 2147483647);
        // null arrays
        tb_reset(h, 20);
        CHECK(insert(h, make_frame(0, 30, 100)));
        f = make_frame(1, 30, 100);
        std::vector<uint64_t> seen;
        TbPlan p;
        TbInsertIn in = f.in();
        in.kp_xy = nullptr;
        CHECK(tb_plan_insert(h, in, &p, seen, msg, sizeof msg) != 0 && strstr(msg, "null array") && unchanged());
        in = f.in(); in.status = nullptr;
        CHECK(tb_plan_insert(h, in, &p, seen, msg, sizeof msg) != 0);
        in = f.in(); in.pose_qt = nullptr;
        CHECK(tb_plan_insert(h, in, &p, seen, msg, sizeof msg) != 0);
        in = f.in(); in.n = -1;
        CHECK(tb_plan_insert(h, in, &p, seen, msg, sizeof msg) != 0);
        // an empty frame is a snapshot all the same (no array is read)
        in = TbInsertIn{0, nullptr, nullptr, nullptr, nullptr, nullptr, f.pose, 0.f};
        CHECK(tb_plan_insert(h, in, &p, seen, msg, sizeof msg) == 0 && p.m == 0);
        uint32_t head[TBUF_HEAD];
        tb_pack(in, p, head);
        tb_commit(h, in, p);
        CHECK(h.snaps.size() == 2 && h.n_candidates() == 0 && h.n_ids() == n_ids && h.snaps.back().id_hi < h.snaps.back().id_lo);
        CHECK(tb_span(h, &lo, &hi) && lo >= 100 && hi < 130);
    }

    // ---- the doubling of the slots: never shrinks, the smallest power-of-two multiple that holds the snapshot
    {
        TbufHost h;
        tb_reset(h, 20);
        CHECK(h.cap == TBUF_MIN_CAP);
        Frame f = make_frame(0, 257, 0);
        f.status.assign(257, 0);
        CHECK(insert(h, f) && h.cap == 2 * TBUF_MIN_CAP);
        f = make_frame(1, 2049, 0);
        f.status.assign(2049, 1);
        CHECK(insert(h, f) && h.cap == 4096 && h.n_candidates() == 2049);
        CHECK(insert(h, make_frame(2, 5, 0)) && h.cap == 4096);
        CHECK(tb_slot_words(4096) == 8 + 7 * 4096);
    }

    // ---- the layout of the dense tables: aligned, disjoint, in order; the cleared part ends where the status begins
    for (size_t F : {1, 21}) for (size_t n : {1, 63, 4446}) for (size_t span : {n, 3 * n + 5}) {
        const TbLayout L(F, n, span);
        const size_t at[] = {L.row, L.has_kp, L.has_lm, L.kp_xy, L.lm_xyz, L.status, L.row_id, L.poses, L.mag, L.bytes};
        const size_t need[] = {4 * span, F * n, F * n, 8 * F * n, 12 * F * n, 4 * n, 4 * n, 28 * F, 4 * F};
        for (int k = 0; k < 9; ++k) CHECK(at[k] % 256 == 0 && at[k] + need[k] <= at[k + 1]);
        CHECK(L.zero_end == L.status && L.row == 0);
    }

    // ---- the checks of the mapping call
    {
        TbufHost h;
        tb_reset(h, 20);
        int cam = 0, d = 0;
        const void* outs[10] = {&d, &d, &d, &d, &d, &d, &d, &d, &d, &d};
        bool state = false;
        CHECK(tb_check_map(h, &cam, 0, 0.001f, 0.004f, -1, outs, &state, msg, sizeof msg) != 0 && state && strstr(msg, "holds no snapshot"));
        CHECK(insert(h, make_frame(0, 30, 100)) && insert(h, make_frame(1, 30, 100)));
        CHECK(tb_check_map(h, &cam, 0, 0.001f, 0.004f, -1, outs, &state, msg, sizeof msg) == 0);
        CHECK(tb_check_map(h, &cam, 1, 0.001f, 0.004f, 1, outs, &state, msg, sizeof msg) == 0);
        CHECK(tb_check_map(h, &cam, 0, 0.001f, 0.004f, 2, outs, &state, msg, sizeof msg) != 0 && !state && strstr(msg, "index_snapshot 2 outside [-1, 2)"));
        CHECK(tb_check_map(h, &cam, 0, 0.001f, 0.004f, -2, outs, &state, msg, sizeof msg) != 0 && !state);
        CHECK(tb_check_map(h, &cam, 7, 0.001f, 0.004f, -1, outs, &state, msg, sizeof msg) != 0 && strstr(msg, "camera model"));
        CHECK(tb_check_map(h, nullptr, 0, 0.001f, 0.004f, -1, outs, &state, msg, sizeof msg) != 0);
        CHECK(tb_check_map(h, &cam, 0, NAN, 0.004f, -1, outs, &state, msg, sizeof msg) != 0 && strstr(msg, "finite"));
        CHECK(tb_check_map(h, &cam, 0, 0.001f, INFINITY, -1, outs, &state, msg, sizeof msg) != 0);
        outs[8] = nullptr;
        CHECK(tb_check_map(h, &cam, 0, 0.001f, 0.004f, -1, outs, &state, msg, sizeof msg) != 0);
    }
    printf(fails ? "tbuf_check: %d FAILED\n" : "tbuf_check: OK\n", fails);
    return fails ? 1 : 0;
}
