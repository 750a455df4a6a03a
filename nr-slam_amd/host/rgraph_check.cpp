// Stand-alone check of the host half of the device-resident RegularizationGraph (csrc/nrs_rgraph_host.hpp) under AddressSanitizer +
// UBSan: `make rgraph_check` (builds and runs it).  No HIP, no library.  Every expectation is restated here -- the pointer sequences,
// loops and conditions as they stood inline in nrs_rgraph.hip before the header took them over -- and not taken from the header's own
// functions.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../csrc/nrs_rgraph_host.hpp"

using namespace nrs;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

// the limit of candidates per row as the two sites computed it
static size_t ref_cand_max(int lds_max) {
    size_t cand_max = 512;
    while (sizeof(unsigned long long) * (cand_max << 1) + 4096 + 512 <= (size_t)lds_max) cand_max <<= 1;
    return cand_max;
}
static bool pow2(size_t v) { return v && !(v & (v - 1)); }

static void check_layout(int n_ids, int cap_per_point) {
    const RgListLayout L(n_ids, cap_per_point);
    const size_t no = (size_t)n_ids * cap_per_point;
    // a block of exactly the length the library allocates: every pointer below stays inside it
    std::vector<int> block(4 * no + (size_t)n_ids + 1);
    CHECK(L.bytes() == sizeof(int) * block.size() && L.list_bytes() == sizeof(int) * (block.size() - 1));
    // (1) the device pointers of rg_get_edges_impl
    int* d_cnt = block.data();
    int* d_col = d_cnt + n_ids;
    int* d_st = d_col + no;
    float* d_w = reinterpret_cast<float*>(d_st + no);
    float* d_d0 = d_w + no;
    int* d_ovf = reinterpret_cast<int*>(d_d0 + no);
    CHECK(d_cnt + L.col == d_col && d_cnt + L.status == d_st && (void*)(d_cnt + L.w) == (void*)d_w && (void*)(d_cnt + L.d0) == (void*)d_d0);
    CHECK(d_cnt + L.overflow == d_ovf && d_ovf == &block.back());
    // (2) its pinned host pointers, (3) the overflow word's index
    const int* h = block.data();
    const RgDeviceLists v = L.view(h);
    CHECK(v.n_rows == n_ids && v.stride == cap_per_point);
    CHECK(v.count == h && v.col == h + n_ids && v.status == h + n_ids + no);
    CHECK((const void*)v.w == (const void*)(h + n_ids + 2 * no) && (const void*)v.d0 == (const void*)(h + n_ids + 3 * no));
    CHECK(L.overflow == 4 * no + (size_t)n_ids);
    // (4) rg_walk's and (5) rg_get_edges_device's sequences from the start of the device block
    const int* w_cnt = block.data();
    const int* w_col = w_cnt + n_ids;
    const int* w_st = w_col + no;
    const float* w_w = reinterpret_cast<const float*>(w_st + no);
    const float* w_d0 = w_w + no;
    CHECK(v.count == w_cnt && v.col == w_col && v.status == w_st && v.w == w_w && v.d0 == w_d0);
    // the last entry of the last array is the word in front of the overflow word
    block[L.overflow] = 7;
    CHECK((const void*)(v.d0 + no) == (const void*)&block[L.overflow]);
}

static void check_pass(int cap, int cap_per_point, int lds_max) {
    const size_t cand_max = ref_cand_max(lds_max);
    for (int pass = 0; pass < 2; ++pass) {
        const int cand_cap = pass == 0 ? std::min(cap, cap_per_point + 1024) : (int)std::min<size_t>({(size_t)cap, (size_t)12000, cand_max});
        size_t pad = 512;
        while (pad < (size_t)cand_cap) pad <<= 1;
        const RgPass p = rg_pass_plan(pass, cap, cap_per_point, rg_cand_limit((size_t)lds_max));
        CHECK(p.cand_cap == cand_cap && p.pad == pad && p.lds_bytes == sizeof(unsigned long long) * pad);
        CHECK(pow2(p.pad) && p.pad >= 512 && p.pad >= (size_t)p.cand_cap);
        CHECK(p.lds_bytes + 4096 + 512 <= (size_t)lds_max);        // a call that passed rg_check_fits_lds launches
    }
}

int main() {
    char msg[256];
    // ---- the layout against the five written-out pointer sequences
    const int shapes[][2] = {{1, 1}, {1, 16}, {7, 1}, {3, 5}, {80, 16}, {80, 256}, {321, 64}, {4446, 11}};
    for (const auto& s : shapes) check_layout(s[0], s[1]);

    // ---- what fits a row's sort buffer in LDS
    CHECK(rg_cand_limit(65536) == ref_cand_max(65536) && rg_cand_limit(65536) == 4096);
    CHECK(rg_cand_limit(163840) == ref_cand_max(163840) && rg_cand_limit(163840) == 16384);
    CHECK(rg_cand_limit(0) == 512);
    for (int lds : {65536, 163840}) {
        const int lim = (int)ref_cand_max(lds) - 1024;             // the longest prefix: rg_max_cap_per_point of a large graph
        for (int cpp : {16, 256, lim})
            for (int cap : {321, 577, 5000, 20000}) check_pass(cap, std::min(cpp, cap), lds);
    }
    CHECK(rg_pass_plan(1, 20000, 16, 8192).cand_cap == 8192 && rg_pass_plan(1, 20000, 16, 16384).cand_cap == 12000);   // the 12000 of the second pass
    CHECK(rg_pass_plan(1, 20000, 16, 16384).pad == 16384 && rg_pass_plan(0, 100, 16, 4096).pad == 512);
    CHECK(rg_pass_plan(0, 200000, 2147483647, 8192).cand_cap == 200000);   // (no overflow in prefix + slack)
    // rg_max_cap_per_point
    CHECK(rg_cap_limit(5000, 8192, false, 0) == 5000 && rg_cap_limit(20000, 8192, false, 0) == 8192 - 1024);
    CHECK(rg_cap_limit(20000, 8192, true, 64) == 64 && rg_cap_limit(20000, 8192, true, 0) == 1 && rg_cap_limit(300, 8192, true, 100000) == 300);
    CHECK(rg_check_fits_lds(20000, 15360, 16384, 163840, msg, sizeof msg) == 0);
    CHECK(rg_check_fits_lds(20000, 15361, 16384, 163840, msg, sizeof msg) != 0 &&
          !strcmp(msg, "GetEdges: cap_per_point 15361 needs more than the 16384 candidates per row that fit this device's 163840 bytes of LDS"));
    CHECK(rg_check_fits_lds(5000, 15361, 16384, 163840, msg, sizeof msg) == 0);   // (a row has no more than capacity candidates)

    // ---- the form of an update: 4 n_ids >= cap and no duplicate
    {
        std::vector<int> slot;
        std::vector<int32_t> ids;
        for (int i = 0; i < 81; ++i) ids.push_back((i * 37 + 5) % 321);   // a permuted list of distinct ids (37 and 321 are coprime)
        CHECK(!rg_update_one_pass(321, 80, ids.data(), slot));     // 320 < 321
        CHECK(rg_update_one_pass(321, 81, ids.data(), slot));      // 324 >= 321
        CHECK(rg_update_one_pass(320, 80, ids.data(), slot));      // 320 >= 320
        CHECK(slot.size() == 320);
        std::vector<int> want(320, -1);
        for (int a = 0; a < 80; ++a) want[ids[a]] = a;
        CHECK(slot == want);
        for (int dup_at : {0, 40, 79}) {                           // a duplicate of the first, a middle and the last entry
            std::vector<int32_t> d(ids.begin(), ids.begin() + 80);
            d.push_back(d[dup_at]);
            CHECK(!rg_update_one_pass(321, 81, d.data(), slot));
        }
        std::vector<int32_t> d(ids.begin(), ids.begin() + 81);
        d[1] = d[0];                                               // ... and a duplicate that comes first
        CHECK(!rg_update_one_pass(321, 81, d.data(), slot));
        d[1] = ids[1]; d[41] = d[40];
        CHECK(!rg_update_one_pass(321, 81, d.data(), slot));
        const int32_t one = 0;
        CHECK(rg_update_one_pass(2, 1, &one, slot) && slot[0] == 0 && slot[1] == -1);
    }

    // ---- the mirror: (int64_t)n_ids * 8 >= cap && cap >= 512 && no switch
    CHECK(!rg_use_mirror(511, 511, false) && rg_use_mirror(512, 512, false) && rg_use_mirror(64, 512, false) && !rg_use_mirror(63, 512, false));
    CHECK(rg_use_mirror(72, 575, false) && rg_use_mirror(72, 576, false) && !rg_use_mirror(72, 577, false));   // 8 n = cap + 1, cap, cap - 1
    CHECK(rg_use_mirror(73, 577, false) && rg_use_mirror(80, 577, false) && !rg_use_mirror(80, 577, true));
    CHECK(rg_use_mirror(2000000000, 200000, false));               // (no overflow in 8 n)

    // ---- the walk's scratch plan: the order and sizes of the parent's offsets
    const size_t walks[][2] = {{1, 1}, {300, 299}, {4446, 4000}, {5000, 5000}};
    for (const auto& s : walks) {
        const size_t n_map = s[0], n = s[1];
        const RgWalkPlan P(n_map, n);
        auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t o_code = 0, o_node = o_code + al(4 * n_map), o_acc = o_node + al(n), o_nacc = o_acc + al(4 * 11 * n), o_w = o_nacc + al(4 * n),
                     o_d0 = o_w + al(4 * 11 * n), o_end = o_d0 + al(4 * 11 * n), o_lost = o_end + al(n), o_chg = o_lost + al(n_map), total = o_chg + al(4 * (96 + 1));
        CHECK(P.code == o_code && P.node == o_node && P.acc == o_acc && P.n_acc == o_nacc && P.w == o_w && P.d0 == o_d0 && P.ended == o_end);
        CHECK(P.lost == o_lost && P.changed == o_chg && P.total == total);
        // 256-byte aligned, ordered, each part as long as what is kept there: disjoint
        const size_t off[] = {P.code, P.node, P.acc, P.n_acc, P.w, P.d0, P.ended, P.lost, P.changed, P.total};
        const size_t need[] = {4 * n_map, n, 44 * n, 4 * n, 44 * n, 44 * n, n, n_map, 4 * 97};
        for (int k = 0; k < 9; ++k) CHECK(off[k] % 256 == 0 && off[k] + need[k] <= off[k + 1]);
        // the one fill clears exactly the lost flags through the last change counter
        CHECK(P.zero_bytes == o_chg - o_lost + 4 * (96 + 1) && P.lost + P.zero_bytes == P.changed + 4 * 97 && P.lost + P.zero_bytes <= P.total);
    }
    CHECK(RG_WALK_MAX == 11 && RG_WALK_PASSES == 96);

    // ---- every refusal with its text
    {
        const int32_t ids[4] = {0, 3, 9, 2}, neg[2] = {1, -1};
        CHECK(rg_check_ids(10, 4, ids, "f", msg, sizeof msg) == 0 && rg_check_ids(10, 0, nullptr, "f", msg, sizeof msg) == 0);
        CHECK(rg_check_ids(10, -1, ids, "nrs_rgraph_update", msg, sizeof msg) != 0 && !strcmp(msg, "nrs_rgraph_update: null / negative id list"));
        CHECK(rg_check_ids(10, 2, nullptr, "nrs_rgraph_rows", msg, sizeof msg) != 0 && !strcmp(msg, "nrs_rgraph_rows: null / negative id list"));
        CHECK(rg_check_ids(9, 4, ids, "nrs_rgraph_add_edges", msg, sizeof msg) != 0 && !strcmp(msg, "nrs_rgraph_add_edges: point index 9 outside [0, 9)"));
        CHECK(rg_check_ids(9, 2, neg, "GetEdges", msg, sizeof msg) != 0 && !strcmp(msg, "GetEdges: point index -1 outside [0, 9)"));

        CHECK(rg_check_create(2, 2.2f, 1.1f, msg, sizeof msg) == 0 && rg_check_create(200000, 1e-3f, 1e-3f, msg, sizeof msg) == 0);
        const float nan = std::nanf("");
        const struct { int cap; float sigma, th; } bad[] = {{1, 1, 1}, {0, 1, 1}, {-5, 1, 1}, {200001, 1, 1}, {10, 0, 1}, {10, -1, 1}, {10, nan, 1}, {10, 1, 0}, {10, 1, nan}};
        for (const auto& b : bad) { msg[0] = 0; CHECK(rg_check_create(b.cap, b.sigma, b.th, msg, sizeof msg) != 0 && !strcmp(msg, "nrs_rgraph_create: bad argument")); }

        CHECK(rg_check_resize(130, 130, msg, sizeof msg) == 0 && rg_check_resize(130, 577, msg, sizeof msg) == 0 && rg_check_resize(130, 200000, msg, sizeof msg) == 0);
        CHECK(rg_check_resize(130, 12, msg, sizeof msg) != 0 && !strcmp(msg, "nrs_rgraph_resize: capacity 12 is below the graph's 130"));
        CHECK(rg_check_resize(130, 200001, msg, sizeof msg) != 0 &&
              !strcmp(msg, "nrs_rgraph_resize: capacity 200001 is past the limit of 200000 points (nrs_rgraph_create: bad argument)"));

        CHECK(rg_check_get_edges(10, 4, ids, false, 8, msg, sizeof msg) == 0 && rg_check_get_edges(10, 10, nullptr, true, 1, msg, sizeof msg) == 0);
        CHECK(rg_check_get_edges(10, 0, nullptr, true, 8, msg, sizeof msg) != 0 && !strcmp(msg, "GetEdges: 0 device-side ids for 10 points"));
        CHECK(rg_check_get_edges(10, 11, nullptr, true, 8, msg, sizeof msg) != 0 && !strcmp(msg, "GetEdges: 11 device-side ids for 10 points"));
        CHECK(rg_check_get_edges(9, 4, ids, false, 8, msg, sizeof msg) != 0 && !strcmp(msg, "GetEdges: point index 9 outside [0, 9)"));
        CHECK(rg_check_get_edges(10, 4, ids, false, 0, msg, sizeof msg) != 0 && !strcmp(msg, "GetEdges: cap_per_point must be positive"));
        CHECK(rg_check_get_edges(9, 4, ids, false, 0, msg, sizeof msg) != 0 && !strcmp(msg, "GetEdges: point index 9 outside [0, 9)"));   // (the ids first)

        CHECK(rg_check_get_edges_abi(4, 8, true, msg, sizeof msg) == 0 && rg_check_get_edges_abi(0, 8, false, msg, sizeof msg) == 0);
        CHECK(rg_check_get_edges_abi(4, 8, false, msg, sizeof msg) != 0 && !strcmp(msg, "nrs_rgraph_get_edges: bad argument"));
        msg[0] = 0;
        CHECK(rg_check_get_edges_abi(0, 0, true, msg, sizeof msg) != 0 && !strcmp(msg, "nrs_rgraph_get_edges: bad argument"));
    }

    // ---- min_weight and the far-distance bound: the reference's float expression (regularization_graph.cc:29), the same casts
    for (float sigma : {2.2f, 1.0f}) {
        const float d = (float)((double)sigma * 1.5);
        const float arg = -(d * d) / (2.0f * sigma * sigma);
        const float want = (float)exp((double)arg);
        const float got = rg_min_weight(sigma);
        CHECK(!memcmp(&got, &want, 4));
        const float far_want = (float)((double)sigma * 1.5 * (1.0 + 1e-4)), far = rg_far_distance(sigma);
        CHECK(!memcmp(&far, &far_want, 4) && far > d);
        CHECK(rg_weight(far, sigma) < got && rg_weight(0.f, sigma) == 1.f);
    }
    CHECK(std::fabs(rg_min_weight(1.0f) - 0.32465247f) < 1e-6f);   // exp(-1.125): sigma cancels (guards against a wrong formula, not a last bit)

    if (fails) { printf("rgraph_check: %d check(s) FAILED\n", fails); return 1; }
    printf("rgraph_check: all checks passed\n");
    return 0;
}
