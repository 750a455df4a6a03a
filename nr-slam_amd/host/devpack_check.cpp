// Stand-alone check of the host pieces of the device-side problem construction (csrc/nrs_devpack_host.hpp) for a sanitizer build:
// `make devpack_check && ./devpack_check`.  No HIP, no library.
//   scratch plans   each of the five plans, over a table of sizes (zeros, ones, C2-like, a rank with an empty share, the resident-graph form
//                   with far more map points than landmarks, counts near 2^31), against a LITERAL restatement of the bump-allocator
//                   sequences and byte sums the plans replaced (`Old` below: one get<> per array, in the order the packer had them):
//                   the same offsets, the same bytes asked of `ensure`; regions in table order, 256-aligned, not overlapping
//   host decisions  the fall-back reasons of the two host scans, the tile range of a pack range, row_bits, ec_nblk, halo_ptr and the
//                   empty-tile reach fix-up against brute-force restatements on hand-made inputs
// Seeded into a scratch copy of the header, one at a time, each of these makes the program fail:
//    1  pack scratch 1: `cd` not placed                             7  the 256 bytes of slack behind an array dropped
//    2  pack scratch 2: D_o at nnz_d ints, not 3 nnz_d              8  resident-graph form: `mark` one int short
//    3  dp_place: bytes as an int product                           9  embedded lists: kfb at 2 n_kf + 1 ints
//    4  dp_tile_range: tb1 from pack_hi - 1                        10  dp_row_bits from n_rows, not n_rows - 1
//    5  the reach fix-up over every tile, not the rank's           11  dp_precheck: -1 accepted as a damper vertex
//    6  pack scratch 2 with the margin of scratch 1                12  dp_ec_nblk without the cap of 2048
#include <cstdio>
#include <cstdlib>
#include "../csrc/nrs_devpack_host.hpp"

using namespace nrs;
typedef std::vector<int> VI;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "devpack_check: %s:%d: %s\n", __FILE__, __LINE__, #x); std::abort(); } } while (0)

// the bump allocator the packer had (DpScratch::get), recording what it hands out: region, offset, bytes
struct Old {
    size_t off = 0;
    std::vector<int> id; std::vector<size_t> at, bytes;
    template <class Tp> void get(int r, size_t n) {
        id.push_back(r); at.push_back(off); bytes.push_back(n * sizeof(Tp));
        off += ((n * sizeof(Tp) + 255) / 256) * 256 + 256;
    }
};
static size_t al(size_t b) { return ((b + 255) / 256) * 256 + 256; }

// plan against restatement; `asked`: what the packer asked `ensure` for
template <int N> static void check_plan(const DpPlan<N>& P, const Old& o, size_t asked, size_t margin) {
    CHECK(P.need == asked && P.total == asked - margin && P.total == o.off);
    std::vector<bool> placed(N, false);
    for (size_t i = 0; i < o.id.size(); ++i) {
        const int r = o.id[i];
        CHECK(r >= 0 && r < N && !placed[r] && (i == 0 || r > o.id[i - 1]));            // table order = the enum's
        placed[r] = true;
        CHECK(P.off[r] == o.at[i] && P.bytes[r] == o.bytes[i] && P.off[r] % 256 == 0);
        const size_t end = i + 1 < o.id.size() ? P.off[o.id[i + 1]] : P.total;
        CHECK(P.off[r] + P.bytes[r] + 256 <= end);                  // (its bytes and the slack lie in front of the next region)
        char* const base = reinterpret_cast<char*>((uintptr_t)0x1000);
        const char* at = P.elem[r] == 1 ? P.template at<char>(base, r) : P.elem[r] == 4 ? reinterpret_cast<char*>(P.template at<int>(base, r)) : reinterpret_cast<char*>(P.template at<double>(base, r));
        CHECK(at == base + o.at[i] && o.bytes[i] % P.elem[r] == 0 && (P.elem[r] == 1 || P.elem[r] == 4 || P.elem[r] == 8));
    }
    for (int r = 0; r < N; ++r) if (!placed[r]) CHECK(P.bytes[r] == 0);                  // (not present: nothing to point at)
}

// ---- pack scratch 1: engine_create_device's `layout`, sh = a rank of a sharded window
static void check_pack1(int M, int K, int n_sp, int n_dm, int n_rows, int T, int tile_rows, size_t tmp_bytes, bool sh) {
    const int n_slices = n_rows / (64 / T), n_tiles = n_rows / tile_rows;
    const int64_t ni_s = 2 * (int64_t)n_sp, ni_d = 4 * (int64_t)n_dm;
    Old W;
    W.get<double>(P1_r_x, 3 * (size_t)M); W.get<int>(P1_r_kf, M); W.get<float>(P1_r_uv, 2 * (size_t)M);
    W.get<int>(P1_r_sp, 2 * (size_t)n_sp); W.get<float>(P1_r_d0, n_sp); W.get<int>(P1_r_dm, 4 * (size_t)n_dm); W.get<float>(P1_r_w, n_dm);
    W.get<uint64_t>(P1_code_a, M); W.get<uint64_t>(P1_code_b, M);
    W.get<int>(P1_val_a, M); W.get<int>(P1_val_b, M); W.get<int>(P1_cs, M); W.get<int>(P1_cd, M);
    W.get<int>(P1_pose_ptr, K + 1); W.get<int>(P1_pgp, K + 1); W.get<int>(P1_tile_off, n_tiles + 1);
    W.get<int>(P1_vrow, M); W.get<int>(P1_row_v, n_rows);
    W.get<uint32_t>(P1_tk_a, n_rows); W.get<uint32_t>(P1_tk_b, n_rows); W.get<int>(P1_tv_a, n_rows); W.get<int>(P1_tv_b, n_rows);
    W.get<int>(P1_cnt_s, (size_t)n_rows + 1); W.get<int>(P1_cnt_d, (size_t)n_rows + 1); W.get<int>(P1_rs_s, (size_t)n_rows + 1); W.get<int>(P1_rs_d, (size_t)n_rows + 1);
    if (!sh) { W.get<uint64_t>(P1_key_s, ni_s); W.get<uint64_t>(P1_key_s2, ni_s); W.get<uint64_t>(P1_key_d, ni_d); W.get<uint64_t>(P1_key_d2, ni_d); }
    W.get<int>(P1_ws, (size_t)n_slices + 1); W.get<int>(P1_wd, (size_t)n_slices + 1); W.get<int>(P1_ss, (size_t)n_slices + 1); W.get<int>(P1_sd, (size_t)n_slices + 1);
    W.get<char>(P1_tmp, tmp_bytes);
    W.get<double>(P1_mm, 8);
    W.get<int>(P1_hs, n_tiles); W.get<int>(P1_hns, n_tiles); W.get<int>(P1_hmin, n_tiles); W.get<int>(P1_hmax, n_tiles); W.get<int>(P1_flag, 16);
    const auto P = dp_pack1_plan(DpPack1In{(size_t)M, (size_t)K, (size_t)n_sp, (size_t)n_dm, (size_t)n_rows, (size_t)n_slices, (size_t)n_tiles, tmp_bytes, !sh});
    check_plan(P, W, W.off + 4096, 4096);
}

// ---- pack scratch 2: the byte sum `need2` and the get<> sequence behind it
static void check_pack2(size_t nnz_s, size_t nnz_d, int ec_nsp, int ec_ndm, int64_t own_s, int64_t own_d, size_t tmp2_bytes, bool sh) {
    const size_t need2 = 2 * al(4 * nnz_s) + al(nnz_s) + al(12 * nnz_d) + al(4 * nnz_d) + al(nnz_d) + 2 * al(8 * (size_t)ec_nsp) + 2 * al(8 * (size_t)ec_ndm) +
                         (sh ? 2 * al(8 * (size_t)own_s) + 2 * al(8 * (size_t)own_d) + al(tmp2_bytes) : 0) + (1 << 16);
    Old W2;
    W2.get<int>(P2_S_other, nnz_s);
    W2.get<uint8_t>(P2_S_side, nnz_s);
    W2.get<int>(P2_D_o, 3 * nnz_d);
    W2.get<int8_t>(P2_D_role, nnz_d);
    W2.get<uint64_t>(P2_ek_s, ec_nsp); W2.get<uint64_t>(P2_ek_s2, ec_nsp);
    W2.get<uint64_t>(P2_ek_d, ec_ndm); W2.get<uint64_t>(P2_ek_d2, ec_ndm);
    W2.get<float>(P2_t_d0, nnz_s);
    W2.get<float>(P2_t_w, nnz_d);
    if (sh) {
        W2.get<uint64_t>(P2_key_s, own_s); W2.get<uint64_t>(P2_key_s2, own_s); W2.get<uint64_t>(P2_key_d, own_d); W2.get<uint64_t>(P2_key_d2, own_d);
        W2.get<char>(P2_tmp, tmp2_bytes);
    }
    const auto P = dp_pack2_plan(DpPack2In{nnz_s, nnz_d, (size_t)ec_nsp, (size_t)ec_ndm, (size_t)own_s, (size_t)own_d, tmp2_bytes, sh});
    check_plan(P, W2, need2, (size_t)1 << 16);
}

// ---- window-edge scratch: win_edges_device's `layout`; rg: the resident graph serves the lists (nnz = 0, n_points = its capacity)
static void check_winedge(int n_kf, int n_lm, int n_points, int nnz, size_t tb, bool g) {
    Old W;
    W.get<int>(WE_rowptr, n_kf + 1); W.get<int>(WE_pt, n_lm); W.get<int>(WE_k, n_lm);
    W.get<int>(WE_nrp, g ? 0 : n_points + 1); W.get<int>(WE_col, nnz); W.get<int>(WE_st, nnz); W.get<float>(WE_w, nnz); W.get<float>(WE_d0, nnz);
    W.get<int>(WE_cur, (size_t)n_kf * n_points);
    W.get<int>(WE_cs, (size_t)n_lm + 1); W.get<int>(WE_cd, (size_t)n_lm + 1); W.get<int>(WE_os, (size_t)n_lm + 1); W.get<int>(WE_od, (size_t)n_lm + 1);
    W.get<int>(WE_mark, g ? (size_t)n_points + 1 : 0); W.get<int>(WE_pos, g ? (size_t)n_points + 1 : 0);
    W.get<int>(WE_ids, g ? n_points : 0); W.get<int>(WE_row, g ? n_points : 0);
    W.get<int>(WE_flag, 2);
    W.get<char>(WE_tmp, tb + 256);
    const auto P = dp_winedge_plan(DpWinEdgeIn{(size_t)n_kf, (size_t)n_lm, (size_t)n_points, (size_t)nnz, tb + 256, g});
    check_plan(P, W, W.off + 4096, 4096);
}

// ---- window-edge output: the byte sum in front of pack_ws4 and the four get<> behind it
static void check_winout(int tot0, int tot1) {
    const size_t asked = al(8 * (size_t)tot0) + al(4 * (size_t)tot0) + al(16 * (size_t)tot1) + al(4 * (size_t)tot1) + 4096;
    Old W4;
    W4.get<int>(WO_sp_ij, 2 * (size_t)tot0); W4.get<float>(WO_sp_d0, tot0);
    W4.get<int>(WO_dm_idx, 4 * (size_t)tot1); W4.get<float>(WO_dm_w, tot1);
    check_plan(dp_winout_plan((size_t)tot0, (size_t)tot1), W4, asked, 4096);
}

// ---- embedded-lists scratch: the `layout` of engine_build_embedded_window_device; g: of engine_build_embedded_window_device_rg (the
// resident graph serves the lists: nnz = 0, n_points = its capacity, the tables of the distinct map points behind the CSR form's arrays)
static void check_embwin(int n_kf, int n_obs, int n_points, int nnz, size_t tb, bool g) {
    Old W;
    W.get<int>(EL_pt, n_obs); W.get<int>(EL_k, n_obs); W.get<uint8_t>(EL_node, n_points);
    W.get<int>(EL_nrp, g ? 0 : n_points + 1); W.get<int>(EL_col, nnz); W.get<int>(EL_st, nnz); W.get<float>(EL_w, nnz); W.get<float>(EL_d0, nnz);
    W.get<float>(EL_xyz, 3 * (size_t)n_obs); W.get<float>(EL_uv, 2 * (size_t)n_obs);
    W.get<int>(EL_cur, (size_t)n_kf * n_points);
    W.get<int>(EL_flag, (size_t)n_obs + 1); W.get<int>(EL_lm, (size_t)n_obs + 1);
    W.get<int>(EL_cs, (size_t)n_obs + 1); W.get<int>(EL_cd, (size_t)n_obs + 1); W.get<int>(EL_ck, (size_t)n_obs + 1);
    W.get<int>(EL_os, (size_t)n_obs + 1); W.get<int>(EL_od, (size_t)n_obs + 1); W.get<int>(EL_ok, (size_t)n_obs + 1);
    W.get<int>(EL_tot, 8);
    W.get<int>(EL_krp, (size_t)n_kf + 1); W.get<int>(EL_kfb, 2 * ((size_t)n_kf + 1));
    W.get<char>(EL_tmp, tb + 256);
    if (g) {
        W.get<int>(EL_mark, (size_t)n_points + 1); W.get<int>(EL_pos, (size_t)n_points + 1); W.get<int>(EL_ids, n_points); W.get<int>(EL_row, n_points);
        W.get<int>(EL_ran, 2); W.get<int>(EL_skn, n_obs); W.get<double>(EL_sktot, n_obs);
    }
    const auto P = dp_embwin_plan(DpEmbWinIn{(size_t)n_kf, (size_t)n_obs, (size_t)n_points, (size_t)nnz, tb + 256, g});
    check_plan(P, W, W.off + 4096, 4096);
}

static void check_plans() {
    const int BIG = 0x7FFFFFF0;                                     // near 2^31: every product has to be taken in size_t
    // M, K, n_sp, n_dm, n_rows (a multiple of 256), T, tile rows, tmp bytes
    const struct { int M, K, n_sp, n_dm, n_rows, T, tile; size_t tmp; } p1[] = {
        {0, 0, 0, 0, 0, 8, 32, 0}, {1, 1, 1, 1, 256, 8, 32, 1}, {100000, 20, 600000, 550000, 102400, 2, 128, 5000000 + 1024},
        {3000, 3, 20000, 12000, 3072, 8, 32, 70000}, {BIG, 64, BIG / 2, BIG / 4, 0x7FFFFF00, 2, 128, (size_t)BIG * 3}};
    for (const auto& x : p1) for (int sh = 0; sh < 2; ++sh) check_pack1(x.M, x.K, x.n_sp, x.n_dm, x.n_rows, x.T, x.tile, x.tmp, sh != 0);
    // nnz_s, nnz_d, counted springs / dampers, own incidences, tmp2 bytes ({.. 0, 0, 0, 0 ..}: a rank with an empty share)
    const struct { size_t nnz_s, nnz_d; int ec_nsp, ec_ndm; int64_t own_s, own_d; size_t tmp2; } p2[] = {
        {0, 0, 0, 0, 0, 0, 0}, {64, 64, 1, 1, 2, 4, 1}, {1400000, 2300000, 600000, 550000, 1200000, 2200000, 9000000}, {4096, 0, 0, 0, 0, 0, 1024 + 300},
        {(size_t)BIG, (size_t)BIG, BIG / 2, BIG / 4, BIG, 0xFFFFFFF0LL, (size_t)BIG * 5}};
    for (const auto& x : p2) for (int sh = 0; sh < 2; ++sh) check_pack2(x.nnz_s, x.nnz_d, x.ec_nsp, x.ec_ndm, x.own_s, x.own_d, x.tmp2, sh != 0);
    // n_kf, n_lm, n_points, nnz, scan bytes; the resident-graph form has nnz = 0 and as many points as the graph holds
    const struct { int n_kf, n_lm, n_points, nnz; size_t tb; } we[] = {
        {0, 0, 0, 0, 0}, {1, 1, 1, 1, 1}, {20, 100000, 5000, 60000, 33000}, {4, 300, 2000000, 0, 700000}, {64, BIG, 0x40000000, BIG, (size_t)BIG}};
    for (const auto& x : we) {
        check_winedge(x.n_kf, x.n_lm, x.n_points, x.nnz, x.tb, false);
        check_winedge(x.n_kf, x.n_lm, x.n_points, 0, x.tb, true);
        check_embwin(x.n_kf, x.n_lm, x.n_points, x.nnz, x.tb, false);
        check_embwin(x.n_kf, x.n_lm, x.n_points, 0, x.tb, true);
    }
    const int wo[][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}, {600000, 550000}, {63, 65}, {BIG, BIG}};
    for (const auto& x : wo) check_winout(x[0], x[1]);
}

static void check_decisions() {
    // the two host scans
    const uint8_t plain = RF_OBS | RF_REPROJ_ACTIVE;
    const uint8_t f0[4] = {plain, plain, plain, plain}, f1[4] = {plain, plain, RF_OBS, plain}, f2[4] = {plain, plain, plain, (uint8_t)(plain | RF_FIXED)};
    const int d0[8] = {0, 1, 2, 3, 3, 2, 1, 0}, d1[8] = {0, 1, 2, 3, 3, 2, 1, -1};
    CHECK(dp_precheck(4, f0, 2, d0) == DP_BUILT && dp_precheck(0, f0, 0, d0) == DP_BUILT && dp_precheck(4, f0, 2, nullptr) == DP_BUILT);
    CHECK(dp_precheck(4, f1, 2, d0) == DP_NOT_PLAIN_VERTEX && dp_precheck(4, f2, 2, d1) == DP_NOT_PLAIN_VERTEX && dp_precheck(3, f2, 2, d0) == DP_BUILT);
    CHECK(dp_precheck(4, f0, 2, d1) == DP_INCOMPLETE_DAMPER && dp_precheck(4, f0, 1, d1) == DP_BUILT);
    for (int r = DP_BUILT; r <= DP_GATHER_PATH; ++r) CHECK(dp_reason_name((DpReason)r)[0] != 0);
    // tile range: the tiles whose rows all lie in [lo, hi), by brute force over the tiles
    for (int tile : {32, 128})
        for (int lo = 0; lo <= 1024; lo += 256)
            for (int hi = lo; hi <= 1280; hi += 256) {
                int tb0, tb1, first = -1, n = 0;
                dp_tile_range(lo, hi, tile, tb0, tb1);
                for (int b = 0; b < 1280 / tile; ++b) if (b * tile >= lo && (b + 1) * tile <= hi) { if (first < 0) first = b; ++n; }
                CHECK(tb1 - tb0 == n && (n == 0 || tb0 == first) && tb0 * tile == lo && tb1 * tile == hi);
            }
    // row_bits: the smallest b with every row below 2^b (one bit for a window of one row)
    for (int n_rows : {1, 2, 3, 256, 257, 2048, 32768, 32769, 0x7FFFFF00}) {
        int b = 1;
        while (((int64_t)1 << b) < n_rows) ++b;
        CHECK(dp_row_bits(n_rows) == b);
    }
    // ec_nblk: a workgroup per BLK counted edges, 2048 at the most
    CHECK(dp_ec_nblk(0, 0) == 0 && dp_ec_nblk(1, 0) == 1 && dp_ec_nblk(200, 56) == 1 && dp_ec_nblk(200, 57) == 2 && dp_ec_nblk(600000, 550000) == 2048 &&
          dp_ec_nblk(BLK * 2047, 1) == 2048 && dp_ec_nblk(BLK * 2047, 0) == 2047);
    // halo_ptr
    const VI hs = {3, 0, 5, 0, 0, 2048, 1};
    const VI hp = dp_halo_ptr(hs);
    CHECK(hp.size() == hs.size() + 1 && dp_halo_ptr(VI{}) == VI{0});
    for (size_t b = 0; b <= hs.size(); ++b) { int sum = 0; for (size_t i = 0; i < b; ++i) sum += hs[i]; CHECK(hp[b] == sum); }
    // the reach fix-up: the rank's tiles without halo rows, and only those (the words of other ranks' tiles are never written nor read)
    for (int tb0 = 0; tb0 <= 7; ++tb0)
        for (int tb1 = tb0; tb1 <= 7; ++tb1) {
            VI mn(7), mx(7);
            for (int b = 0; b < 7; ++b) { mn[b] = 100 + b; mx[b] = 200 + b; }
            dp_empty_tile_reach(hs, tb0, tb1, mn, mx);
            for (int b = 0; b < 7; ++b) {
                const bool fixed = b >= tb0 && b < tb1 && hs[b] == 0;
                CHECK(mn[b] == (fixed ? INT_MAX : 100 + b) && mx[b] == (fixed ? -1 : 200 + b));
            }
        }
}

int main() {
    check_plans();
    check_decisions();
    std::printf("devpack_check OK: pack scratch 1 and 2 on one GPU and on a rank, window-edge scratch in the CSR and resident-graph forms, window-edge output, "
                "embedded-lists scratch -- zeros, ones, C2-like sizes, an empty share, counts near 2^31 -- against the bump-allocator sequences and byte "
                "sums they replace; fall-back reasons, tile range, row_bits, ec_nblk, halo_ptr, the empty-tile reach fix-up\n");
    return 0;
}
