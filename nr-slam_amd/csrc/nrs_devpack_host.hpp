// Host pieces of the device-side problem construction (nrs_engine_devpack.hpp, nrs_engine_winedges.hpp, nrs_engine_embwin.hpp): the
// scratch plans of its device buffers, the reasons a window falls back to the host packer, and the small host decisions of the staged
// build.  Plain C++17, no HIP: host/devpack_check.cpp runs all of it under sanitizers (`make devpack_check`).
#pragma once
#include <algorithm>
#include <cassert>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "nrs_engine_consts.hpp"

namespace nrs {

// ---- scratch plans: every array of a buffer stated ONCE (element size and count, in the buffer's order).  dp_place gives the offsets and
// what to ask `ensure` for; DpPlan::at hands out the typed pointers from the buffer's base and asserts the element size.  Placement: every
// array present is rounded up to 256 bytes and followed by 256 bytes of slack (an array of count 0 takes its slack); an array that is NOT
// present takes nothing.
struct DpArr { int r; size_t elem, count; bool present; };
template <int N> struct DpPlan {
    size_t off[N], bytes[N], elem[N], total = 0, need = 0;          // need = total + the buffer's fixed margin
    template <class T> T* at(char* base, int r) const {             // (the element type asked for is the one the table states)
        assert(sizeof(T) == elem[r]);
        return reinterpret_cast<T*>(base + off[r]);
    }
};
template <int N> inline DpPlan<N> dp_place(const DpArr (&t)[N], size_t margin) {
    DpPlan<N> P;
    for (int i = 0; i < N; ++i) {
        const size_t b = t[i].present ? t[i].elem * t[i].count : 0;
        P.off[t[i].r] = P.total; P.bytes[t[i].r] = b; P.elem[t[i].r] = t[i].elem;
        if (t[i].present) P.total += ((b + 255) / 256) * 256 + 256;
    }
    P.need = P.total + margin;
    return P;
}
constexpr size_t DP_MARGIN = 4096, DP_MARGIN2 = (size_t)1 << 16;     // behind the plan's total: pack scratch 1, window scratch and output; pack scratch 2

// pack scratch 1 (nrs_ctx::pack_ws): the caller's arrays as they are + the intermediates sized from the inputs.  keys: the (row, sequence)
// keys of EVERY incidence, on one GPU; a rank of a sharded window keeps the keys of its share in scratch 2
enum DpPack1 {
    P1_r_x, P1_r_kf, P1_r_uv, P1_r_sp, P1_r_d0, P1_r_dm, P1_r_w, P1_code_a, P1_code_b, P1_val_a, P1_val_b, P1_cs, P1_cd, P1_pose_ptr, P1_pgp, P1_tile_off,
    P1_vrow, P1_row_v, P1_tk_a, P1_tk_b, P1_tv_a, P1_tv_b, P1_cnt_s, P1_cnt_d, P1_rs_s, P1_rs_d, P1_key_s, P1_key_s2, P1_key_d, P1_key_d2,
    P1_ws, P1_wd, P1_ss, P1_sd, P1_tmp, P1_mm, P1_hs, P1_hns, P1_hmin, P1_hmax, P1_flag, P1_COUNT
};
struct DpPack1In { size_t M, K, n_sp, n_dm, n_rows, n_slices, n_tiles, tmp_bytes; bool keys; };
inline DpPlan<P1_COUNT> dp_pack1_plan(const DpPack1In& n) {
    const size_t I = 4, F = 4, D = 8, U = 8;                        // bytes of an int / uint32_t, a float, a double, a uint64_t
    const DpArr t[P1_COUNT] = {
        {P1_r_x, D, 3 * n.M, true}, {P1_r_kf, I, n.M, true}, {P1_r_uv, F, 2 * n.M, true},
        {P1_r_sp, I, 2 * n.n_sp, true}, {P1_r_d0, F, n.n_sp, true}, {P1_r_dm, I, 4 * n.n_dm, true}, {P1_r_w, F, n.n_dm, true},
        {P1_code_a, U, n.M, true}, {P1_code_b, U, n.M, true}, {P1_val_a, I, n.M, true}, {P1_val_b, I, n.M, true}, {P1_cs, I, n.M, true}, {P1_cd, I, n.M, true},
        {P1_pose_ptr, I, n.K + 1, true}, {P1_pgp, I, n.K + 1, true}, {P1_tile_off, I, n.n_tiles + 1, true},
        {P1_vrow, I, n.M, true}, {P1_row_v, I, n.n_rows, true},
        {P1_tk_a, I, n.n_rows, true}, {P1_tk_b, I, n.n_rows, true}, {P1_tv_a, I, n.n_rows, true}, {P1_tv_b, I, n.n_rows, true},
        {P1_cnt_s, I, n.n_rows + 1, true}, {P1_cnt_d, I, n.n_rows + 1, true}, {P1_rs_s, I, n.n_rows + 1, true}, {P1_rs_d, I, n.n_rows + 1, true},
        {P1_key_s, U, 2 * n.n_sp, n.keys}, {P1_key_s2, U, 2 * n.n_sp, n.keys}, {P1_key_d, U, 4 * n.n_dm, n.keys}, {P1_key_d2, U, 4 * n.n_dm, n.keys},
        {P1_ws, I, n.n_slices + 1, true}, {P1_wd, I, n.n_slices + 1, true}, {P1_ss, I, n.n_slices + 1, true}, {P1_sd, I, n.n_slices + 1, true},
        {P1_tmp, 1, n.tmp_bytes, true}, {P1_mm, D, 8, true},
        {P1_hs, I, n.n_tiles, true}, {P1_hns, I, n.n_tiles, true}, {P1_hmin, I, n.n_tiles, true}, {P1_hmax, I, n.n_tiles, true}, {P1_flag, I, 16, true}};
    return dp_place(t, DP_MARGIN);
}

// pack scratch 2 (pack_ws2): the sliced-ELL intermediates with GLOBAL neighbour rows and the chi2 edge keys, sized from what is held
// here; keys: on a rank of a sharded window also the keys of its share and the temporary storage of their sorts
enum DpPack2 { P2_S_other, P2_S_side, P2_D_o, P2_D_role, P2_ek_s, P2_ek_s2, P2_ek_d, P2_ek_d2, P2_t_d0, P2_t_w, P2_key_s, P2_key_s2, P2_key_d, P2_key_d2, P2_tmp, P2_COUNT };
struct DpPack2In { size_t nnz_s, nnz_d, ec_nsp, ec_ndm, own_s, own_d, tmp_bytes; bool keys; };
inline DpPlan<P2_COUNT> dp_pack2_plan(const DpPack2In& n) {
    const size_t I = 4, F = 4, U = 8;
    const DpArr t[P2_COUNT] = {
        {P2_S_other, I, n.nnz_s, true}, {P2_S_side, 1, n.nnz_s, true}, {P2_D_o, I, 3 * n.nnz_d, true}, {P2_D_role, 1, n.nnz_d, true},
        {P2_ek_s, U, n.ec_nsp, true}, {P2_ek_s2, U, n.ec_nsp, true}, {P2_ek_d, U, n.ec_ndm, true}, {P2_ek_d2, U, n.ec_ndm, true},
        {P2_t_d0, F, n.nnz_s, true}, {P2_t_w, F, n.nnz_d, true},
        {P2_key_s, U, n.own_s, n.keys}, {P2_key_s2, U, n.own_s, n.keys}, {P2_key_d, U, n.own_d, n.keys}, {P2_key_d2, U, n.own_d, n.keys}, {P2_tmp, 1, n.tmp_bytes, n.keys}};
    return dp_place(t, DP_MARGIN2);
}

// window-edge scratch (pack_ws3, nrs_engine_winedges.hpp).  CSR form: the caller's n_points lists of nnz entries; rg form (the resident
// graph serves the lists): nnz = 0, n_points = the graph's capacity, and the mark / scan / id / list-row tables of the distinct map points
enum DpWinEdge { WE_rowptr, WE_pt, WE_k, WE_nrp, WE_col, WE_st, WE_w, WE_d0, WE_cur, WE_cs, WE_cd, WE_os, WE_od, WE_mark, WE_pos, WE_ids, WE_row, WE_flag, WE_tmp, WE_COUNT };
struct DpWinEdgeIn { size_t n_kf, n_lm, n_points, nnz, tmp_bytes; bool rg; };
inline DpPlan<WE_COUNT> dp_winedge_plan(const DpWinEdgeIn& n) {
    const size_t I = 4, F = 4;
    const DpArr t[WE_COUNT] = {
        {WE_rowptr, I, n.n_kf + 1, true}, {WE_pt, I, n.n_lm, true}, {WE_k, I, n.n_lm, true},
        {WE_nrp, I, n.rg ? 0 : n.n_points + 1, true}, {WE_col, I, n.nnz, true}, {WE_st, I, n.nnz, true}, {WE_w, F, n.nnz, true}, {WE_d0, F, n.nnz, true},
        {WE_cur, I, n.n_kf * n.n_points, true},
        {WE_cs, I, n.n_lm + 1, true}, {WE_cd, I, n.n_lm + 1, true}, {WE_os, I, n.n_lm + 1, true}, {WE_od, I, n.n_lm + 1, true},
        {WE_mark, I, n.rg ? n.n_points + 1 : 0, true}, {WE_pos, I, n.rg ? n.n_points + 1 : 0, true}, {WE_ids, I, n.rg ? n.n_points : 0, true}, {WE_row, I, n.rg ? n.n_points : 0, true},
        {WE_flag, I, 2, true}, {WE_tmp, 1, n.tmp_bytes, true}};
    return dp_place(t, DP_MARGIN);
}

// window-edge output (pack_ws4): the edge lists as nrs_dba_build_edges leaves them, n_sp springs and n_dm dampers
enum DpWinOut { WO_sp_ij, WO_sp_d0, WO_dm_idx, WO_dm_w, WO_COUNT };
inline DpPlan<WO_COUNT> dp_winout_plan(size_t n_sp, size_t n_dm) {
    const size_t I = 4, F = 4;
    const DpArr t[WO_COUNT] = {{WO_sp_ij, I, 2 * n_sp, true}, {WO_sp_d0, F, n_sp, true}, {WO_dm_idx, I, 4 * n_dm, true}, {WO_dm_w, F, n_dm, true}};
    return dp_place(t, DP_MARGIN);
}

// embedded-lists scratch (pack_ws3, nrs_engine_embwin.hpp): n_obs observations of n_kf keyframes over n_points lists of nnz entries.
// rg form (the resident graph serves the lists, as for the window-edge scratch): nnz = 0, n_points = the graph's capacity, and behind the
// CSR form's arrays the mark / scan / id / list-row tables of the distinct map points, the two words of the ran-off flag, and per observation
// the accepted count and the fp64 weight sum the count pass leaves for the emit pass
enum DpEmbWin {
    EL_pt, EL_k, EL_node, EL_nrp, EL_col, EL_st, EL_w, EL_d0, EL_xyz, EL_uv, EL_cur, EL_flag, EL_lm, EL_cs, EL_cd, EL_ck, EL_os, EL_od, EL_ok, EL_tot, EL_krp, EL_kfb, EL_tmp,
    EL_mark, EL_pos, EL_ids, EL_row, EL_ran, EL_skn, EL_sktot, EL_COUNT
};
struct DpEmbWinIn { size_t n_kf, n_obs, n_points, nnz, tmp_bytes; bool rg = false; };
inline DpPlan<EL_COUNT> dp_embwin_plan(const DpEmbWinIn& n) {
    const size_t I = 4, F = 4;
    const DpArr t[EL_COUNT] = {
        {EL_pt, I, n.n_obs, true}, {EL_k, I, n.n_obs, true}, {EL_node, 1, n.n_points, true},
        {EL_nrp, I, n.rg ? 0 : n.n_points + 1, true}, {EL_col, I, n.nnz, true}, {EL_st, I, n.nnz, true}, {EL_w, F, n.nnz, true}, {EL_d0, F, n.nnz, true},
        {EL_xyz, F, 3 * n.n_obs, true}, {EL_uv, F, 2 * n.n_obs, true}, {EL_cur, I, n.n_kf * n.n_points, true},
        {EL_flag, I, n.n_obs + 1, true}, {EL_lm, I, n.n_obs + 1, true}, {EL_cs, I, n.n_obs + 1, true}, {EL_cd, I, n.n_obs + 1, true}, {EL_ck, I, n.n_obs + 1, true},
        {EL_os, I, n.n_obs + 1, true}, {EL_od, I, n.n_obs + 1, true}, {EL_ok, I, n.n_obs + 1, true},
        {EL_tot, I, 8, true}, {EL_krp, I, n.n_kf + 1, true}, {EL_kfb, I, 2 * (n.n_kf + 1), true}, {EL_tmp, 1, n.tmp_bytes, true},
        {EL_mark, I, n.n_points + 1, n.rg}, {EL_pos, I, n.n_points + 1, n.rg}, {EL_ids, I, n.n_points, n.rg}, {EL_row, I, n.n_points, n.rg}, {EL_ran, I, 2, n.rg},
        {EL_skn, I, n.n_obs, n.rg}, {EL_sktot, 8, n.n_obs, n.rg}};
    return dp_place(t, DP_MARGIN);
}

// ---- why a window is built by the host packer after all (engine_create; printed under NRS_TIMING, observed by nothing else)
enum DpReason { DP_BUILT, DP_INELIGIBLE, DP_NOT_PLAIN_VERTEX, DP_INCOMPLETE_DAMPER, DP_HALO_BEYOND_LIMITS, DP_GATHER_PATH };
inline const char* dp_reason_name(DpReason r) {
    static const char* const name[] = {"built on the device", "ineligible up front", "a vertex that is not plain", "an incomplete damper", "a halo beyond the limits",
                                       "the gather path chosen"};
    return name[r];
}
// the two host scans in front of the build: every vertex observed with its reprojection active; no absent damper vertex (-1 is valid for
// engine_create, but the device kernels index by these values).  dm_idx = null: the edges were built on the device, complete by construction
inline DpReason dp_precheck(int M, const uint8_t* rflag, int n_dm, const int* dm_idx) {
    unsigned odd = 0;                                               // (no early exit in either scan: a window that fails is the rare case, and
    for (int v = 0; v < M; ++v) odd |= (unsigned)(rflag[v] ^ (RF_OBS | RF_REPROJ_ACTIVE));   //  reductions vectorise -- 2.2 M indices at C2)
    if (odd) return DP_NOT_PLAIN_VERTEX;
    int neg = 0;
    if (dm_idx)
        for (int64_t q = 0; q < 4 * (int64_t)n_dm; ++q) neg |= dm_idx[q];
    return neg < 0 ? DP_INCOMPLETE_DAMPER : DP_BUILT;
}

// ---- host decisions of the build
// the tiles [tb0, tb1) of the rows [pack_lo, pack_hi) a build packs (both ends on tile boundaries: keyframes are padded to ROW_ALIGN rows)
inline void dp_tile_range(int pack_lo, int pack_hi, int tile_rows, int& tb0, int& tb1) { tb0 = pack_lo / tile_rows; tb1 = pack_hi / tile_rows; }
// significant bits of a row number: the radix sorts of (row << 32 | sequence) keys look at 32 + row_bits bits
inline int dp_row_bits(int n_rows) { return 32 - __builtin_clz((unsigned)std::max(1, n_rows - 1)); }
// workgroups of the chi2 pass over the counted edges
inline int dp_ec_nblk(int ec_nsp, int ec_ndm) { return std::min((ec_nsp + ec_ndm + BLK - 1) / BLK, 2048); }
// offsets of the tiles' halo lists from their sizes
inline std::vector<int> dp_halo_ptr(const std::vector<int>& hs) {
    std::vector<int> p(hs.size() + 1, 0);
    for (size_t b = 0; b < hs.size(); ++b) p[b + 1] = p[b] + hs[b];
    return p;
}
// a rank's smallest / largest halo row per tile: pass 0 of k_dp_halo leaves the two words of a tile without halo rows unwritten, and writes
// those of the rank's own tiles [tb0, tb1) only
inline void dp_empty_tile_reach(const std::vector<int>& hs, int tb0, int tb1, std::vector<int>& hmin, std::vector<int>& hmax) {
    for (int b = tb0; b < tb1; ++b) if (!hs[b]) { hmin[b] = INT_MAX; hmax[b] = -1; }
}

}  // namespace nrs
