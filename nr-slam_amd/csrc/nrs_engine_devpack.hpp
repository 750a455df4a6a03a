// Device-side problem construction for plain deformable-BA windows (part of nrs_engine.hip; see nrs_engine_setup.hpp for the
// host form it reproduces BIT FOR BIT -- tests/test_gpu_devpack.py compares checksums of every packed array).
//
// LocalDeformableBundleAdjustment is called with a NEW window at every keyframe (reference modules/mapping/mapping.cc:57), so
// what a drop-in caller pays is the one-shot nrs_dba_solve: with the packing on a few host threads that was 69-90 ms at C2 for
// a 2.7 ms solve.  Here the caller's arrays (OPT:927-1137's edges as nrs_dba_build_edges leaves them) are uploaded as they are
// and everything else happens on the device, in the order and with the tie-breaks of the host code:
//   row layout      Morton code of every vertex (same fp64 expression), segmented radix sort per keyframe (stable: ties by vertex
//                   index), then inside every 128-row tile a stable sort by (damper, spring) incidence counts
//   sliced ELL      incidence counts per row (integer atomics), slice widths, scans; the k-th incidence of a row is the k-th in
//                   edge order: radix sort of (row, edge sequence) keys
//   halo lists      one workgroup per tile: LDS hash set of the rows referenced outside the tile, spring-referenced rows first,
//                   each part ascending (bitonic sort in LDS), tile-local ids by binary search, headers written in final form
//   chi2 edge lists edges ordered by the row that counts them (stable): radix sort of (row, edge) keys
// The host keeps what it needs to drive the solve: the vertex -> row map (download), the tile classes (from the halo sizes).
// Conditions (otherwise engine_create takes the host path): a plain BA window (nothing fixed, no masks, offsets or unary
// dampers, every damper with four vertices, springs without kernel) of >= 2 keyframes and >= 2048 padded rows -- the two-kernel
// path (>= 32768 rows, T = 2) and the fused one (T = 8) alike -- halos that fit the LDS budget, at most 2048 halo rows per tile.
// NRS_HOST_PACK=1 forces the host path, and so does every A/B switch that path honours (devpack_eligible).
//
// On a communicator (a world of one included) every rank runs this construction for ITSELF, without a collective: the row layout
// is the window's (integer sorts and one fp64 expression: the same vrow on every rank, O(window) work), everything behind it is
// the rank's share -- the (row, edge) keys of rows in [pack_lo, pack_hi) only (k_dp_count_own / k_dp_keys_own compact them; the
// sorts, k_dp_fill_s/d, both halo passes over the rank's own tiles and the chi2 edge lists see nothing else), rows of other ranks
// keep empty lists.  A sharded window is always on the two-kernel PCG, so a window under 32768 rows is two-kernel with T = 8 here.
// The shard fields (tile ranges per class, boundary tiles, the adjacent-keyframe check) come from the per-tile minimum / maximum
// halo row that pass 0 leaves, BEFORE the arena is carved: a rank's per-row arrays hold its own keyframes and one ghost keyframe
// either side only (ArenaPlan::get_rows), and every kernel here that writes one is bounded to [row_lo, row_hi).  A rank whose
// window does not qualify after all takes the host path on its own: the two constructions give the same bits.
#pragma once
#include <rocprim/rocprim.hpp>
#include "nrs_devpack_host.hpp"

namespace nrs {

static bool devpack_eligible(nrs_ctx* c, const EngineSpec& s, int n_pad_rows) {
    if (c->dbg.forces_host_pack())                                 // (a switch marked HOST_PACK in nrs_switches.hpp is set)
        return false;                                                // (test / A-B switches are honoured by the host path)
    // a communicator: one window over its ranks, with a rank count the sharded path accepts (engine_create has refused the others)
    if (c->comm && (!s.shard || c->comm->world > 8 || s.K < c->comm->world)) return false;
    if (s.X0 || s.n_un || s.sp_active || s.dm_active || s.pose_fixed || s.force_gather || s.sk_window() > 0) return false;
    if (s.K < 2 || n_pad_rows < 2048 || s.delta_pos > 0 || s.spring_form != 0 || s.n_dm <= 0 || s.n_sp <= 0) return false;   // (single-frame problems: a2, host)
    if (4 * (int64_t)s.n_dm >= 0xFFFFFFFFLL || (int64_t)n_pad_rows >= 0x7FFFFFFFLL) return false;
    return true;
}

bool engine_device_pack_ok(nrs_ctx* c, const EngineSpec& s) { return devpack_eligible(c, s, row_groups(s).n_pad_rows); }

// ---- the staged build (DeviceBuild: nrs_engine_setup.hpp, next to the host packer's; engine_create calls the stages in this order).
// Every stage enqueues on the context's stream in the order of the host packer's steps and ends at its NRS_TIMING line.

// false: the window is for the host packer, `why` says why.  Two host scans behind the eligibility: O(window), no device work yet
bool DeviceBuild::precheck() {
    if (!devpack_eligible(c, s, g.n_pad_rows)) { why = DP_INELIGIBLE; return false; }
    mark.t_prev = std::chrono::steady_clock::now();                  // (the "uploads" lap starts behind the eligibility test)
    why = dp_precheck(s.M, s.rflag, s.n_dm, s.edges_on_device ? nullptr : s.dm_idx);
    return why == DP_BUILT;
}

// ---- scratch 1 and the caller's arrays, as they are
int DeviceBuild::uploads() {
    dev_init(d, s, g, T);
    n_rows = d.n_rows; n_slices = n_rows / (64 / T); n_tiles = d.n_regblk;
    row_bits = dp_row_bits(n_rows);
    pack_range(c, s, g, pack_lo, pack_hi);
    dp_tile_range(pack_lo, pack_hi, d.tile_rows, tb0, tb1);
    {
        size_t b1 = 0, b2 = 0, b3 = 0, b4 = 0;
        if (!sh) (void)rocprim::radix_sort_keys(nullptr, b1, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)std::max(ni_s, ni_d), 0, 64, c->stream);   // (a rank: sized from its share, scratch2)
        (void)rocprim::segmented_radix_sort_pairs(nullptr, b2, (uint64_t*)nullptr, (uint64_t*)nullptr, (int*)nullptr, (int*)nullptr, (size_t)M, (unsigned)K,
                                                  (int*)nullptr, (int*)nullptr, 0, 64, c->stream);
        (void)rocprim::segmented_radix_sort_pairs(nullptr, b3, (uint32_t*)nullptr, (uint32_t*)nullptr, (int*)nullptr, (int*)nullptr, (size_t)n_rows,
                                                  (unsigned)n_tiles, (int*)nullptr, (int*)nullptr, 0, 32, c->stream);
        (void)rocprim::exclusive_scan(nullptr, b4, (int*)nullptr, (int*)nullptr, 0, (size_t)n_rows + 1, rocprim::plus<int>(), c->stream);
        tmp_bytes = std::max(std::max(b1, b2), std::max(b3, b4)) + 1024;
    }
    const auto P = dp_pack1_plan(DpPack1In{(size_t)M, (size_t)K, (size_t)n_sp, (size_t)n_dm, (size_t)n_rows, (size_t)n_slices, (size_t)n_tiles, tmp_bytes, !sh});
    NRS_TRY(c->ensure(c->pack_ws, P.need));
    char* const w = c->pack_ws.as<char>();
    auto I = [&](int r) { return P.at<int>(w, r); };
    auto U = [&](int r) { return P.at<uint64_t>(w, r); };
    r_x = P.at<double>(w, P1_r_x); r_kf = I(P1_r_kf); r_uv = P.at<float>(w, P1_r_uv);
    r_sp = I(P1_r_sp); r_d0 = P.at<float>(w, P1_r_d0); r_dm = I(P1_r_dm); r_w = P.at<float>(w, P1_r_w);
    code_a = U(P1_code_a); code_b = U(P1_code_b); val_a = I(P1_val_a); val_b = I(P1_val_b); cs = I(P1_cs); cd = I(P1_cd);
    d_pose_ptr = I(P1_pose_ptr); d_pgp = I(P1_pgp); tile_off = I(P1_tile_off); vrow = I(P1_vrow); row_v = I(P1_row_v);
    tk_a = P.at<uint32_t>(w, P1_tk_a); tk_b = P.at<uint32_t>(w, P1_tk_b); tv_a = I(P1_tv_a); tv_b = I(P1_tv_b);
    cnt_s = I(P1_cnt_s); cnt_d = I(P1_cnt_d); rs_s = I(P1_rs_s); rs_d = I(P1_rs_d);
    if (!sh) { key_s = U(P1_key_s); key_s2 = U(P1_key_s2); key_d = U(P1_key_d); key_d2 = U(P1_key_d2); }
    ws = I(P1_ws); wd = I(P1_wd); d_ss = I(P1_ss); d_sd = I(P1_sd); tmp = P.at<char>(w, P1_tmp); mm = P.at<double>(w, P1_mm);
    hs = I(P1_hs); hns = I(P1_hns); hmin = I(P1_hmin); hmax = I(P1_hmax); d_flag = I(P1_flag);
    NRS_HIP(c, hipMemcpyAsync(r_x, s.x, sizeof(double) * 3 * (size_t)M, hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(r_kf, s.lm_pose, sizeof(int) * (size_t)M, hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(r_uv, s.uv, sizeof(float) * 2 * (size_t)M, hipMemcpyHostToDevice, st));
    const hipMemcpyKind ek = s.edges_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;      // (nrs_dba_solve_window builds them there)
    NRS_HIP(c, hipMemcpyAsync(r_sp, s.sp_ij, sizeof(int) * 2 * (size_t)n_sp, ek, st));
    NRS_HIP(c, hipMemcpyAsync(r_d0, s.sp_d0, sizeof(float) * (size_t)n_sp, ek, st));
    NRS_HIP(c, hipMemcpyAsync(r_dm, s.dm_idx, sizeof(int) * 4 * (size_t)n_dm, ek, st));
    NRS_HIP(c, hipMemcpyAsync(r_w, s.dm_w, sizeof(float) * (size_t)n_dm, ek, st));
    NRS_HIP(c, hipMemcpyAsync(d_pose_ptr, g.pose_ptr.data(), sizeof(int) * (K + 1), hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(d_pgp, g.pose_grp_ptr.data(), sizeof(int) * (K + 1), hipMemcpyHostToDevice, st));
    std::vector<int> to(n_tiles + 1);
    for (int i = 0; i <= n_tiles; ++i) to[i] = i * d.tile_rows;
    NRS_HIP(c, hipMemcpyAsync(tile_off, to.data(), sizeof(int) * (n_tiles + 1), hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipStreamSynchronize(st));                            // (`to` dies here)
    mark("uploads");
    return NRS_OK;
}

// ---- row layout: Morton order inside a keyframe, then (damper, spring) incidence counts inside a tile
int DeviceBuild::row_layout() {
    hipLaunchKernelGGL(k_dp_minmax, dim3(1), dim3(1024), 0, st, M, r_x, mm);
    hipLaunchKernelGGL(k_dp_morton, nb(M), dim3(256), 0, st, M, r_x, mm, c->dbg.is_set(SW_NO_MORTON) ? 0 : 1, code_a, val_a);
    size_t tb = tmp_bytes;
    NRS_HIP(c, rocprim::segmented_radix_sort_pairs(tmp, tb, code_a, code_b, val_a, val_b, (size_t)M, (unsigned)K, d_pose_ptr, d_pose_ptr + 1, 0, 64, st));
    NRS_HIP(c, hipMemsetAsync(row_v, 0xFF, sizeof(int) * (size_t)n_rows, st));
    hipLaunchKernelGGL(k_dp_rows0, nb(M), dim3(256), 0, st, M, val_b, r_kf, d_pose_ptr, d_pgp, vrow, row_v);
    if (!c->dbg.is_set(SW_NO_TILE_SORT)) {
        NRS_HIP(c, hipMemsetAsync(cs, 0, sizeof(int) * (size_t)M, st));
        NRS_HIP(c, hipMemsetAsync(cd, 0, sizeof(int) * (size_t)M, st));
        hipLaunchKernelGGL(k_dp_vcounts, nb(std::max(ni_s, ni_d)), dim3(256), 0, st, n_sp, r_sp, n_dm, r_dm, cs, cd);
        hipLaunchKernelGGL(k_dp_tilekeys, nb(n_rows), dim3(256), 0, st, n_rows, row_v, cs, cd, tk_a, tv_a);
        tb = tmp_bytes;
        NRS_HIP(c, rocprim::segmented_radix_sort_pairs(tmp, tb, tk_a, tk_b, tv_a, tv_b, (size_t)n_rows, (unsigned)n_tiles, tile_off, tile_off + 1, 0, 32, st));
        hipLaunchKernelGGL(k_dp_rows1, nb(n_rows), dim3(256), 0, st, n_rows, tv_b, vrow);
        NRS_HIP(c, hipMemsetAsync(row_v, 0xFF, sizeof(int) * (size_t)n_rows, st));
        hipLaunchKernelGGL(k_dp_rowv, nb(M), dim3(256), 0, st, M, vrow, row_v);
    }
    mark("row layout");
    return NRS_OK;
}

// slice widths from the counts per row, the four scans, and the download of the two sliced-ELL sizes (into h_nnz: read after the next synchronise)
int DeviceBuild::slice_offsets() {
    hipLaunchKernelGGL(k_dp_widths, nb(n_slices), dim3(256), 0, st, n_slices, T, cnt_s, cnt_d, ws, wd);
    NRS_HIP(c, hipMemsetAsync(ws + n_slices, 0, sizeof(int), st));
    NRS_HIP(c, hipMemsetAsync(wd + n_slices, 0, sizeof(int), st));
    size_t tb = tmp_bytes; NRS_HIP(c, rocprim::exclusive_scan(tmp, tb, ws, d_ss, 0, (size_t)n_slices + 1, rocprim::plus<int>(), st));
    tb = tmp_bytes; NRS_HIP(c, rocprim::exclusive_scan(tmp, tb, wd, d_sd, 0, (size_t)n_slices + 1, rocprim::plus<int>(), st));
    tb = tmp_bytes; NRS_HIP(c, rocprim::exclusive_scan(tmp, tb, cnt_s, rs_s, 0, (size_t)n_rows + 1, rocprim::plus<int>(), st));
    tb = tmp_bytes; NRS_HIP(c, rocprim::exclusive_scan(tmp, tb, cnt_d, rs_d, 0, (size_t)n_rows + 1, rocprim::plus<int>(), st));
    NRS_HIP(c, hipMemcpyAsync(&h_nnz[0], d_ss + n_slices, sizeof(int), hipMemcpyDeviceToHost, st));
    NRS_HIP(c, hipMemcpyAsync(&h_nnz[1], d_sd + n_slices, sizeof(int), hipMemcpyDeviceToHost, st));
    return NRS_OK;
}

// ---- scratch 2, sized from the share (sr): sliced-ELL intermediates with GLOBAL neighbour rows; on a rank also its keys and the sorts'
// temporary storage
int DeviceBuild::scratch2() {
    if (sr.rank) {
        (void)rocprim::radix_sort_keys(nullptr, tmp2_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)std::max<int64_t>(std::max(sr.own_s, sr.own_d), 1), 0, 64, c->stream);
        tmp2_bytes += 1024;
    }
    const auto P = dp_pack2_plan(DpPack2In{sr.nnz_s, sr.nnz_d, (size_t)sr.ec_nsp, (size_t)sr.ec_ndm, (size_t)sr.own_s, (size_t)sr.own_d, tmp2_bytes, sr.rank});
    NRS_TRY(c->ensure(c->pack_ws2, P.need));
    char* const w = c->pack_ws2.as<char>();
    auto U = [&](int r) { return P.at<uint64_t>(w, r); };
    S_other = P.at<int>(w, P2_S_other); S_side = P.at<uint8_t>(w, P2_S_side); D_o = P.at<int>(w, P2_D_o); D_role = P.at<int8_t>(w, P2_D_role);
    ek_s = U(P2_ek_s); ek_s2 = U(P2_ek_s2); ek_d = U(P2_ek_d); ek_d2 = U(P2_ek_d2);
    t_d0 = P.at<float>(w, P2_t_d0); t_w = P.at<float>(w, P2_t_w);
    if (sr.rank) { key_s = U(P2_key_s); key_s2 = U(P2_key_s2); key_d = U(P2_key_d); key_d2 = U(P2_key_d2); tmp2 = P.at<char>(w, P2_tmp); }
    return NRS_OK;
}

// one GPU: every incidence is held here.  Keys with the counts; the sorts run while the host waits for the two sizes
int DeviceBuild::incidences_whole() {
    hipLaunchKernelGGL(k_dp_inc, nb(std::max(ni_s, ni_d)), dim3(256), 0, st, n_sp, r_sp, n_dm, r_dm, vrow, cnt_s, cnt_d, key_s, key_d);
    NRS_TRY(slice_offsets());
    size_t tb = tmp_bytes; NRS_HIP(c, rocprim::radix_sort_keys(tmp, tb, key_s, key_s2, (size_t)ni_s, 0, 32 + row_bits, st));
    tb = tmp_bytes; NRS_HIP(c, rocprim::radix_sort_keys(tmp, tb, key_d, key_d2, (size_t)ni_d, 0, 32 + row_bits, st));
    NRS_HIP(c, hipStreamSynchronize(st));
    sr = DpShare{ni_s, ni_d, n_sp, n_dm, (size_t)h_nnz[0], (size_t)h_nnz[1], false};
    mark("counts + sorts");
    return scratch2();
}

// a rank: counts first -- its keys and their sorts are sized from them (scratch 2) -- then the keys of its rows, compacted, and the
// keys of the edges it counts with them
int DeviceBuild::incidences_own() {
    hipLaunchKernelGGL(k_dp_count_own, nb(std::max(ni_s, ni_d)), dim3(256), 0, st, n_sp, r_sp, n_dm, r_dm, vrow, pack_lo, pack_hi, cnt_s, cnt_d, d_flag + 4);
    NRS_TRY(slice_offsets());
    NRS_HIP(c, hipMemcpyAsync(&h_own[0], rs_s + n_rows, sizeof(int), hipMemcpyDeviceToHost, st));
    NRS_HIP(c, hipMemcpyAsync(&h_own[1], rs_d + n_rows, sizeof(int), hipMemcpyDeviceToHost, st));
    NRS_HIP(c, hipMemcpyAsync(&h_own[2], d_flag + 6, sizeof(int) * 2, hipMemcpyDeviceToHost, st));
    NRS_HIP(c, hipStreamSynchronize(st));
    sr = DpShare{h_own[0], h_own[1], h_own[2], h_own[3], (size_t)h_nnz[0], (size_t)h_nnz[1], true};
    NRS_TRY(scratch2());
    hipLaunchKernelGGL(k_dp_keys_own, nb(std::max(ni_s, ni_d)), dim3(256), 0, st, n_sp, r_sp, n_dm, r_dm, vrow, pack_lo, pack_hi, key_s, key_d, ek_s, ek_d, d_flag + 8);
    size_t t2 = tmp2_bytes; NRS_HIP(c, rocprim::radix_sort_keys(tmp2, t2, key_s, key_s2, (size_t)sr.own_s, 0, 32 + row_bits, st));
    t2 = tmp2_bytes; NRS_HIP(c, rocprim::radix_sort_keys(tmp2, t2, key_d, key_d2, (size_t)sr.own_d, 0, 32 + row_bits, st));
    t2 = tmp2_bytes; NRS_HIP(c, rocprim::radix_sort_keys(tmp2, t2, ek_s, ek_s2, (size_t)sr.ec_nsp, 0, 32 + row_bits, st));
    t2 = tmp2_bytes; NRS_HIP(c, rocprim::radix_sort_keys(tmp2, t2, ek_d, ek_d2, (size_t)sr.ec_ndm, 0, 32 + row_bits, st));
    mark("counts + sorts");
    return NRS_OK;
}

// ---- incidence counts, slice widths, offsets, sorted keys: the one place where the builds of one GPU and of a rank differ in kind.
// Both leave the share (sr), its sorted keys (key_s2, key_d2) and scratch 2; the stages behind read those
int DeviceBuild::incidences() {
    NRS_HIP(c, hipMemsetAsync(cnt_s, 0, sizeof(int) * ((size_t)n_rows + 1), st));
    NRS_HIP(c, hipMemsetAsync(cnt_d, 0, sizeof(int) * ((size_t)n_rows + 1), st));
    NRS_HIP(c, hipMemsetAsync(d_flag, 0, sizeof(int) * 16, st));
    NRS_TRY(sh ? incidences_own() : incidences_whole());
    d.ss_nnz = (int)sr.nnz_s; d.sd_nnz = (int)sr.nnz_d;
    return NRS_OK;
}

// ---- halo sizes (pass 0 needs S_other / D_o: the fill kernels write them into scratch 2 first; S_d0 / D_w are staged there too: the
// arena is carved only once the halo sizes are known), and what the host decides from
int DeviceBuild::fill_and_halo_sizes() {
    const size_t nnz_s = sr.nnz_s, nnz_d = sr.nnz_d;
    NRS_HIP(c, hipMemsetAsync(S_other, 0xFF, sizeof(int) * nnz_s, st));
    NRS_HIP(c, hipMemsetAsync(S_side, 0, nnz_s, st));
    NRS_HIP(c, hipMemsetAsync(D_o, 0xFF, sizeof(int) * 3 * nnz_d, st));
    NRS_HIP(c, hipMemsetAsync(D_role, 0xFF, nnz_d, st));
    NRS_HIP(c, hipMemsetAsync(t_d0, 0, sizeof(float) * nnz_s, st));
    NRS_HIP(c, hipMemsetAsync(t_w, 0, sizeof(float) * nnz_d, st));
    if (sr.own_s) hipLaunchKernelGGL(k_dp_fill_s, nb(sr.own_s), dim3(256), 0, st, sr.own_s, T, key_s2, rs_s, d_ss, r_sp, r_d0, vrow, S_other, t_d0, S_side);
    if (sr.own_d) hipLaunchKernelGGL(k_dp_fill_d, nb(sr.own_d), dim3(256), 0, st, sr.own_d, T, key_d2, rs_d, d_sd, r_dm, r_w, vrow, D_o, t_w, D_role);
    if (sr.rank) {                                                        // (tiles of other ranks: empty lists)
        NRS_HIP(c, hipMemsetAsync(hs, 0, sizeof(int) * n_tiles, st));
        NRS_HIP(c, hipMemsetAsync(hns, 0, sizeof(int) * n_tiles, st));
    }
    hipLaunchKernelGGL((k_dp_halo<0>), dim3(tb1 - tb0), dim3(256), 0, st, tb0, sr.rank ? hmin : (int*)nullptr, sr.rank ? hmax : (int*)nullptr, d.tile_rows, T, (uint16_t*)nullptr, d_ss, d_sd,
                       S_other, S_side, D_o, D_role, hs, hns, (const int*)nullptr, (int*)nullptr, (uint32_t*)nullptr, (uint2*)nullptr, d_flag);
    h_hs.resize(n_tiles); h_hns.resize(n_tiles); h_vrow.resize(M);
    NRS_HIP(c, hipMemcpyAsync(h_hs.data(), hs, sizeof(int) * n_tiles, hipMemcpyDeviceToHost, st));
    NRS_HIP(c, hipMemcpyAsync(h_hns.data(), hns, sizeof(int) * n_tiles, hipMemcpyDeviceToHost, st));
    if (sr.rank) {                                                        // (the shard fields are derived from a tile's smallest / largest halo row)
        h_hmin.resize(n_tiles); h_hmax.resize(n_tiles);
        NRS_HIP(c, hipMemcpyAsync(h_hmin.data() + tb0, hmin + tb0, sizeof(int) * (tb1 - tb0), hipMemcpyDeviceToHost, st));
        NRS_HIP(c, hipMemcpyAsync(h_hmax.data() + tb0, hmax + tb0, sizeof(int) * (tb1 - tb0), hipMemcpyDeviceToHost, st));
    }
    NRS_HIP(c, hipMemcpyAsync(&h_flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    NRS_HIP(c, hipMemcpyAsync(h_vrow.data(), vrow, sizeof(int) * (size_t)M, hipMemcpyDeviceToHost, st));
    NRS_HIP(c, hipStreamSynchronize(st));
    mark("fill + halo sizes");
    return NRS_OK;
}

// ---- the decisions both packers share (nrs_engine_plan.hpp; host, O(tiles)): tile classes, LDS and path flags, the shard window --
// BEFORE the arena is carved.  Leaves `why` set when the window is for the host packer after all
int DeviceBuild::decide() {
    if (h_flag) { why = DP_HALO_BEYOND_LIMITS; return NRS_OK; }      // (a halo beyond the kernel's limits)
    halo_ptr = dp_halo_ptr(h_hs);
    n_halo = (size_t)halo_ptr[n_tiles];
    tile_list = tile_classes(c, d, h_hs, h_hns);
    path_flags(c, d, s);
    if (!d.use_lds) { why = DP_GATHER_PATH; return NRS_OK; }
    // what the host reads off its halo lists -- a row beyond the adjacent keyframes, a row of another rank -- a tile's smallest and
    // largest halo row decide (TileReach)
    if (sr.rank) dp_empty_tile_reach(h_hs, tb0, tb1, h_hmin, h_hmax);
    NRS_TRY(shard_window(c, d, e->halo, s, g, tile_list, TileReach{h_hmin.data(), h_hmax.data(), h_hmin.data(), h_hmax.data()}));
    if (d.row_hi <= 0) { d.row_lo = 0; d.row_hi = n_rows; }         // (unsharded: every row, as carve has it)
    d.ec_on = 1; d.plain = 1;
    d.lin_rb = ROW_ALIGN / (64 / T);
    d.ec_nsp = sr.ec_nsp; d.ec_ndm = sr.ec_ndm;
    d.ec_nblk = dp_ec_nblk(sr.ec_nsp, sr.ec_ndm);
    e->pack_rows = pack_hi - pack_lo;
    if (mark.on) fprintf(stderr, "[nrs] device pack: tiles %d x %d rows, halo rows: max %d, mean %.1f, spring part max %d, classes %d (cap %d/%d) + %d (cap %d/%d)\n", n_tiles, d.tile_rows,
                    d.max_halo, (double)n_halo / n_tiles, d.max_halo_s, d.n_tiles_cls[0], d.cap_h[0], d.cap_s[0], d.n_tiles_cls[1], d.cap_h[1], d.cap_s[1]);
    return NRS_OK;
}

// ---- the arena, then the packed arrays in their final form: pass 1 of the halo kernel writes the lists and the incidence headers
int DeviceBuild::final_arrays() {
    const size_t nnz_s = sr.nnz_s, nnz_d = sr.nnz_d;
    spec_pcg_sets(c, e, 0);                                          // shadow sets for speculative LM trials (carved with the arena)
    NRS_TRY(arena_fit(c, arena, e, d, false, nnz_s, nnz_d, (size_t)n_slices, n_halo));
    mark("arena");
    const int row_lo = d.row_lo, row_hi = d.row_hi;
    NRS_HIP(c, hipMemcpyAsync(d.grp_pose, g.grp_pose.data(), sizeof(int) * g.grp_pose.size(), hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(d.pose_grp_ptr, g.pose_grp_ptr.data(), sizeof(int) * (K + 1), hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(d.halo_ptr, halo_ptr.data(), sizeof(int) * (n_tiles + 1), hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(d.tile_list, tile_list.data(), sizeof(int) * n_tiles, hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(d.halo_ns, hns, sizeof(int) * n_tiles, hipMemcpyDeviceToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(d.ss_ptr, d_ss, sizeof(int) * ((size_t)n_slices + 1), hipMemcpyDeviceToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(d.sd_ptr, d_sd, sizeof(int) * ((size_t)n_slices + 1), hipMemcpyDeviceToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(d.s_d0, t_d0, sizeof(float) * nnz_s, hipMemcpyDeviceToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(d.d_w, t_w, sizeof(float) * nnz_d, hipMemcpyDeviceToDevice, st));
    poses.assign(s.poses, s.poses + K);
    NRS_HIP(c, hipMemcpyAsync(d.pose_init, poses.data(), sizeof(Pose) * K, hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemsetAsync(d.pose_fixed, 0, K, st));
    NRS_HIP(c, hipMemsetAsync(d.row_tp + row_lo, 0xFF, sizeof(uint32_t) * (size_t)(row_hi - row_lo), st));
    hipLaunchKernelGGL((k_dp_halo<1>), dim3(tb1 - tb0), dim3(256), 0, st, tb0, (int*)nullptr, (int*)nullptr, d.tile_rows, T, reinterpret_cast<uint16_t*>(d.row_tp), d.ss_ptr, d.sd_ptr, S_other, S_side, D_o, D_role, hs, hns, d.halo_ptr,
                       d.halo_rows, d.s_om, d.d_hdr, d_flag);
    if (d.fused) {
        const std::vector<int> tile_desc = tile_desc_build(d, g, halo_ptr);
        NRS_HIP(c, hipMemcpyAsync(d.tile_desc, tile_desc.data(), sizeof(int) * tile_desc.size(), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_dp_halofix, dim3(n_tiles), dim3(BLK), 0, st, n_tiles, d.halo_ptr, d.halo_rows, d.halo_fix, BLK, 0);
        NRS_HIP(c, hipStreamSynchronize(st));                        // (tile_desc dies here)
    } else if (d.use_lds)
        hipLaunchKernelGGL(k_dp_halofix, dim3(n_tiles), dim3(BLK), 0, st, n_tiles, d.halo_ptr, d.halo_rows, d.halo_fix, HALO_FIX, -1);
    hipLaunchKernelGGL(k_dp_rowdata, nb(row_hi - row_lo), dim3(256), 0, st, row_lo, row_hi, row_v, r_x, r_uv, d.rflag, d.uv, d.xl_init);
    hipLaunchKernelGGL(k_dp_rowcnt, nb(row_hi - row_lo), dim3(256), 0, st, row_lo, row_hi, cnt_s, cnt_d, d.row_cnt);
    if (!sr.rank) {                                                 // chi2 edge lists: keys (counting row, edge), sorted
        hipLaunchKernelGGL(k_dp_eckeys, nb(std::max(n_sp, n_dm)), dim3(256), 0, st, n_sp, r_sp, n_dm, r_dm, vrow, ek_s, ek_d);
        size_t tb = tmp_bytes; NRS_HIP(c, rocprim::radix_sort_keys(tmp, tb, ek_s, ek_s2, (size_t)n_sp, 0, 32 + row_bits, st));
        tb = tmp_bytes; NRS_HIP(c, rocprim::radix_sort_keys(tmp, tb, ek_d, ek_d2, (size_t)n_dm, 0, 32 + row_bits, st));
    }
    if (sr.ec_nsp + sr.ec_ndm > 0)
        hipLaunchKernelGGL(k_dp_ecfill, nb(std::max(sr.ec_nsp, sr.ec_ndm)), dim3(256), 0, st, sr.ec_nsp, ek_s2, r_sp, r_d0, sr.ec_ndm, ek_d2, r_dm, r_w, vrow, d.ec_sp, d.ec_dm, d.ec_w);
    NRS_TRY(zero_work_arrays(c, d));
    NRS_HIP(c, hipGetLastError());
    return NRS_OK;
}

// ---- host side of the engine: what the host keeps to drive the solve; the overflow word of pass 1 is final after the synchronise
int DeviceBuild::host_side() {
    const int row_lo = d.row_lo, row_hi = d.row_hi;
    e->vrow.swap(h_vrow);
    e->h_rflag.assign(n_rows, RF_FIXED);
    for (int v = 0; v < M; ++v) e->h_rflag[e->vrow[v]] = RF_OBS | RF_REPROJ_ACTIVE;
    if (row_hi - row_lo < n_rows) {                                  // (a row-limited rank: the residual taps stage the observations of every row from here)
        e->h_uv.assign(2 * (size_t)n_rows, 0.f);
        for (int v = 0; v < M; ++v) { e->h_uv[2 * (size_t)e->vrow[v]] = s.uv[2 * (size_t)v]; e->h_uv[2 * (size_t)e->vrow[v] + 1] = s.uv[2 * (size_t)v + 1]; }
    }
    e->h_pose_fixed.assign(K, 0);
    e->dev_edges = true;                                             // residual taps copy the raw edges from the pack scratch (device to device)
    e->raw_sp = r_sp; e->raw_d0 = r_d0; e->raw_dm = r_dm; e->raw_w = r_w;
    e->serial = ++c->engine_serial;
    NRS_TRY(pin_host_words(c, e));
    if (e->n_spec > 0) NRS_TRY(spec_prepare(c, e));
    NRS_HIP(c, hipStreamSynchronize(st));                            // (the overflow word of pass 1 is final)
    int h_fl2[2] = {0, 0};
    NRS_HIP(c, hipMemcpy(h_fl2, d_flag, sizeof(int) * 2, hipMemcpyDeviceToHost));
    if (h_fl2[0]) return c->fail(NRS_ERR_HIP, "device pack: halo hash overflow in the second pass");
    d.tp_ok = h_fl2[1] ? 0 : 1;
    if (c->pack_ws2.cap > ((size_t)512 << 20)) c->pack_ws2.reset();      // intermediates of a large window: not worth keeping resident
    mark("final arrays");
    engine_compact_headers(c, e);
    NRS_TRY(engine_reset(c, e));
    return NRS_OK;
}

}  // namespace nrs
