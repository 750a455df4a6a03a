// What the two problem constructions decide alike, stated once: row groups, lanes per row, tile classes, LDS and path flags, the shard
// window, the arena, and the small arrays both finish with.  The host packer (nrs_engine_setup.hpp, engine_create) and the device packer
// (nrs_engine_devpack.hpp, DeviceBuild) call these, so the two give the same bits by construction.
// Part of nrs_engine.hip (one translation unit); see that file's header for the design.
#pragma once

namespace nrs {

// ---- row layout: pose-major, each pose padded to ROW_ALIGN rows
struct RowGroups {
    std::vector<int> pose_ptr, pose_grp_ptr, grp_pose;             // first vertex / first ROW_ALIGN group of a pose; the pose of a group
    int n_pad_rows = 0;
};
static RowGroups row_groups(const EngineSpec& s) {
    RowGroups g;
    g.pose_ptr.assign(s.K + 1, 0); g.pose_grp_ptr.assign(s.K + 1, 0);
    for (int i = 0; i < s.M; ++i) g.pose_ptr[s.lm_pose[i] + 1]++;
    for (int k = 0; k < s.K; ++k) g.pose_ptr[k + 1] += g.pose_ptr[k];
    for (int k = 0; k < s.K; ++k) {
        const int ng = std::max(1, (g.pose_ptr[k + 1] - g.pose_ptr[k] + ROW_ALIGN - 1) / ROW_ALIGN);
        g.pose_grp_ptr[k + 1] = g.pose_grp_ptr[k] + ng;
        g.grp_pose.insert(g.grp_pose.end(), ng, k);
    }
    g.n_pad_rows = g.pose_grp_ptr[s.K] * ROW_ALIGN;
    return g;
}

// lanes per row: 2 measured best on C2 (92k rows), 8 on single-frame problems (4.5k rows), where
// the kernels are bound by per-lane latency chains rather than by traffic (profiles/README.md)
static int lanes_per_row(const nrs_ctx* c, int n_pad_rows) {
    const int v = c->dbg.int_of(SW_SELL_T);                       // (0 unless set)
    if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) return v;
    return n_pad_rows >= 32768 ? 2 : 8;
}

// a zeroed Dev with the problem's constants and sizes
static void dev_init(Dev& d, const EngineSpec& s, const RowGroups& g, int T) {
    memset(&d, 0, sizeof(d));
    d.T = T;
    d.K = s.K; d.M = s.M; d.n_sp = s.n_sp; d.n_dm = s.n_dm; d.n_un = s.n_un;
    d.cam = s.cam;
    d.info_reproj = s.info_reproj; d.delta_reproj = s.delta_reproj;
    d.info_pos = s.info_pos; d.delta_pos = s.delta_pos;
    d.info_spatial = s.info_spatial; d.delta_spatial = s.delta_spatial;
    d.k_spring = s.k_spring; d.spring_form = s.spring_form;
    d.n_groups = g.pose_grp_ptr[s.K];
    d.n_rows = d.n_groups * ROW_ALIGN;
    d.tile_rows = BLK / T;
    d.n_regblk = d.n_rows / d.tile_rows;
    d.n_vecblk = d.n_rows / BLK;
}

// ---- tile classes: if a few tiles have much larger halos than the rest they get their own launch (class 1) with their own LDS
// size, and the bulk (class 0) keeps its occupancy.  hs / halo_ns: halo rows / spring-part halo rows per tile.  Returns tile_list
// (class 0 then class 1, ascending inside a class) and sets max_halo, max_halo_s, n_tiles_cls, cap_h, cap_s.
static std::vector<int> tile_classes(const nrs_ctx* c, Dev& d, const std::vector<int>& hs, const std::vector<int>& halo_ns) {
    const int nb = d.n_regblk;
    for (int b = 0; b < nb; ++b) { d.max_halo = std::max(d.max_halo, hs[b]); d.max_halo_s = std::max(d.max_halo_s, halo_ns[b]); }
    std::vector<int> tile_list(nb), sorted = hs;
    std::sort(sorted.begin(), sorted.end());
    int cut = d.max_halo;
    if (nb >= 1024) {                                              // small problems are latency-bound: one launch
        // (the second launch has to fill the chip by itself: >= 4 workgroups per CU, or be needed
        // for the bulk to fit the LDS budget at all)
        const int p97 = sorted[(size_t)(0.97 * (nb - 1))];
        const bool fits = sizeof(double) * 3 * (size_t)(2 * d.tile_rows + d.max_halo + d.max_halo_s + 2) <= 48 * 1024;
        if (4 * d.max_halo > 5 * p97 && (nb - (int)(0.97 * nb) >= 1024 || !fits) && !c->dbg.is_set(SW_ONE_CLASS)) cut = p97;
    }
    if (c->dbg.is_set(SW_TILE_CUT_PCT)) cut = sorted[(size_t)(c->dbg.real_of(SW_TILE_CUT_PCT) / 100.0 * (nb - 1))];   // test switch: force a split at a percentile
    int n0 = 0;
    for (int b = 0; b < nb; ++b) if (hs[b] <= cut) tile_list[n0++] = b;
    d.n_tiles_cls[0] = n0; d.n_tiles_cls[1] = nb - n0;
    for (int b = 0; b < nb; ++b) if (hs[b] > cut) tile_list[n0++] = b;
    for (int b = 0; b < nb; ++b) {
        const int cls = hs[b] <= cut ? 0 : 1;
        d.cap_h[cls] = std::max(d.cap_h[cls], hs[b]);
        d.cap_s[cls] = std::max(d.cap_s[cls], halo_ns[b]);
    }
    return tile_list;
}

// ---- LDS staging or the gather fallback, and which solver path the problem takes
static void path_flags(const nrs_ctx* c, Dev& d, const EngineSpec& s) {
    size_t lds_need = 0;
    for (int cls = 0; cls < 2; ++cls) {
        if (!d.n_tiles_cls[cls]) continue;
        if (d.dform) {
            lds_need = std::max(lds_need, sizeof(double) * 9 * (size_t)(d.tile_rows + d.cap_h[cls] + 1));                                    // linearise: x, G^f, G^b
            lds_need = std::max(lds_need, sizeof(double) * 3 * (3 * (size_t)(d.tile_rows + d.cap_h[cls] + 1) + d.tile_rows + d.cap_s[cls] + 1));  // operator: u, G^f, G^b + positions
            continue;
        }
        lds_need = std::max(lds_need, sizeof(double) * 3 * (size_t)(d.tile_rows + d.cap_h[cls]) * (s.X0 ? 2 : 1));                          // linearise
        lds_need = std::max(lds_need, sizeof(double) * 3 * (size_t)(2 * d.tile_rows + d.cap_h[cls] + d.cap_s[cls] + 2));                    // operator: u + positions
    }
    d.use_lds = !(c->dbg.is_set(SW_NO_LDS) || s.force_gather || lds_need > 64 * 1024 - 512 || d.tile_rows + d.max_halo >= 65535);   // irregular graph / A-B switch
    if (!d.use_lds) d.dform = 0;
    d.lin_rb = d.use_lds ? ROW_ALIGN / d.tile_rows : 1;              // lineariser partials: per tile (LDS path) or per group
    // single-launch PCG iteration for problems that are bound by launch latency, not by traffic
    const int fused_max = c->dbg.int_of(SW_FUSED_MAX_ROWS);
    d.fused = (d.use_lds && d.n_rows < fused_max && !c->dbg.is_set(SW_NO_FUSED)) ? 1 : 0;
    if (s.sk_window() > 0) d.fused = 0;                            // embedded mode: the skinned observations' operator kernels sit between the two launches of an iteration
    d.hier = (d.n_regblk > 4096 || c->dbg.is_set(SW_HIER)) ? 1 : 0;
    // (a profiling context times full operator launches only: no convergence-detecting early exits)
    d.ecd = (d.use_lds && !d.fused && !c->opt.profile && !c->dbg.is_set(SW_NO_ECD)) ? 1 : 0;
    // two-level preconditioner: fused path, one pose, small enough coarse system
    d.co_n = 3 * d.n_groups + 6;
    // (worth its per-iteration cost on the pose + deformation problems; the lost-point stage, pose
    // fixed and few free rows, converges in a few dozen block-Jacobi iterations anyway)
    const bool pose_free = !(s.pose_fixed && s.pose_fixed[0]);
    const size_t fused_shm = sizeof(double) * (6 * (size_t)(d.tile_rows + d.max_halo) + 12 * (size_t)d.n_regblk + 16 * CO_MAX);
    // (and only from ~1.5k rows on: below, its per-iteration cost outweighs the iterations it saves -- 1013 points 31.3 ms with it,
    // 29.2 without; 2220 points 47.4 / 51.8; 4525 points 76.7 / 94.1, tools/small_frame_probe.py)
    const int co_min_tiles = c->dbg.int_of(SW_COARSE_MIN_TILES);
    d.coarse = (d.fused && s.K == 1 && pose_free && d.co_n <= CO_MAX && d.n_regblk <= BLK && d.n_regblk >= co_min_tiles && fused_shm <= 63 * 1024 &&
                !c->dbg.is_set(SW_NO_COARSE)) ? 1 : 0;
}

// Contiguous keyframe ranges for `world` ranks, balanced by padded rows, every rank at least one
// keyframe: kb[r] .. kb[r+1] are rank r's keyframes.  grp_ptr[k] = first ROW_ALIGN group of keyframe k.
void shard_plan(int K, const int* grp_ptr, int world, int* kb) {
    const int total = grp_ptr[K];
    kb[0] = 0;
    for (int r = 1; r < world; ++r) {
        const int64_t want = (int64_t)total * r / world;
        int k = kb[r - 1] + 1;                                     // at least one keyframe for rank r-1 ...
        while (k < K - (world - r) && grp_ptr[k] < want) ++k;      // ... and for every rank that follows
        // the boundary closest to the ideal split
        if (k - 1 > kb[r - 1] && want - grp_ptr[k - 1] < grp_ptr[k] - want) --k;
        kb[r] = k;
    }
    kb[world] = K;
}

// The rows whose incidence records this engine packs (and later stores).  Sharded: the rows of ITS keyframe range only.  Rows of other
// ranks keep empty lists: their tiles never run here, and what this rank's tiles read of them are vector rows (the boundary-keyframe
// exchange), not records.  Packing time and record memory scale with 1 / ranks.
static void pack_range(const nrs_ctx* c, const EngineSpec& s, const RowGroups& g, int& lo, int& hi) {
    lo = 0; hi = g.n_pad_rows;
    if (!(c->comm && s.shard && c->comm->world <= 8 && s.K >= c->comm->world) || c->dbg.is_set(SW_SHARD_PACK_ALL)) return;
    std::vector<int> kb(c->comm->world + 1);
    shard_plan(s.K, g.pose_grp_ptr.data(), c->comm->world, kb.data());
    lo = g.pose_grp_ptr[kb[c->comm->rank]] * ROW_ALIGN; hi = g.pose_grp_ptr[kb[c->comm->rank + 1]] * ROW_ALIGN;
}

// What the tiles reach outside themselves, per tile: the smallest and largest halo row (lo / hi: INT_MAX / -1 for a tile without
// halo rows), and the same widened by whatever else a launch of the tile reads (blo / bhi: the temporal partners of the
// temporal-difference form; otherwise the halo extents themselves).  Only a sharded window needs them.
struct TileReach { const int *lo, *hi, *blo, *bhi; };

// ---- shard window: the whole problem, or this rank's contiguous range of poses (balanced by rows)
static int shard_window(nrs_ctx* c, Dev& d, HaloPlan& h, const EngineSpec& s, const RowGroups& g, const std::vector<int>& tile_list, const TileReach& reach) {
    d.sh_on = 0; d.sh_rank = 0; d.sh_world = 1; d.sh_lead = 1;
    d.sh_k0 = 0; d.sh_nk = s.K; d.sh_g0 = 0; d.sh_ng = d.n_groups; d.sh_vb0 = 0; d.sh_nvb = d.n_vecblk;
    for (int cls = 0; cls < 2; ++cls) { d.sh_t0[cls] = 0; d.sh_nt[cls] = d.n_tiles_cls[cls]; }      // (boundary-tile fields: zero from dev_init)
    if (!(c->comm && s.shard)) return NRS_OK;
    const int W = c->comm->world, rk = c->comm->rank;
    const std::vector<int>& pgp = g.pose_grp_ptr;
    // (a rank packs its own keyframe range only, so the halo sizes -- and with them this decision -- are rank-local)
    if (!d.use_lds) return c->fail(NRS_ERR_INVALID, "sharded solve: the graph's halo does not fit the LDS-staged path");
    std::vector<int> kb(W + 1);
    shard_plan(s.K, pgp.data(), W, kb.data());
    d.sh_on = 1; d.sh_rank = rk; d.sh_world = W; d.sh_lead = rk == 0;
    d.sh_k0 = kb[rk]; d.sh_nk = kb[rk + 1] - kb[rk];
    d.sh_g0 = pgp[kb[rk]]; d.sh_ng = pgp[kb[rk + 1]] - d.sh_g0;
    d.sh_vb0 = d.sh_g0 * (ROW_ALIGN / BLK); d.sh_nvb = d.sh_ng * (ROW_ALIGN / BLK);
    if ((int64_t)d.sh_nvb * BLK < s.K) return c->fail(NRS_ERR_INVALID, "sharded solve: shard smaller than the pose count");
    const int tb0 = d.sh_g0 * (ROW_ALIGN / d.tile_rows), tb1 = (d.sh_g0 + d.sh_ng) * (ROW_ALIGN / d.tile_rows);
    for (int cls = 0; cls < 2; ++cls) {                           // tile_list is ascending inside a class
        const int* tl = tile_list.data() + (cls ? d.n_tiles_cls[0] : 0);
        const int n = d.n_tiles_cls[cls];
        const int a = (int)(std::lower_bound(tl, tl + n, tb0) - tl), b2 = (int)(std::lower_bound(tl, tl + n, tb1) - tl);
        d.sh_t0[cls] = a; d.sh_nt[cls] = b2 - a;
    }
    // everything the own tiles reference must be owned or lie in the keyframe next to the range
    const int r_lo = (kb[rk] > 0 ? pgp[kb[rk] - 1] : d.sh_g0) * ROW_ALIGN;
    const int r_hi = (kb[rk + 1] < s.K ? pgp[kb[rk + 1] + 1] : d.sh_g0 + d.sh_ng) * ROW_ALIGN;
    for (int b = tb0; b < tb1; ++b)
        if (reach.lo[b] < r_lo || reach.hi[b] >= r_hi)
            return c->fail(NRS_ERR_INVALID, "sharded solve: an edge of keyframe range [%d, %d) reaches beyond the adjacent keyframes", kb[rk], kb[rk + 1]);
    // ... so the rank holds the per-row arrays (state, vectors, diagonal blocks: ~410 bytes a row) of its own keyframes and of ONE ghost
    // keyframe either side only: its tiles' halos end there (just checked), the boundary exchange fills the ghosts, and no launch of
    // this rank touches a row beyond them (ArenaPlan::get_rows).  NRS_SHARD_FULL_VECTORS=1: every row, the round-1..4 form.
    if (W > 1 && !d.dform && !c->dbg.is_set(SW_SHARD_FULL_VECTORS)) { d.row_lo = r_lo; d.row_hi = r_hi; }
    // boundary tiles (they read rows of another rank) sit at the two ends of the rank's tile range:
    // they run after the interior tiles, once the neighbours' rows have arrived
    const int own_lo = d.sh_g0 * ROW_ALIGN, own_hi = (d.sh_g0 + d.sh_ng) * ROW_ALIGN;
    auto foreign = [&](int b) { return reach.blo[b] < own_lo || reach.bhi[b] >= own_hi; };
    for (int cls = 0; cls < 2; ++cls) {
        const int* tl = tile_list.data() + (cls ? d.n_tiles_cls[0] : 0) + d.sh_t0[cls];
        const int n = d.sh_nt[cls];
        int first = n, last = -1;                                  // first / last own tile of the class that is interior
        for (int i = 0; i < n; ++i) if (!foreign(tl[i])) { first = i; break; }
        for (int i = n - 1; i >= 0; --i) if (!foreign(tl[i])) { last = i; break; }
        bool clean = last >= first;                                // (dampers reach one keyframe: the middle is interior)
        for (int i = first; i <= last && clean; ++i) clean = !foreign(tl[i]);
        d.sh_front[cls] = clean ? first : n; d.sh_back[cls] = clean ? n - 1 - last : 0;          // (no interior run: every tile waits)
    }
    auto rows_of = [&](int k, size_t& off, size_t& n) { off = 3 * (size_t)pgp[k] * ROW_ALIGN; n = 3 * (size_t)(pgp[k + 1] - pgp[k]) * ROW_ALIGN; };
    if (rk > 0) { rows_of(kb[rk], h.lo_send, h.lo_send_n); rows_of(kb[rk] - 1, h.lo_recv, h.lo_recv_n); }
    if (rk < W - 1) { rows_of(kb[rk + 1] - 1, h.hi_send, h.hi_send_n); rows_of(kb[rk + 1], h.hi_recv, h.hi_recv_n); }
    d.fused = 0; d.coarse = 0; d.ecd = 0; d.hier = 1;             // always the two-kernel PCG, reductions over the ranks
    return NRS_OK;
}

// ---- device memory: one arena allocation, reused across calls when large enough
struct ArenaPlan {                   // two passes: size, then carve
    Arena* a;
    bool dry;
    size_t off = 0;
    size_t row_lo = 0, row_n = 0;    // the rows this engine holds of every per-row array (a rank of a sharded window: its keyframes and one ghost keyframe either side)
    template <class Tp> Tp* get(size_t n) {
        const size_t bytes = ((n * sizeof(Tp) + 255) / 256) * 256 + 256;
        Tp* p = dry ? nullptr : reinterpret_cast<Tp*>(a->mem.as<char>() + off);
        off += bytes;
        return p;
    }
    // a per-row array (per_row elements a row): storage for rows [row_lo, row_lo + row_n) only, addressed by the GLOBAL row index --
    // the pointer handed out is the storage's start minus row_lo rows, so every kernel and every exchange indexes as on one GPU and
    // nothing outside the held rows is ever touched (engine_create: the launches of a rank cover its own tiles, whose halos end one
    // keyframe away)
    template <class Tp> Tp* get_rows(size_t per_row) {
        Tp* p = get<Tp>(row_n * per_row);
        return dry ? nullptr : p - row_lo * per_row;
    }
};

static void carve(ArenaPlan& A, Dev& d, bool has_X0, size_t nnz_s, size_t nnz_d, size_t n_slices, size_t n_halo, Engine* e) {
    const size_t nr = (size_t)d.n_rows, K = (size_t)d.K;
    if (d.row_hi <= 0) { d.row_lo = 0; d.row_hi = d.n_rows; }     // (callers that never shard leave the range unset: every row)
    A.row_lo = (size_t)d.row_lo; A.row_n = (size_t)(d.row_hi - d.row_lo);
    d.grp_pose = A.get<int>(d.n_groups);
    d.pose_grp_ptr = A.get<int>(K + 1);
    d.rflag = A.get_rows<uint8_t>(1);
    d.pose_fixed = A.get<uint8_t>(K);
    d.uv = A.get_rows<float>(2);
    double* X0 = has_X0 ? A.get_rows<double>(3) : A.get<double>(1);
    d.X0 = has_X0 ? X0 : nullptr;
    d.ss_ptr = A.get<int>(n_slices + 1);
    d.sd_ptr = A.get<int>(n_slices + 1);
    d.halo_ptr = A.get<int>((size_t)d.n_regblk + 1);
    d.halo_rows = A.get<int>(n_halo);
    d.halo_ns = A.get<int>((size_t)d.n_regblk);
    d.tile_list = A.get<int>((size_t)d.n_regblk);
    d.s_om = A.get<uint32_t>(d.use_lds ? nnz_s : 1);
    d.s_qc = A.get<double>(d.use_lds ? nnz_s : 1);
    d.d_hdr = A.get<uint2>(d.use_lds && !d.dform ? nnz_d : 1);
    d.d_om = A.get<uint32_t>(d.use_lds && d.dform ? nnz_d : 1);
    d.nxt_row = A.get<int>(d.dform ? nr : 1); d.prv_row = A.get<int>(d.dform ? nr : 1);
    d.halo_nxt = A.get<int>(d.dform ? std::max<size_t>(1, n_halo) : 1); d.halo_prv = A.get<int>(d.dform ? std::max<size_t>(1, n_halo) : 1);
    const size_t us = d.use_lds ? 1 : nnz_s, ud = d.use_lds ? 1 : nnz_d;     // unpacked arrays: fallback path only
    d.s_other = A.get<int>(us); d.s_d0 = A.get<float>(nnz_s); d.s_meta = A.get<int>(us);
    d.d_o0 = A.get<int>(ud); d.d_o1 = A.get<int>(ud); d.d_o2 = A.get<int>(ud);
    d.d_w = A.get<float>(nnz_d); d.d_meta = A.get<int>(ud);
    for (int s = 0; s < 2; ++s) { d.pose[s] = A.get<Pose>(K); d.xl[s] = A.get_rows<double>(3); }
    d.pose_init = A.get<Pose>(K);
    d.xl_init = A.get_rows<double>(3);
    d.D = A.get_rows<double>(6);
    d.Hpl = A.get<double>(d.use_lds ? 1 : 18 * nr);
    d.rowrec = d.use_lds ? A.get_rows<RowRec>(1) : A.get<RowRec>(1);
    d.row_tp = d.plain ? A.get_rows<uint32_t>(1) : A.get<uint32_t>(1);
    d.row_cnt = d.plain ? A.get_rows<uint32_t>(1) : A.get<uint32_t>(1);
    d.d_h4 = A.get<uint32_t>(d.plain && d.use_lds && !d.fused ? nnz_d : 1);
    d.s_g = A.get<double>(3 * us);
    d.d_s = A.get<double>(nnz_d);
    d.Hpp = A.get<double>(21 * K);
    d.bp = A.get<double>(6 * K);
    d.bl = A.get_rows<double>(3);
    d.Dinv = A.get_rows<double>(6);
    d.Hppinv = A.get<double>(36 * K);
    double** pv[] = {&d.xp, &d.rp, &d.up, &d.pp, &d.sp, &d.wp};
    for (auto p : pv) *p = A.get<double>(6 * K);
    double** rvv[] = {&d.xv, &d.rv, &d.uv3, &d.pv, &d.sv, &d.wv};
    for (auto p : rvv) *p = A.get_rows<double>(3);
    d.rp2 = A.get<double>(6 * K); d.sp2 = A.get<double>(6 * K); d.up2 = A.get<double>(6 * K);
    d.rv2 = A.get<double>(d.fused ? 3 * nr : 1); d.sv2 = A.get<double>(d.fused ? 3 * nr : 1); d.wv2 = A.get<double>(d.fused ? 3 * nr : 1);
    d.part_spmv2 = A.get<double>(d.fused ? NPART * (size_t)d.n_regblk : 1);
    {
        const size_t nb = d.coarse ? (size_t)d.n_regblk : 1, nc = d.coarse ? (size_t)d.co_n : 1;
        d.co_ct = A.get<double>(nb * (d.coarse ? (size_t)d.n_groups : 1) * 6);
        d.co_cp = A.get<double>(nb * 18);
        d.co_tb = A.get<double>(nb * 4);
        d.co_bt = A.get<double>(nb * 6);
        d.co_bti = A.get<double>(nb * 6);
        d.part_ts = A.get<double>(nb * 9); d.part_ts2 = A.get<double>(nb * 9);
        d.co_c0 = A.get<double>(nc * nc); d.co_nn = A.get<double>(nc); d.co_bc = A.get<double>(nc);
        d.co_inv = A.get<double>(nc * nc); d.co_y0 = A.get<double>(nc);
    }
    d.tile_desc = A.get<int>(d.fused ? 8 * (size_t)d.n_regblk : 4);
    d.halo_fix = A.get<int>(d.fused ? BLK * (size_t)d.n_regblk : d.plain && d.use_lds ? HALO_FIX * (size_t)d.n_regblk : 4);
    d.red = A.get<double>(4 + 6 * K);
    d.red_loc = A.get<double>(4 + 6 * K);
    d.pk = A.get<double>(2 + 8 + 27 * K);
    d.pk_loc = A.get<double>(2 + 8 + 27 * K);
    d.part_ru = A.get<double>(d.ecd ? 2 * (size_t)d.n_vecblk : 1);
    d.part_lin = A.get<double>(32 * (size_t)d.n_groups * (size_t)d.lin_rb);
    d.part_rchi = A.get<double>((size_t)d.n_groups);
    d.part_pchi = A.get<double>(K);
    d.part_reg = A.get<double>(2 * (size_t)d.n_regblk);
    d.part_spmv = A.get<double>(NPART * (size_t)d.n_regblk);
    d.part_apply = A.get<double>((size_t)d.n_vecblk);
    d.scal = A.get<double>(SC_N);
    d.flags = A.get<int>(8);
    d.ec_sp = A.get<EcSpring>(d.ec_on ? std::max(1, d.ec_nsp) : 1);
    d.ec_dm = A.get<EcDamper>(d.ec_on ? std::max(1, d.ec_ndm) : 1);
    d.ec_w = A.get<float>(d.ec_on ? std::max(1, d.ec_ndm) : 1);
    d.part_ec = A.get<double>(d.ec_on ? std::max(1, d.ec_nblk) : 1);
    for (int j = 0; j < e->n_spec; ++j) {                          // shadow sets of what an LM trial writes (speculative trials: nrs_engine_types.hpp)
        SpecSet& q = e->spec[j];
        q.xv = A.get_rows<double>(3); q.xp = A.get<double>(6 * K);
        q.pose = A.get<Pose>(K); q.xl = A.get_rows<double>(3);
        q.part_apply = A.get<double>((size_t)d.n_vecblk); q.part_rchi = A.get<double>((size_t)d.n_groups); q.part_reg = A.get<double>(2 * (size_t)d.n_regblk);
        q.scal = A.get<double>(SC_N); q.flags = A.get<int>(8); q.abort = A.get<int>(1);
        // (the sets' abort words are consecutive, so that one fill discards the trials of every set, TrialBatch::join: they all live
        // in the first set's slot -- a slot is 256 bytes at the least -- and the later sets' slots stay unused: the arena's size is unchanged)
        static_assert(SPEC_MAX * sizeof(int) <= 256, "the abort words share one slot");
        q.abort = e->spec[0].abort + j;
        q.sk_part = q.sk_chi = nullptr;
        q.rv = q.uv3 = q.pv = q.sv = q.wv = q.Dinv = q.Hppinv = q.rp = q.rp2 = q.up = q.up2 = q.pp = q.sp = nullptr;
        q.part_spmv = q.part_ru = q.red = q.part_ec = nullptr;
        if (!e->spec_pcg) continue;
        double** rows[] = {&q.rv, &q.uv3, &q.pv, &q.sv, &q.wv};
        for (auto p : rows) *p = A.get_rows<double>(3);
        q.Dinv = A.get_rows<double>(6);
        q.Hppinv = A.get<double>(36 * K);
        double** poses[] = {&q.rp, &q.rp2, &q.up, &q.up2, &q.pp, &q.sp};
        for (auto p : poses) *p = A.get<double>(6 * K);
        q.part_spmv = A.get<double>(NPART * (size_t)d.n_regblk);
        q.part_ru = A.get<double>(d.ecd ? 2 * (size_t)d.n_vecblk : 1);
        q.red = A.get<double>(4 + 6 * K);
        q.part_ec = A.get<double>(d.ec_on ? std::max(1, d.ec_nblk) : 1);
    }
}

// Sizes the arena for this engine (a dry carve on a copy), grows it when it is too small, and carves it.  The caller has chosen the
// engine's shadow sets (e->n_spec, e->spec_pcg) before.
static int arena_fit(nrs_ctx* c, Arena* arena, Engine* e, Dev& d, bool has_X0, size_t nnz_s, size_t nnz_d, size_t n_slices, size_t n_halo) {
    ArenaPlan dry{arena, true};
    {
        Dev tmp = d;
        Engine te;
        te.n_spec = e->n_spec; te.spec_pcg = e->spec_pcg;
        carve(dry, tmp, has_X0, nnz_s, nnz_d, n_slices, n_halo, &te);
    }
    if (dry.off > arena->mem.cap) {
        NRS_HIP(c, hipStreamSynchronize(c->stream));
        const size_t want = dry.off + dry.off / 8;
        hipError_t he = c->alloc(arena->mem, want);                // (the old arena is freed first)
        if (he != hipSuccess) return c->fail(NRS_ERR_ALLOC, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(he));
        if (c->dbg.is_set(SW_POISON)) { (void)hipMemset(arena->mem.p, 0xFF, want); (void)hipDeviceSynchronize(); }    // (debug: a read of memory nobody wrote shows up as NaN)
    }
    ArenaPlan real{arena, false};
    carve(real, d, has_X0, nnz_s, nnz_d, n_slices, n_halo, e);
    e->arena_bytes = real.off;
    return NRS_OK;
}

// ---- what both constructions finish with
// the fused iteration's tile descriptors: {keyframe, its first tile, its end tile, first halo entry, halo entries, 0, 0, 0}
static std::vector<int> tile_desc_build(const Dev& d, const RowGroups& g, const std::vector<int>& halo_ptr) {
    std::vector<int> tile_desc(8 * (size_t)d.n_regblk, 0);
    const int rb = ROW_ALIGN / d.tile_rows;
    for (int b = 0; b < d.n_regblk; ++b) {
        const int kf = g.grp_pose[(size_t)b * d.tile_rows / ROW_ALIGN];
        int* td = &tile_desc[8 * (size_t)b];
        td[0] = kf; td[1] = g.pose_grp_ptr[kf] * rb; td[2] = g.pose_grp_ptr[kf + 1] * rb;
        td[3] = halo_ptr[b]; td[4] = halo_ptr[b + 1] - halo_ptr[b];
    }
    return tile_desc;
}

// partial slots, scalars and status words start at zero, and so do the factor streams' padding slots
static int zero_work_arrays(nrs_ctx* c, Dev& d) {
    if (d.use_lds) {
        NRS_HIP(c, hipMemsetAsync(d.s_qc, 0, sizeof(double) * (size_t)d.ss_nnz, c->stream));
        NRS_HIP(c, hipMemsetAsync(d.d_s, 0, sizeof(double) * (size_t)d.sd_nnz, c->stream));
    }
    NRS_HIP(c, hipMemsetAsync(d.part_apply, 0, sizeof(double) * (size_t)d.n_vecblk, c->stream));
    if (d.sh_on) {                                                // slots of other ranks' tiles are never written: zero for good
        NRS_HIP(c, hipMemsetAsync(d.part_lin, 0, sizeof(double) * 32 * (size_t)d.n_groups * (size_t)d.lin_rb, c->stream));
        NRS_HIP(c, hipMemsetAsync(d.part_rchi, 0, sizeof(double) * (size_t)d.n_groups, c->stream));
        NRS_HIP(c, hipMemsetAsync(d.part_reg, 0, sizeof(double) * 2 * (size_t)d.n_regblk, c->stream));
        NRS_HIP(c, hipMemsetAsync(d.part_spmv, 0, sizeof(double) * NPART * (size_t)d.n_regblk, c->stream));
        NRS_HIP(c, hipMemsetAsync(d.red, 0, sizeof(double) * (4 + 6 * (size_t)d.K), c->stream));
        NRS_HIP(c, hipMemsetAsync(d.red_loc, 0, sizeof(double) * (4 + 6 * (size_t)d.K), c->stream));
    }
    NRS_HIP(c, hipMemsetAsync(d.scal, 0, sizeof(double) * SC_N, c->stream));
    NRS_HIP(c, hipMemsetAsync(d.flags, 0, sizeof(int) * 8, c->stream));
    return NRS_OK;
}

// host words the kernels publish into (mapped: the same pointer on the device)
constexpr unsigned PIN_PUBLISHED = hipHostMallocMapped | hipHostMallocCoherent;

// the engine's scalar and status mirrors live in the context (reused by every engine)
static int pin_host_words(nrs_ctx* c, Engine* e) {
    NRS_HIP(c, c->ensure_pinned(c->pin_scal, sizeof(double) * SC_N, PIN_PUBLISHED));
    if (!c->pin_flags.p) {
        NRS_HIP(c, c->ensure_pinned(c->pin_flags, sizeof(int) * 8, PIN_PUBLISHED));
        memset(c->pin_flags.p, 0, sizeof(int) * 8);                // [7] is the publication sequence word the host polls
    }
    e->h_scal = e->d.h_scal = c->pin_scal.as<double>();
    e->h_flags = e->d.h_flags = c->pin_flags.as<int>();
    return NRS_OK;
}

}  // namespace nrs
