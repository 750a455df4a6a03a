// Host side of the engine: arena, row layout, sliced-ELL packing, halo lists, tile classes, uploads (engine_create and friends).
// Part of nrs_engine.hip (one translation unit); see that file's header for the design.
#pragma once
#include "nrs_devpack_host.hpp"     // the device packer's scratch plans, fall-back reasons and host decisions (DeviceBuild)

namespace nrs {

// =====================================================================================
// host side
// =====================================================================================
int engine_num_poses(const Engine* e) { return e->d.K; }
void engine_edge_counts(const Engine* e, int* n_sp, int* n_dm) { *n_sp = e->d.n_sp; *n_dm = e->d.n_dm; }

// the shadow sets' arrays as the engine's own start out (zero partials, scalars and status words), their host mirrors, and the
// context's streams and events for them (created on first use)
static int spec_prepare(nrs_ctx* c, Engine* e) {
    const Dev& d = e->d;
    if (!c->pin_spec_scal.p) {
        NRS_HIP(c, c->ensure_pinned(c->pin_spec_scal, sizeof(double) * SC_N * SPEC_MAX, PIN_PUBLISHED));
        NRS_HIP(c, c->ensure_pinned(c->pin_spec_flags, sizeof(int) * 8 * SPEC_MAX, PIN_PUBLISHED));
        memset(c->pin_spec_flags.p, 0, sizeof(int) * 8 * SPEC_MAX);
        // (measured and dropped: shadow streams at the lowest priority so that they yield to the context's stream -- a level of the
        // factorisation on such a stream takes 57 us instead of 28 even with the device to itself)
        for (int j = 0; j < SPEC_MAX; ++j) {
            NRS_HIP(c, stream_create(c->spec_stream[j]));
            NRS_HIP(c, event_create(c->spec_join[j]));
        }
        NRS_HIP(c, event_create(c->spec_fork));
        for (int j = 0; j < 1 + SPEC_MAX; ++j) NRS_HIP(c, event_create(c->spec_back[j]));
    }
    for (int j = 0; j < e->n_spec; ++j) {
        SpecSet& q = e->spec[j];
        q.h_scal = c->pin_spec_scal.as<double>() + SC_N * j; q.h_flags = c->pin_spec_flags.as<int>() + 8 * j;
        NRS_HIP(c, hipMemsetAsync(q.part_apply, 0, sizeof(double) * (size_t)d.n_vecblk, c->stream));
        NRS_HIP(c, hipMemsetAsync(q.part_rchi, 0, sizeof(double) * (size_t)d.n_groups, c->stream));
        NRS_HIP(c, hipMemsetAsync(q.part_reg, 0, sizeof(double) * 2 * (size_t)d.n_regblk, c->stream));
        NRS_HIP(c, hipMemsetAsync(q.scal, 0, sizeof(double) * SC_N, c->stream));
        NRS_HIP(c, hipMemsetAsync(q.flags, 0, sizeof(int) * 8, c->stream));
        NRS_HIP(c, hipMemsetAsync(q.abort, 0, sizeof(int), c->stream));
    }
    return NRS_OK;
}

// shadow sets of a single-frame engine (speculative LM trials, nrs_engine_types.hpp): NRS_SPEC_TRIALS=<0..3> (0: one trial at a time)
static int spec_sets(const nrs_ctx* c) {
    static_assert(SPEC_TRIALS_MAX == SPEC_MAX, "the clamp of NRS_SPEC_TRIALS is the number of shadow sets");
    if (c->opt.profile) return 0;                                  // (a profiling context times its launches one by one)
    // two shadow sets = three trials in flight: a fourth stream's launches are serialised behind another stream's on this runtime (its result
    // arrives a whole trial after the third's: 240 / 266 / 298 / 516 us at 1k points), so a third set only adds work that may be discarded
    return c->dbg.int_of(SW_SPEC_TRIALS);                          // (2 unless set)
}

// shadow sets of a BA window on the two-kernel PCG (speculative LM trials, nrs_engine_types.hpp): unsharded windows without skinned
// observations (no keyframe-block factorisation either: that needs them), not profiling, up to NRS_SPEC_MAX_ROWS rows (default 2^18).
// A set is 27 doubles a row (20 MB at C2's 92k rows).  Above the default the trials' launches fill the device on their own: C3 (455k
// rows) takes 17.5 ms per step with sets against 17.0 without, so larger windows carve none.
static void spec_pcg_sets(const nrs_ctx* c, Engine* e, int n_skin) {
    const Dev& d = e->d;
    const long max_rows = c->dbg.long_of(SW_SPEC_MAX_ROWS);
    const bool on = !e->nd && !d.fused && !d.coarse && !d.sh_on && n_skin == 0 && !c->opt.profile && (long)d.n_rows <= max_rows;
    e->spec_pcg = on;
    e->n_spec = on ? spec_sets(c) : 0;
}

template <class Tp>
static int h2d(nrs_ctx* c, Tp* dst, const std::vector<Tp>& src) {
    if (!src.empty()) NRS_HIP(c, hipMemcpyAsync(dst, src.data(), sizeof(Tp) * src.size(), hipMemcpyHostToDevice, c->stream));
    return NRS_OK;
}

// a full-length host image of a per-row array (per_row elements a row) into the rows this engine holds of it
template <class Tp>
static int h2d_rows(nrs_ctx* c, const Dev& d, Tp* dst, const std::vector<Tp>& src, size_t per_row) {
    const size_t o = (size_t)d.row_lo * per_row, n = (size_t)(d.row_hi - d.row_lo) * per_row;
    if (n) NRS_HIP(c, hipMemcpyAsync(dst + o, src.data() + o, sizeof(Tp) * n, hipMemcpyHostToDevice, c->stream));
    return NRS_OK;
}

// Host-side set-up work split over a few threads.  Every use below is order-free (disjoint outputs, or integer counts) or
// reproduces the sequential order (a thread owns a range of ROWS and scans the edges in edge order): the packed problem is
// the same bits for any thread count (tests/test_gpu_scale.py).
static int host_threads(const nrs_ctx* c, size_t work) {
    if (work < 600000) {
        // single-frame problems (a 4.5k-point frame: 0.3 M incidences): sixteen threads per stage cost more than they save (8 ms per frame,
        // round 2); NRS_HOST_THREADS_SMALL=<n> tries a few (round 5: see profiles/README.md)
        if (c->dbg.is_set(SW_HOST_THREADS_SMALL) && work >= 100000) return std::max(1, std::min(8, c->dbg.int_of(SW_HOST_THREADS_SMALL)));
        return 1;
    }
    int n = (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (c->dbg.is_set(SW_HOST_THREADS)) n = c->dbg.int_of(SW_HOST_THREADS);
    return n;
}
// plain two-kernel windows whose rows all know their temporal partners: the dampers' 8-byte headers {o0, o1, o2, meta} shrink
// to 4 bytes {o0 : 12, o2 : 12, meta : 8} -- o1 is the row's own partner (row_tp) and tile-local ids stay below 4096.  Derived
// on the device from d_hdr, whichever packer built that.
__global__ void k_compact_headers(size_t n, const uint2* __restrict__ hdr, uint32_t* __restrict__ h4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint2 h = hdr[i];
    const uint32_t m16 = h.y >> 16;
    h4[i] = m16 == REC_NONE ? 0xFFFFFFFFu : ((h.x & 0xFFFu) | ((h.y & 0xFFFu) << 12) | ((m16 & 0xFFu) << 24));
}
static void engine_compact_headers(nrs_ctx* c, Engine* e) {
    Dev& d = e->d;
    d.h4 = 0; d.rc = 0; d.nt = 0;
    if (!(d.plain && d.tp_ok && d.use_lds && !d.fused && d.T == 2) || c->dbg.is_set(SW_NO_H4)) return;
    if (d.tile_rows + std::max(d.cap_h[0], d.cap_h[1]) + 2 >= 4096 || d.sd_nnz <= 0) return;
    hipLaunchKernelGGL(k_compact_headers, dim3((unsigned)(((size_t)d.sd_nnz + 255) / 256)), dim3(256), 0, c->stream, (size_t)d.sd_nnz, d.d_hdr, d.d_h4);
    d.h4 = 1;
    d.rc = c->dbg.int_of(SW_RC);
    d.nt = 12 * ((size_t)d.ss_nnz + (size_t)d.sd_nnz) > ((size_t)128 << 20);   // the streams (with the vectors next to them) do not stay in the 256 MB Infinity Cache between launches
    if (c->dbg.is_set(SW_NT)) d.nt = c->dbg.int_of(SW_NT) != 0;
}

template <class F>
static void parallel_for(int nt, F&& fn) {                         // fn(thread index, thread count)
    if (nt <= 1) { fn(0, 1); return; }
    std::vector<std::thread> th;
    th.reserve(nt - 1);
    for (int t = 1; t < nt; ++t) {
        try { th.emplace_back([&fn, t, nt] { fn(t, nt); }); }
        catch (const std::system_error&) { fn(t, nt); }            // no thread to be had: this share runs here
    }
    fn(0, nt);
    for (auto& x : th) x.join();
}
static inline void chunk(int64_t n, int t, int nt, int64_t& a, int64_t& b) { a = n * t / nt; b = n * (t + 1) / nt; }
// count into a shared array: a plain increment when the stage runs on one thread (a locked add costs ~2 ns even uncontended:
// 2.5 ms per tracked frame over its two engines)
static inline void count_up(int* p, int nt) { if (nt == 1) ++*p; else __atomic_fetch_add(p, 1, __ATOMIC_RELAXED); }

// per-edge masks -> per-incidence meta words and per-row flags (host), then upload
static int push_masks(nrs_ctx* c, Engine* e, const uint8_t* sp_active, const uint8_t* dm_active) {
    Dev& d = e->d;
    auto vfixed = [&](int v) { return (e->h_rflag[e->vrow[v]] & RF_FIXED) != 0; };
    const int nt = host_threads(c, (size_t)d.n_sp + (size_t)d.n_dm);
    parallel_for(nt, [&](int ti, int n_thr) {                     // every edge writes its own incidence slots
    int64_t q0, q1;
    chunk(d.n_sp, ti, n_thr, q0, q1);
    for (int s = (int)q0; s < (int)q1; ++s) {
        const int i = e->sp_ij[2 * s], j = e->sp_ij[2 * s + 1];
        const bool act = (!sp_active || sp_active[s]) && !(vfixed(i) && vfixed(j));
        const int m = act ? SM_ACTIVE : 0;
        if (e->sp_pos[2 * s] >= 0) e->h_s_meta[e->sp_pos[2 * s]] = m | (act ? SM_COUNT : 0);      // (-1: the row belongs to another rank)
        if (e->sp_pos[2 * s + 1] >= 0) e->h_s_meta[e->sp_pos[2 * s + 1]] = m;
    }
    chunk(d.n_dm, ti, n_thr, q0, q1);
    for (int s = (int)q0; s < (int)q1; ++s) {
        bool allfix = true;
        int first = -1;
        for (int r = 0; r < 4; ++r) {
            const int v = e->dm_idx[4 * s + r];
            if (v >= 0) { if (first < 0) first = r; allfix = allfix && vfixed(v); }
        }
        const bool act = (!dm_active || dm_active[s]) && !allfix;
        for (int r = 0; r < 4; ++r) {
            const int p = e->dm_pos[4 * s + r];
            if (p < 0) continue;
            e->h_d_meta[p] = r | (act ? DM_ACTIVE : 0) | ((act && r == first) ? DM_COUNT : 0);
        }
    }
    chunk(d.n_un, ti, n_thr, q0, q1);
    for (int s = (int)q0; s < (int)q1; ++s) {
        const bool act = !vfixed(e->un_ij[2 * s]);
        if (e->un_pos[s] >= 0) e->h_d_meta[e->un_pos[s]] = 2 | DM_UNARY | (act ? (DM_ACTIVE | DM_COUNT) : 0);
    }
    });
    if (d.use_lds) {
        // the meta half-words of the static header streams (the factor streams are not touched)
        parallel_for(nt, [&](int ti, int n_thr) {
            int64_t a, b;
            chunk((int64_t)e->h_s_om.size(), ti, n_thr, a, b);
            for (int64_t i = a; i < b; ++i) {
                const int m = e->h_s_meta[i];
                const uint32_t m16 = (uint32_t)(((m & SM_ACTIVE) ? SR_ACTIVE : 0) | ((m & SM_COUNT) ? SR_COUNT : 0));
                e->h_s_om[i] = (e->h_s_om[i] & 0xFFFFu) | (m16 << 16);
            }
            chunk((int64_t)e->h_d_hdr.size(), ti, n_thr, a, b);
            for (int64_t i = a; i < b; ++i) {
                const uint32_t m16 = e->h_d_meta[i] < 0 ? (uint32_t)REC_NONE : (uint32_t)(e->h_d_meta[i] & 0xFFFF);
                e->h_d_hdr[i].y = (e->h_d_hdr[i].y & 0xFFFFu) | (m16 << 16);
            }
        });
        for (size_t i = 0; i < e->h_d_om.size(); ++i) {
            const uint32_t m16 = e->h_d_meta[i] < 0 ? (uint32_t)REC_NONE : (uint32_t)(e->h_d_meta[i] & 0xFFFF);
            e->h_d_om[i] = (e->h_d_om[i] & 0xFFFFu) | (m16 << 16);
        }
        NRS_TRY(h2d(c, d.s_om, e->h_s_om));
        if (d.dform) NRS_TRY(h2d(c, d.d_om, e->h_d_om));
        else NRS_TRY(h2d(c, d.d_hdr, e->h_d_hdr));
    } else {
        NRS_TRY(h2d(c, d.s_meta, e->h_s_meta));
        NRS_TRY(h2d(c, d.d_meta, e->h_d_meta));
    }
    NRS_TRY(h2d_rows(c, d, d.rflag, e->h_rflag, 1));
    NRS_TRY(h2d(c, d.pose_fixed, e->h_pose_fixed));
    return NRS_OK;
}

// ---- engine_create: the host construction, stage by stage
// argument checks on inputs every rank of a sharded upload holds alike
static int spec_validate(nrs_ctx* c, const EngineSpec& s) {
    if (s.K <= 0 || s.M <= 0 || !s.poses || !s.x || !s.lm_pose || !s.uv || !s.rflag || s.n_sp < 0 || s.n_dm < 0 || s.n_un < 0)
        return c->fail(NRS_ERR_INVALID, "engine: bad specification");
    for (int i = 0; i < s.M; ++i)
        if (s.lm_pose[i] < 0 || s.lm_pose[i] >= s.K || (i > 0 && s.lm_pose[i] < s.lm_pose[i - 1]))
            return c->fail(NRS_ERR_INVALID, "vertex pose index must be non-decreasing and in [0, n_poses)");
    if (!s.edges_on_device) {                                      // (device-built edge lists are valid by construction)
        for (int64_t i = 0; i < 2 * (int64_t)s.n_sp; ++i)
            if (s.sp_ij[i] < 0 || s.sp_ij[i] >= s.M) return c->fail(NRS_ERR_INVALID, "spring index out of range");
        for (int64_t i = 0; i < 4 * (int64_t)s.n_dm; ++i)
            if (s.dm_idx[i] < -1 || s.dm_idx[i] >= s.M) return c->fail(NRS_ERR_INVALID, "damper index out of range");
    }
    for (int64_t i = 0; i < 2 * (int64_t)s.n_un; ++i)
        if (s.un_ij[i] < 0 || s.un_ij[i] >= s.M) return c->fail(NRS_ERR_INVALID, "unary damper index out of range");
    if (c->comm && s.shard) {                                      // the same on every rank: no collective follows these returns
        if (c->comm->world > 8) return c->fail(NRS_ERR_INVALID, "sharded solve: at most 8 ranks");
        if (s.K < c->comm->world) return c->fail(NRS_ERR_INVALID, "sharded solve: %d keyframes cannot be split over %d ranks", s.K, c->comm->world);
    }
    return NRS_OK;
}

// a2's single-frame engines: the direct solver's symbolic phase needs the structure only and runs next to the packing (on the context's
// plan worker, which keeps references to nd_in and nd_prep: both live in engine_create's frame)
static int nd_plan_start(nrs_ctx* c, const EngineSpec& s, Engine* e, NdIn& nd_in, NdPrep& nd_prep) {
    e->nd = new (std::nothrow) NdEngine();
    if (!e->nd) return c->fail(NRS_ERR_ALLOC, "out of host memory");
    e->n_spec = spec_sets(c);                                  // shadow sets for speculative LM trials (carved with the arena below)
    e->nd->pos.resize(3 * (size_t)s.M);
    for (size_t i = 0; i < 3 * (size_t)s.M; ++i) e->nd->pos[i] = s.x[i] + (s.X0 ? s.X0[i] : 0.0);
    nd_in.M = s.M; nd_in.rflag = s.rflag; nd_in.pose_fixed = s.pose_fixed && s.pose_fixed[0];
    nd_in.n_sp = s.n_sp; nd_in.sp_ij = s.sp_ij; nd_in.n_dm = s.n_dm; nd_in.dm_idx = s.dm_idx;
    nd_in.n_skin = s.n_skin; nd_in.sk_vert = s.sk_node; nd_in.sk_om = s.sk_om;
    nd_in.vpos = e->nd->pos.data();
    bool inline_run = c->dbg.is_set(SW_HOST_THREADS) && c->dbg.int_of(SW_HOST_THREADS) <= 1;
    if (!inline_run) {
        PlanWorker* pw = c->plan_worker;
        if (!pw) {
            pw = new (std::nothrow) PlanWorker();
            if (pw && !pw->start()) { delete pw; pw = nullptr; }
            c->plan_worker = pw;
        }
        if (pw) { nd_prep.worker = pw; pw->submit([c, &nd_in, &nd_prep] { nd_prep_run(c, nd_in, nd_prep); }); }
        else inline_run = true;
    }
    if (inline_run) nd_prep_run(c, nd_in, nd_prep);
    return NRS_OK;
}

// The host packer's state: what one stage leaves for the next, and the staging vectors of the uploads, which must outlive the
// stream synchronise that follows them in engine_create -- so they live here, not in the stage that fills them.
struct HostBuild {
    nrs_ctx* c; const EngineSpec& s; Engine* e; Dev& d; const RowGroups& g; int T;
    StageTimer mark{c, "engine_create", false};
    int nt_all = host_threads(c, 2 * (size_t)s.n_sp + 4 * (size_t)s.n_dm + (size_t)s.n_un);   // one decision for every set-up stage
    int Rw = 0, n_slices = 0, pack_lo = 0, pack_hi = 0;
    size_t nnz_s = 0, nnz_d = 0;
    std::vector<int> sp_row, dm_row, un_row, cnt_s, cnt_d, ss_ptr, sd_ptr;      // the row of every incidence; per row counts; slice offsets
    std::vector<int> S_other, D_o, D_role, nxt_row, prv_row, L_s, L_d;          // sliced-ELL neighbours: global rows, temporal partners, tile-local ids
    std::vector<float> S_d0, D_w;
    std::vector<int> halo_ptr, halo_rows, halo_ns, tile_list;
    std::vector<uint32_t> row_tp;
    std::vector<EcSpring> ec_sp; std::vector<EcDamper> ec_dm; std::vector<float> ec_w;
    std::vector<float> uv; std::vector<double> xl, X0; std::vector<Pose> poses;      // upload staging only
    std::vector<int> d_o0, d_o1, d_o2, tile_desc, halo_fix;
    // packed position of the k-th incidence of a row
    size_t pos_of(const std::vector<int>& ptr, int row, int k) const {
        const int sl = row / Rw, r = row - sl * Rw;
        return (size_t)ptr[sl] + (size_t)(k / T) * 64 + (size_t)r * T + (size_t)(k % T);
    }
    void row_layout();
    void incidence_rows();
    void sell_pack();
    void temporal_form();
    void halo_lists();
    int decide();
    void ec_lists_build();
    void edge_lists();
    void host_mirrors();
    int uploads();
};

// What a device build holds of the window: the incidences (own_s, own_d) and counted edges (ec_*) of the rows it packs and the sliced-ELL
// sizes.  rank: the share is a rank's of a sharded window -- tiles of other ranks exist and keep empty lists, the shard fields want every
// own tile's smallest / largest halo row, and the keys of the counted edges were sorted with the incidence keys (incidences_own)
struct DpShare { int64_t own_s, own_d; int ec_nsp, ec_ndm; size_t nnz_s, nnz_d; bool rank; };
// The device packer's state (the stages: nrs_engine_devpack.hpp; scratch plans and host decisions: nrs_devpack_host.hpp): what one stage
// leaves for the next -- the two scratch buffers as typed pointers, the share, the host copies the decisions read, upload staging.
// A stage that finds the window does not qualify after all says so in `why`; engine_create then runs the host packer from scratch.
struct DeviceBuild {
    nrs_ctx* c; const EngineSpec& s; Engine* e; Dev& d; const RowGroups& g; Arena* arena; int T;
    StageTimer mark{c, "device pack", true};
    hipStream_t st = c->stream;
    const bool sh = c->comm != nullptr && s.shard;                 // a rank of a sharded window packs the incidence records of its own keyframe range only
    const int K = s.K, M = s.M, n_sp = s.n_sp, n_dm = s.n_dm;
    const int64_t ni_s = 2 * (int64_t)n_sp, ni_d = 4 * (int64_t)n_dm;
    DpReason why = DP_BUILT;
    int n_rows = 0, n_slices = 0, n_tiles = 0, pack_lo = 0, pack_hi = 0, tb0 = 0, tb1 = 0, row_bits = 0;   // [tb0, tb1): the tiles of [pack_lo, pack_hi)
    size_t tmp_bytes = 0, tmp2_bytes = 0, n_halo = 0;
    // scratch 1 (bound in uploads): raw inputs + intermediates sized from the inputs
    double *r_x, *mm; float *r_uv, *r_d0, *r_w; uint64_t *code_a, *code_b; uint32_t *tk_a, *tk_b; void* tmp;
    int *r_kf, *r_sp, *r_dm, *val_a, *val_b, *cs, *cd, *d_pose_ptr, *d_pgp, *tile_off, *vrow, *row_v, *tv_a, *tv_b, *cnt_s, *cnt_d, *rs_s, *rs_d, *ws, *wd, *d_ss, *d_sd,
        *hs, *hns, *hmin, *hmax, *d_flag;
    // scratch 2 (bound in scratch2): sized from the share; the incidence keys live in scratch 1 on one GPU, here on a rank
    int *S_other, *D_o; uint8_t* S_side; int8_t* D_role; float *t_d0, *t_w; uint64_t *ek_s, *ek_s2, *ek_d, *ek_d2, *key_s, *key_s2, *key_d, *key_d2; void* tmp2 = nullptr;
    DpShare sr{};
    int h_nnz[2] = {0, 0}, h_own[4] = {0, 0, 0, 0}, h_flag = 0;     // download targets: they outlive the stage's synchronise
    std::vector<int> h_hs, h_hns, h_vrow, h_hmin, h_hmax, halo_ptr, tile_list;
    std::vector<Pose> poses;                                        // upload staging: alive until host_side's synchronise
    static dim3 nb(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }
    bool precheck();
    int uploads();
    int row_layout();
    int slice_offsets();
    int scratch2();
    int incidences_whole();
    int incidences_own();
    int incidences();
    int fill_and_halo_sizes();
    int decide();
    int final_arrays();
    int host_side();
};

// ---- row layout: pose-major, each pose padded to ROW_ALIGN rows (row_groups), Morton order inside
void HostBuild::row_layout() {
    e->vrow.resize(s.M);
    {
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
        auto pos = [&](int v, int a) { return s.x[3 * (size_t)v + a] + (s.X0 ? s.X0[3 * (size_t)v + a] : 0.0); };
        for (int v = 0; v < s.M; ++v)
            for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], pos(v, a)); hi[a] = std::max(hi[a], pos(v, a)); }
        auto spread = [](uint64_t v) {            // 21 bits -> every third bit
            v &= 0x1fffff;
            v = (v | v << 32) & 0x1f00000000ffffULL;
            v = (v | v << 16) & 0x1f0000ff0000ffULL;
            v = (v | v << 8) & 0x100f00f00f00f00fULL;
            v = (v | v << 4) & 0x10c30c30c30c30c3ULL;
            v = (v | v << 2) & 0x1249249249249249ULL;
            return v;
        };
        const bool morton = !c->dbg.is_set(SW_NO_MORTON);
        parallel_for(std::min(nt_all, s.K), [&](int ti, int nt) {
        std::vector<std::pair<uint64_t, int>> keys;
        int64_t k0, k1;
        chunk(s.K, ti, nt, k0, k1);
        for (int k = (int)k0; k < (int)k1; ++k) {
            keys.clear();
            for (int v = g.pose_ptr[k]; v < g.pose_ptr[k + 1]; ++v) {
                uint64_t code = 0;
                if (morton)
                    for (int a = 0; a < 3; ++a) {
                        const double ext = hi[a] - lo[a];
                        const double f = ext > 0 ? (pos(v, a) - lo[a]) / ext : 0.0;
                        code |= spread((uint64_t)(f * 2097151.0)) << a;
                    }
                keys.emplace_back(code, v);
            }
            std::stable_sort(keys.begin(), keys.end());
            for (size_t i = 0; i < keys.size(); ++i) e->vrow[keys[i].second] = g.pose_grp_ptr[k] * ROW_ALIGN + (int)i;
        }
        });
    }
    // Inside a tile the row order is free (neighbour ids are tile-local, the vector kernels stream): rows are sorted
    // by their incidence counts, so that the rows of a slice (64 / T consecutive rows share the slice's width) have
    // similar counts.  C2: sliced-ELL padding 1.34x / 1.37x (springs / dampers) -> 1.22x / 1.15x of the incidences.
    if (!c->dbg.is_set(SW_NO_TILE_SORT)) {
        std::vector<int> cs(s.M, 0), cd(s.M, 0);
        parallel_for(nt_all, [&](int ti, int n) {                  // integer counts: order-free
            int64_t a, b;
            chunk(2 * (int64_t)s.n_sp, ti, n, a, b);
            for (int64_t q = a; q < b; ++q) count_up(&cs[s.sp_ij[q]], n);
            chunk(4 * (int64_t)s.n_dm, ti, n, a, b);
            for (int64_t q = a; q < b; ++q)
                if (s.dm_idx[q] >= 0) count_up(&cd[s.dm_idx[q]], n);
            chunk(s.n_un, ti, n, a, b);
            for (int64_t q = a; q < b; ++q) count_up(&cd[s.un_ij[2 * q]], n);
        });
        const int tile = BLK / T;
        std::vector<int> row_v((size_t)d.n_rows, -1);
        for (int v = 0; v < s.M; ++v) row_v[e->vrow[v]] = v;
        parallel_for(nt_all, [&](int ti, int n) {                  // tiles are independent
            std::vector<int> seg;
            int64_t t0, t1;
            chunk(d.n_rows / tile, ti, n, t0, t1);
            for (int64_t tl = t0; tl < t1; ++tl) {
                const int r0 = (int)tl * tile;
                seg.clear();
                for (int r = r0; r < r0 + tile; ++r) if (row_v[r] >= 0) seg.push_back(row_v[r]);
                std::stable_sort(seg.begin(), seg.end(), [&](int a, int b2) { return cd[a] != cd[b2] ? cd[a] > cd[b2] : cs[a] > cs[b2]; });
                for (size_t i = 0; i < seg.size(); ++i) e->vrow[seg[i]] = r0 + (int)i;
            }
        });
    }
    mark("row layout");
}

void HostBuild::incidence_rows() {
    // ---- incidence lists -> sliced ELL, built with two counting passes (no per-row containers)
    Rw = 64 / T;
    n_slices = d.n_rows / Rw;
    e->sp_pos.assign(2 * (size_t)s.n_sp, -1);
    e->dm_pos.assign(4 * (size_t)s.n_dm, -1);
    e->un_pos.assign((size_t)s.n_un, -1);
    pack_range(c, s, g, pack_lo, pack_hi);
    auto mine = [&](int row) { return row >= pack_lo && row < pack_hi; };
    e->pack_rows = pack_hi - pack_lo;
    // the row of every incidence, once (the passes below scan these flat arrays instead of chasing vrow)
    sp_row.resize(2 * (size_t)s.n_sp); dm_row.resize(4 * (size_t)s.n_dm); un_row.resize((size_t)s.n_un);
    cnt_s.assign(d.n_rows, 0); cnt_d.assign(d.n_rows, 0);
    parallel_for(nt_all, [&](int ti, int n) {
        int64_t a, b;
        chunk(2 * (int64_t)s.n_sp, ti, n, a, b);
        for (int64_t q = a; q < b; ++q) {
            const int r = e->vrow[s.sp_ij[q]];
            sp_row[q] = r;
            if (mine(r)) count_up(&cnt_s[r], n);
        }
        chunk(4 * (int64_t)s.n_dm, ti, n, a, b);
        for (int64_t q = a; q < b; ++q) {
            const int r = s.dm_idx[q] >= 0 ? e->vrow[s.dm_idx[q]] : -1;
            dm_row[q] = r;
            if (r >= 0 && mine(r)) count_up(&cnt_d[r], n);
        }
        chunk(s.n_un, ti, n, a, b);
        for (int64_t q = a; q < b; ++q) {
            const int r = e->vrow[s.un_ij[2 * q]];
            un_row[q] = r;
            if (mine(r)) count_up(&cnt_d[r], n);
        }
    });
    mark("incidence rows");
}

void HostBuild::sell_pack() {
    ss_ptr.assign(n_slices + 1, 0); sd_ptr.assign(n_slices + 1, 0);
    for (int sl = 0; sl < n_slices; ++sl) {
        int ws = 0, wd = 0;
        for (int r = 0; r < Rw; ++r) {
            ws = std::max(ws, (cnt_s[sl * Rw + r] + T - 1) / T);
            wd = std::max(wd, (cnt_d[sl * Rw + r] + T - 1) / T);
        }
        ss_ptr[sl + 1] = ss_ptr[sl] + ws * 64;
        sd_ptr[sl + 1] = sd_ptr[sl] + wd * 64;
    }
    nnz_s = (size_t)ss_ptr[n_slices]; nnz_d = (size_t)sd_ptr[n_slices];
    d.ss_nnz = (int)nnz_s;
    d.sd_nnz = (int)nnz_d;
    S_other.assign(nnz_s, -1); D_o.assign(3 * nnz_d, -1); D_role.assign(nnz_d, -1);
    S_d0.assign(nnz_s, 0.f); D_w.assign(nnz_d, 0.f);
    std::fill(cnt_s.begin(), cnt_s.end(), 0);
    std::fill(cnt_d.begin(), cnt_d.end(), 0);
    mark("sell arrays");
    // fill: a thread owns a contiguous range of rows (balanced by slots) and scans ALL incidences in edge order, taking the
    // ones of its rows -- the k-th incidence of a row is the k-th in edge order, as in a sequential pass
    std::vector<int> row_cut(nt_all + 1, pack_hi);
    row_cut[0] = pack_lo;
    {
        const int sl_lo = pack_lo / Rw, sl_hi = pack_hi / Rw;
        const int64_t tot = ((int64_t)ss_ptr[sl_hi] - ss_ptr[sl_lo]) + ((int64_t)sd_ptr[sl_hi] - sd_ptr[sl_lo]);
        int sl = sl_lo;
        for (int t = 1; t < nt_all; ++t) {
            const int64_t want = tot * t / nt_all;
            while (sl < sl_hi && ((int64_t)ss_ptr[sl] - ss_ptr[sl_lo]) + ((int64_t)sd_ptr[sl] - sd_ptr[sl_lo]) < want) ++sl;
            row_cut[t] = sl * Rw;
        }
    }
    parallel_for(nt_all, [&](int ti, int) {
        const int lo = row_cut[ti], hi = row_cut[ti + 1];
        if (lo >= hi) return;
        auto own = [&](int r) { return r >= lo && r < hi; };
        for (int q = 0; q < s.n_sp; ++q) {
            const int a = sp_row[2 * (size_t)q], b = sp_row[2 * (size_t)q + 1];
            if (own(a)) {
                const size_t pa = pos_of(ss_ptr, a, cnt_s[a]++);
                S_other[pa] = b; S_d0[pa] = s.sp_d0[q]; e->sp_pos[2 * (size_t)q] = (int)pa;
            }
            if (own(b)) {
                const size_t pb = pos_of(ss_ptr, b, cnt_s[b]++);
                S_other[pb] = a; S_d0[pb] = s.sp_d0[q]; e->sp_pos[2 * (size_t)q + 1] = (int)pb;
            }
        }
        for (int q = 0; q < s.n_dm; ++q) {
            const int* r4 = &dm_row[4 * (size_t)q];
            if (!(own(r4[0]) || own(r4[1]) || own(r4[2]) || own(r4[3]))) continue;
            for (int role = 0; role < 4; ++role) {
                if (r4[role] < 0 || !own(r4[role])) continue;
                const size_t pz = pos_of(sd_ptr, r4[role], cnt_d[r4[role]]++);
                int z = 0;
                for (int k = 0; k < 4; ++k)
                    if (k != role) D_o[3 * pz + z++] = r4[k];
                D_w[pz] = s.dm_w[q];
                D_role[pz] = role;
                e->dm_pos[4 * (size_t)q + role] = (int)pz;
            }
        }
        for (int q = 0; q < s.n_un; ++q) {       // own role 2 (1n, +), value-only other in role 3 (2n, -)
            const int row = un_row[q];
            if (!own(row)) continue;
            const size_t pz = pos_of(sd_ptr, row, cnt_d[row]++);
            D_o[3 * pz + 2] = e->vrow[s.un_ij[2 * q + 1]];
            D_w[pz] = s.un_w[q];
            D_role[pz] = 2;
            e->un_pos[q] = (int)pz;
        }
    });
    mark("sell pack");
    mark("sell vectors");
}

void HostBuild::temporal_form() {
    // ---- temporal-difference form of the dampers (nrs_engine_types.hpp), OPT-IN (NRS_DFORM=1).  Measured: C2 (cache
    // resident) operator 24.4 -> 24.9 us, lineariser 42 -> 43 us: neutral; C4 (HBM regime) operator 1.77 -> 4.15 ms,
    // lineariser 3.08 -> 5.69 ms: the three gathers per staged row (v, v[next], v[prev]; 954 row reads per tile against
    // 648 for the generic halo) cost more than the LDS reads and instructions they save.  Kept because it is parity-green
    // and the natural form once G^f / G^b come from a streaming pre-pass.  Needs every damper to join the same two
    // vertices' successors -- next(1c) = 1n, next(2c) = 2n, consistently over all dampers -- a BA window without masks,
    // offsets or unary dampers, and the two-kernel path (the fused single-launch iteration re-derives u for halo rows
    // and keeps the generic four-vertex records)
    {
        const int fused_max0 = c->dbg.int_of(SW_FUSED_MAX_ROWS);
        bool plain = !s.X0 && s.n_un == 0 && s.n_dm > 0 && !s.sp_active && !s.dm_active && !s.pose_fixed && !c->dbg.is_set(SW_NO_EDGE_CHI) && c->dbg.is_set(SW_DFORM) &&
                     !c->dbg.is_set(SW_NO_LDS) && !s.force_gather;
        for (int v = 0; v < s.M && plain; ++v) plain = !(s.rflag[v] & RF_FIXED);
        const bool two_kernel = d.n_rows >= fused_max0 || c->dbg.is_set(SW_NO_FUSED) || (c->comm && s.shard);
        if (plain && two_kernel) {
            nxt_row.assign(d.n_rows, -1); prv_row.assign(d.n_rows, -1);
            for (int q = 0; q < s.n_dm && plain; ++q) {
                int r4[4];
                for (int k = 0; k < 4; ++k) { r4[k] = s.dm_idx[4 * (size_t)q + k] >= 0 ? e->vrow[s.dm_idx[4 * (size_t)q + k]] : -1; plain = plain && r4[k] >= 0; }
                if (!plain) break;
                for (int h = 0; h < 2 && plain; ++h) {
                    const int cur = r4[h], nx = r4[2 + h];
                    if ((nxt_row[cur] >= 0 && nxt_row[cur] != nx) || (prv_row[nx] >= 0 && prv_row[nx] != cur) || cur == nx) plain = false;
                    nxt_row[cur] = nx; prv_row[nx] = cur;
                }
            }
            d.dform = plain ? 1 : 0;
        }
        if (!d.dform) { nxt_row.clear(); prv_row.clear(); }
    }
}

void HostBuild::halo_lists() {
    // ---- LDS staging: per workgroup (= 4 slices = BLK/T rows) the sorted list of rows referenced
    // outside the tile; neighbour ids become tile-local
    halo_ptr.assign(d.n_regblk + 1, 0); halo_ns.assign(d.n_regblk, 0);
    L_s.assign(nnz_s, -1); L_d.assign(3 * nnz_d, -1);          // tile-local ids
    {
        // tiles are independent: a few host threads each take a contiguous range of tiles
        int nt = std::max(1, std::min({8, (int)std::thread::hardware_concurrency(), d.n_regblk / 32}));   // (a 4.5k-point frame: 4 threads, 1.5 -> 0.5 ms)
        if (c->dbg.is_set(SW_HOST_THREADS)) nt = std::min(c->dbg.int_of(SW_HOST_THREADS), std::max(1, d.n_regblk));
        std::vector<std::vector<int>> part(nt);
        std::vector<int> cnt(d.n_regblk, 0);
        auto work = [&](int ti) {
            const int b0 = (int)((int64_t)d.n_regblk * ti / nt), b1 = (int)((int64_t)d.n_regblk * (ti + 1) / nt);
            std::vector<int> stamp(d.n_rows, -1), local(d.n_rows, 0), ext;
            for (int b = b0; b < b1; ++b) {
                const int row0 = b * d.tile_rows, row1 = row0 + d.tile_rows;
                ext.clear();
                const size_t s0 = (size_t)ss_ptr[b * 4], s1 = (size_t)ss_ptr[b * 4 + 4];
                const size_t d0 = (size_t)sd_ptr[b * 4], d1 = (size_t)sd_ptr[b * 4 + 4];
                auto see = [&](int o) {
                    if (o >= 0 && (o < row0 || o >= row1) && stamp[o] != b) { stamp[o] = b; ext.push_back(o); }
                };
                // spring neighbours first (the SpMV stages positions for them only), then damper-only rows
                for (size_t p2 = s0; p2 < s1; ++p2) see(S_other[p2]);
                const size_t ns = ext.size();
                if (d.dform) {                                     // the partner in the same keyframe: 2c / 1c (slot 0) or 2n / 1n (slot 2)
                    for (size_t p2 = d0; p2 < d1; ++p2)
                        if (D_role[p2] >= 0) see(D_o[3 * p2 + (D_role[p2] < 2 ? 0 : 2)]);
                } else
                    for (size_t p2 = 3 * d0; p2 < 3 * d1; ++p2) see(D_o[p2]);
                std::sort(ext.begin(), ext.begin() + ns);
                std::sort(ext.begin() + ns, ext.end());
                halo_ns[b] = (int)ns;
                for (size_t i = 0; i < ext.size(); ++i) local[ext[i]] = d.tile_rows + (int)i;
                auto loc = [&](int o) { return o < 0 ? -1 : (o >= row0 && o < row1) ? o - row0 : local[o]; };
                for (size_t p2 = s0; p2 < s1; ++p2) L_s[p2] = loc(S_other[p2]);
                for (size_t p2 = 3 * d0; p2 < 3 * d1; ++p2) L_d[p2] = loc(D_o[p2]);
                part[ti].insert(part[ti].end(), ext.begin(), ext.end());
                cnt[b] = (int)ext.size();
            }
        };
        mark("halo prep");
        parallel_for(nt, [&](int ti, int) { work(ti); });          // (a share runs inline when no thread can be created)
        mark("halo work");
        for (int b = 0; b < d.n_regblk; ++b) halo_ptr[b + 1] = halo_ptr[b] + cnt[b];
        halo_rows.reserve((size_t)halo_ptr[d.n_regblk]);
        for (int ti = 0; ti < nt; ++ti) halo_rows.insert(halo_rows.end(), part[ti].begin(), part[ti].end());
    }
    mark("halo lists");
}

// ---- the decisions both packers share (nrs_engine_plan.hpp): tile classes, LDS and path flags, the shard window
int HostBuild::decide() {
    {
        std::vector<int> hs(d.n_regblk);
        for (int b = 0; b < d.n_regblk; ++b) hs[b] = halo_ptr[b + 1] - halo_ptr[b];
        tile_list = tile_classes(c, d, hs, halo_ns);
    }
    path_flags(c, d, s);
    std::vector<int> lo, hi, blo, bhi;                             // what the tiles of a sharded window reach (TileReach): one pass over the halo lists
    if (c->comm && s.shard) {
        lo.assign(d.n_regblk, INT_MAX); hi.assign(d.n_regblk, -1);
        for (int b = 0; b < d.n_regblk; ++b)
            for (int i = halo_ptr[b]; i < halo_ptr[b + 1]; ++i) { lo[b] = std::min(lo[b], halo_rows[i]); hi[b] = std::max(hi[b], halo_rows[i]); }
        if (d.dform) {                                             // ... and the temporal partners of its halo rows and of its own rows
            blo = lo; bhi = hi;
            auto see = [&](int b, int r) { if (r >= 0) { blo[b] = std::min(blo[b], r); bhi[b] = std::max(bhi[b], r); } };
            for (int b = 0; b < d.n_regblk; ++b) {
                for (int i = halo_ptr[b]; i < halo_ptr[b + 1]; ++i) { see(b, nxt_row[halo_rows[i]]); see(b, prv_row[halo_rows[i]]); }
                for (int r = b * d.tile_rows; r < (b + 1) * d.tile_rows; ++r) { see(b, nxt_row[r]); see(b, prv_row[r]); }
            }
        }
    }
    const bool wide = !blo.empty();
    NRS_TRY(shard_window(c, d, e->halo, s, g, tile_list, TileReach{lo.data(), hi.data(), wide ? blo.data() : lo.data(), wide ? bhi.data() : hi.data()}));
    mark("halo");
    if (mark.on) fprintf(stderr, "[nrs] tiles %d x %d rows (T=%d), halo rows: max %d, mean %.1f, spring part max %d, classes %d (cap %d/%d) + %d (cap %d/%d), lds %d, fused %d\n", d.n_regblk, d.tile_rows, T, d.max_halo, (double)halo_rows.size() / d.n_regblk, d.max_halo_s, d.n_tiles_cls[0], d.cap_h[0], d.cap_s[0], d.n_tiles_cls[1], d.cap_h[1], d.cap_s[1], d.use_lds, d.fused);
    if (mark.on) fprintf(stderr, "[nrs] coarse level: wanted %d (fused %d, K %d, unknowns %d <= %d), enabled %d\n", d.fused && s.K == 1, d.fused, s.K, 3 * d.n_groups + 6, CO_MAX, d.coarse);
    return NRS_OK;
}

// edge lists for the chi2-only evaluation of trial states (BA form, nothing masked or fixed): each
// edge once, ordered by the row that counts it (locality of the gathers); a rank keeps the edges it counts
void HostBuild::ec_lists_build() {
    const int own_lo = d.sh_g0 * ROW_ALIGN, own_hi = (d.sh_g0 + d.sh_ng) * ROW_ALIGN;
    // counting sort by the counting row (stable: edges of a row keep their order); threads: keys and counts are
    // order-free, the scatter gives every thread a range of rows and scans the keys in edge order
    std::vector<int> key, pos(d.n_rows + 1);
    auto order_by_row = [&](int n_edges, auto row_of) {
        key.assign(n_edges, -1);
        std::fill(pos.begin(), pos.end(), 0);
        parallel_for(nt_all, [&](int ti, int n) {
            int64_t a, b;
            chunk(n_edges, ti, n, a, b);
            for (int64_t q = a; q < b; ++q) {
                const int r = row_of((int)q);
                if (r >= own_lo && r < own_hi) { key[q] = r; count_up(&pos[r + 1], n); }
            }
        });
        for (int r = 0; r < d.n_rows; ++r) pos[r + 1] += pos[r];
        std::vector<int> out(pos[d.n_rows]);
        std::vector<int> cut(nt_all + 1, d.n_rows);
        cut[0] = 0;
        for (int t = 1, r = 0; t < nt_all; ++t) {
            const int64_t want = (int64_t)out.size() * t / nt_all;
            while (r < d.n_rows && pos[r] < want) ++r;
            cut[t] = r;
        }
        parallel_for(nt_all, [&](int ti, int) {
            const int lo = cut[ti], hi = cut[ti + 1];
            if (lo >= hi) return;
            for (int q = 0; q < n_edges; ++q)
                if (key[q] >= lo && key[q] < hi) out[pos[key[q]]++] = q;
        });
        return out;
    };
    const std::vector<int> so = order_by_row(s.n_sp, [&](int q) { return sp_row[2 * (size_t)q]; });
    ec_sp.resize(so.size());
    parallel_for(nt_all, [&](int ti, int n) {
        int64_t a, b;
        chunk((int64_t)so.size(), ti, n, a, b);
        for (int64_t i = a; i < b; ++i) { const int q = so[i]; ec_sp[i] = EcSpring{sp_row[2 * (size_t)q], sp_row[2 * (size_t)q + 1], s.sp_d0[q], 0}; }
    });
    const std::vector<int> dord = order_by_row(s.n_dm, [&](int q) {
        for (int k = 0; k < 4; ++k) if (dm_row[4 * (size_t)q + k] >= 0) return dm_row[4 * (size_t)q + k];
        return -1;
    });
    ec_dm.resize(dord.size()); ec_w.resize(dord.size());
    parallel_for(nt_all, [&](int ti, int n) {
        int64_t a, b;
        chunk((int64_t)dord.size(), ti, n, a, b);
        for (int64_t i = a; i < b; ++i) {
            const int q = dord[i];
            for (int k = 0; k < 4; ++k) ec_dm[i].r[k] = dm_row[4 * (size_t)q + k];
            ec_w[i] = s.dm_w[q];
        }
    });
}

// ---- chi2 edge lists, the specialised (plain) lineariser's conditions, and the temporal partners of its rows
void HostBuild::edge_lists() {
    bool plain = !s.X0 && s.n_un == 0 && !s.sp_active && !s.dm_active && !s.pose_fixed && !c->dbg.is_set(SW_NO_EDGE_CHI);
    for (int v = 0; v < s.M && plain; ++v) plain = !(s.rflag[v] & RF_FIXED);
    d.ec_on = plain ? 1 : 0;
    {   // the specialised lineariser additionally wants every damper with its four vertices and springs without a kernel
        bool p4 = plain && d.use_lds && !d.dform && !(s.delta_pos > 0) && s.spring_form == 0 && !c->dbg.is_set(SW_NO_PLAIN);
        for (int64_t q = 0; q < 4 * (int64_t)s.n_dm && p4; ++q) p4 = s.dm_idx[q] >= 0;
        d.plain = p4 ? 1 : 0;
        if (d.plain) d.lin_rb = ROW_ALIGN / (64 / T);          // k_lin_plain leaves one partial slot per SLICE (no workgroup barrier behind its loops)
    }
    if (plain) ec_lists_build();
    // temporal partners of every row (plain windows): from the dampers' canonical second vertex; all dampers of a row and
    // direction must agree (they do for the reference's BA dampers), else the kernels read it per incidence as before
    d.tp_ok = 0; d.h4 = 0;
    if (d.plain) {
        static const int perm1[4] = {1, 2, 0, 1};                  // (perm[role][1] of the canonical order below)
        row_tp.assign((size_t)d.n_rows, 0xFFFFFFFFu);
        bool ok = true;
        for (int r = 0; r < d.n_rows && ok; ++r)
            for (int k = 0; k < cnt_d[r] && ok; ++k) {
                const size_t pz = pos_of(sd_ptr, r, k);
                const int role = D_role[pz];
                const uint32_t l = (uint32_t)(L_d[3 * pz + perm1[role]] & 0xFFFF);
                const int sh = role < 2 ? 0 : 16;
                const uint32_t cur = (row_tp[r] >> sh) & 0xFFFFu;
                if (cur != 0xFFFFu && cur != l) ok = false;
                row_tp[r] = (row_tp[r] & ~(0xFFFFu << sh)) | (l << sh);
            }
        d.tp_ok = ok ? 1 : 0;
    }
    d.ec_nsp = (int)ec_sp.size(); d.ec_ndm = (int)ec_dm.size();
    d.ec_nblk = std::min((d.ec_nsp + d.ec_ndm + BLK - 1) / BLK, 2048);
    mark("edge lists");
}

void HostBuild::host_mirrors() {
    e->sp_ij.assign(s.sp_ij, s.sp_ij + 2 * (size_t)s.n_sp);
    e->sp_d0.assign(s.sp_d0, s.sp_d0 + (size_t)s.n_sp);
    e->dm_idx.assign(s.dm_idx, s.dm_idx + 4 * (size_t)s.n_dm);
    e->dm_w.assign(s.dm_w, s.dm_w + (size_t)s.n_dm);
    e->un_ij.assign(s.un_ij, s.un_ij + 2 * (size_t)s.n_un);
    e->un_w.assign(s.un_w, s.un_w + (size_t)s.n_un);
    e->h_rflag.assign(d.n_rows, RF_FIXED);            // padding rows: no edges, never move
    for (int v = 0; v < s.M; ++v) e->h_rflag[e->vrow[v]] = s.rflag[v];
    e->h_pose_fixed.assign(s.K, 0);
    if (s.pose_fixed) e->h_pose_fixed.assign(s.pose_fixed, s.pose_fixed + s.K);
    uv.assign((size_t)d.n_rows * 2, 0.f);
    xl.assign((size_t)d.n_rows * 3, 0.0);
    if (s.X0) X0.assign((size_t)d.n_rows * 3, 0.0);
    for (int v = 0; v < s.M; ++v) {
        const size_t row = (size_t)e->vrow[v];
        uv[2 * row] = s.uv[2 * v];
        uv[2 * row + 1] = s.uv[2 * v + 1];
        for (int k = 0; k < 3; ++k) {
            xl[3 * row + k] = s.x[3 * (size_t)v + k];
            if (s.X0) X0[3 * row + k] = s.X0[3 * (size_t)v + k];
        }
    }
    e->h_s_meta.assign(nnz_s, 0);
    e->h_d_meta.assign(nnz_d, -1);
    const int nt_mir = nt_all;
    parallel_for(nt_mir, [&](int ti, int n) {
        int64_t a, b;
        chunk((int64_t)nnz_d, ti, n, a, b);
        for (int64_t i = a; i < b; ++i)
            if (D_role[i] >= 0) e->h_d_meta[i] = D_role[i];
    });
    if (d.use_lds) {
        auto u16 = [](int v) { return v < 0 ? (uint32_t)REC_NONE : (uint32_t)(v & 0xFFFF); };
        e->h_s_om.resize(nnz_s);
        parallel_for(nt_mir, [&](int ti, int n) {
            int64_t a, b;
            chunk((int64_t)nnz_s, ti, n, a, b);
            for (int64_t i = a; i < b; ++i) e->h_s_om[i] = u16(L_s[i]);                        // meta: push_masks
        });
        if (d.dform) {
            e->h_d_om.resize(nnz_d);
            for (size_t i = 0; i < nnz_d; ++i) e->h_d_om[i] = D_role[i] < 0 ? (uint32_t)REC_NONE : u16(L_d[3 * i + (D_role[i] < 2 ? 0 : 2)]);
        } else {
            // canonical order of the three other vertices, so that every role evaluates the same expression
            //   g = (v_i - v[o1]) - (v[o0] - v[o2])   (= sg_i * sum_k sg_k v_k; absent vertices read zeros):
            // o0 = the partner in the same keyframe, o1 = the own temporal partner, o2 = the partner's temporal partner
            static const int perm[4][3] = {{0, 1, 2}, {0, 2, 1}, {2, 0, 1}, {2, 1, 0}};    // indices into the others in ascending role order
            e->h_d_hdr.resize(nnz_d);
            parallel_for(nt_mir, [&](int ti, int n) {
                int64_t a, b;
                chunk((int64_t)nnz_d, ti, n, a, b);
                for (int64_t i = a; i < b; ++i) {
                    const int* pm = perm[D_role[i] < 0 ? 0 : D_role[i]];
                    e->h_d_hdr[i] = make_uint2(u16(L_d[3 * i + pm[0]]) | (u16(L_d[3 * i + pm[1]]) << 16), u16(L_d[3 * i + pm[2]]) | ((uint32_t)REC_NONE << 16));
                }
            });
        }
    } else {
        d_o0.resize(nnz_d); d_o1.resize(nnz_d); d_o2.resize(nnz_d);
        for (size_t i = 0; i < nnz_d; ++i) { d_o0[i] = D_o[3 * i]; d_o1[i] = D_o[3 * i + 1]; d_o2[i] = D_o[3 * i + 2]; }
    }
    mark("host mirrors");
}

int HostBuild::uploads() {
    poses.assign(s.poses, s.poses + s.K);
    NRS_TRY(h2d(c, d.grp_pose, g.grp_pose));
    NRS_TRY(h2d(c, d.pose_grp_ptr, g.pose_grp_ptr));
    NRS_TRY(h2d_rows(c, d, d.uv, uv, 2));
    if (d.row_hi - d.row_lo < d.n_rows) e->h_uv = uv;              // (a row-limited rank: the residual taps stage the observations of every row from here)
    NRS_TRY(h2d_rows(c, d, d.xl_init, xl, 3));
    if (s.X0) NRS_TRY(h2d_rows(c, d, d.X0, X0, 3));
    NRS_TRY(h2d(c, d.pose_init, poses));
    NRS_TRY(h2d(c, d.ss_ptr, ss_ptr));
    NRS_TRY(h2d(c, d.sd_ptr, sd_ptr));
    NRS_TRY(h2d(c, d.halo_ptr, halo_ptr));
    NRS_TRY(h2d(c, d.halo_rows, halo_rows));
    NRS_TRY(h2d(c, d.halo_ns, halo_ns));
    NRS_TRY(h2d(c, d.tile_list, tile_list));
    if (d.dform) {
        std::vector<int> hn(halo_rows.size()), hp(halo_rows.size());
        for (size_t i = 0; i < halo_rows.size(); ++i) { hn[i] = nxt_row[halo_rows[i]]; hp[i] = prv_row[halo_rows[i]]; }
        NRS_TRY(h2d(c, d.nxt_row, nxt_row));
        NRS_TRY(h2d(c, d.prv_row, prv_row));
        NRS_TRY(h2d(c, d.halo_nxt, hn));
        NRS_TRY(h2d(c, d.halo_prv, hp));
        NRS_HIP(c, hipStreamSynchronize(c->stream));               // hn / hp die here
    }
    if (d.fused) {
        tile_desc = tile_desc_build(d, g, halo_ptr);
        halo_fix.assign((size_t)BLK * d.n_regblk, 0);
        for (int b = 0; b < d.n_regblk; ++b)
            for (int i = 0; i < halo_ptr[b + 1] - halo_ptr[b] && i < BLK; ++i) halo_fix[(size_t)b * BLK + i] = halo_rows[halo_ptr[b] + i];
        NRS_TRY(h2d(c, d.tile_desc, tile_desc));
        NRS_TRY(h2d(c, d.halo_fix, halo_fix));
    } else if (d.plain && d.use_lds) {                             // stage_rows<true>: the first HALO_FIX halo rows at a fixed stride
        halo_fix.assign((size_t)HALO_FIX * d.n_regblk, -1);
        for (int b = 0; b < d.n_regblk; ++b) {
            const int hn = std::min(halo_ptr[b + 1] - halo_ptr[b], HALO_FIX);
            for (int i = 0; i < hn; ++i) halo_fix[(size_t)b * HALO_FIX + i] = halo_rows[halo_ptr[b] + i];
        }
        NRS_TRY(h2d(c, d.halo_fix, halo_fix));
    }
    NRS_TRY(h2d(c, d.s_d0, S_d0));
    if (!d.use_lds) {
        NRS_TRY(h2d(c, d.s_other, S_other));
        NRS_TRY(h2d(c, d.d_o0, d_o0));
        NRS_TRY(h2d(c, d.d_o1, d_o1));
        NRS_TRY(h2d(c, d.d_o2, d_o2));
    }
    NRS_TRY(h2d(c, d.d_w, D_w));
    if (d.plain) NRS_TRY(h2d_rows(c, d, d.row_tp, row_tp, 1));
    if (d.plain) {
        std::vector<uint32_t> rc((size_t)d.n_rows);
        for (int r = 0; r < d.n_rows; ++r) rc[r] = (uint32_t)cnt_s[r] | ((uint32_t)cnt_d[r] << 16);
        NRS_TRY(h2d_rows(c, d, d.row_cnt, rc, 1));
        NRS_HIP(c, hipStreamSynchronize(c->stream));               // (rc dies here)
    }
    if (d.ec_on) {
        NRS_TRY(h2d(c, d.ec_sp, ec_sp));
        NRS_TRY(h2d(c, d.ec_dm, ec_dm));
        NRS_TRY(h2d(c, d.ec_w, ec_w));
    }
    NRS_TRY(push_masks(c, e, s.sp_active, s.dm_active));
    e->serial = ++c->engine_serial;                                // (the residual taps are staged on first use: engine_residuals)
    NRS_TRY(zero_work_arrays(c, d));
    mark("uploads enqueued");
    return NRS_OK;
}

int engine_create(nrs_ctx* c, const EngineSpec& s, Arena* arena, Engine** out) {
    *out = nullptr;
    // failures every rank of a sharded upload sees alike (argument validation on identical inputs) are reported
    // without a collective; everything else is rank-local and is agreed on by the caller (nrs_dba_upload)
    c->err_local = false;
    NRS_TRY(spec_validate(c, s));
    c->err_local = true;                                           // from here on a failure may be this rank's alone: the caller lets the ranks agree
    const RowGroups g = row_groups(s);
    NRS_HIP(c, hipSetDevice(c->device));
    Engine* e = new (std::nothrow) Engine();
    if (!e) return c->fail(NRS_ERR_ALLOC, "out of host memory");
    struct Guard { nrs_ctx* c; Engine* e; bool keep = false; ~Guard() { if (!keep) engine_destroy(c, e); } } guard{c, e};
    e->arena = arena;
    HostBuild B{c, s, e, e->d, g, lanes_per_row(c, g.n_pad_rows)};
    StageTimer& mark = B.mark;
    DeviceBuild D{c, s, e, e->d, g, arena, B.T};                    // a plain BA window is built on the device, stage by stage (nrs_engine_devpack.hpp)
    if (D.precheck()) {
        NRS_TRY(D.uploads());
        NRS_TRY(D.row_layout());
        NRS_TRY(D.incidences());
        NRS_TRY(D.fill_and_halo_sizes());
        NRS_TRY(D.decide());
        if (D.why == DP_BUILT) {
            NRS_TRY(D.final_arrays());
            NRS_TRY(D.host_side());
            guard.keep = true; *out = e;
            return NRS_OK;
        }
        *e = Engine();                                             // (did not qualify after all: the host path, from scratch)
        e->arena = arena;
    }
    if (D.mark.on && D.why != DP_INELIGIBLE) fprintf(stderr, "[nrs] device pack: host path (%s)\n", dp_reason_name(D.why));   // (a window that was a candidate)
    if (s.edges_on_device) return c->fail(NRS_ERR_STATE, "device-built edge lists need the device-side construction, which this window does not qualify for");
    // a2's single-frame engines: the direct solver's symbolic phase needs the structure only and runs next to the packing below
    if (s.sk_window() > 0) {                                       // (checked HERE: the plan thread below indexes by these)
        if ((!(arena == &c->arena_trk && s.K == 1) && !s.sk_pose) || !s.sk_uv || !s.sk_X0 || !s.sk_node || !s.sk_om)
            return c->fail(NRS_ERR_INVALID, "skinned observations: single-frame tracking engines, or BA windows with a pose per observation");
        for (size_t q = 0; q < (size_t)SK_MAX * s.n_skin; ++q)
            if (s.sk_node[q] >= s.M || s.sk_node[q] < -1) return c->fail(NRS_ERR_INVALID, "skinned observation: node index out of range");
    }
    NdPrep nd_prep;                                                // (declared after `guard`: joined before the engine can go away)
    NdIn nd_in;
    if (arena == &c->arena_trk && s.K == 1) NRS_TRY(nd_plan_start(c, s, e, nd_in, nd_prep));
    Dev& d = e->d;
    dev_init(d, s, g, B.T);
    B.row_layout();
    B.incidence_rows();
    B.sell_pack();
    B.temporal_form();
    B.halo_lists();
    NRS_TRY(B.decide());
    B.edge_lists();
    if (!e->nd) spec_pcg_sets(c, e, s.sk_window());                // shadow sets for speculative LM trials, carved with the arena (a2's engines chose theirs above)
    NRS_TRY(arena_fit(c, arena, e, d, s.X0 != nullptr, B.nnz_s, B.nnz_d, (size_t)B.n_slices, B.halo_rows.size()));
    mark("arena");
    B.host_mirrors();
    NRS_TRY(B.uploads());
    NRS_TRY(pin_host_words(c, e));
    if (e->n_spec > 0) NRS_TRY(spec_prepare(c, e));
    engine_compact_headers(c, e);
    NRS_HIP(c, hipStreamSynchronize(c->stream));       // B's staging vectors may die from here on
    mark("pinned+sync");
    if (s.sk_window() > 0) NRS_TRY(skin_setup(c, e, s, arena));
    if (e->nd) {                                                   // direct solve when the frame is small enough to gain from it
        NRS_TRY(nd_engine_finish(c, e, e->nd, nd_prep));
        mark("direct solve plan");
    }
    d.sk_pcg = (d.sk_n > 0 && !(e->nd && e->nd->on)) ? 1 : 0;      // (on the direct solver k_nd_values folds the observations into its blocks)
    if (d.sk_pcg) d.ecd = 0;                                       // (k_pcg_update<true> owns 16 rows a workgroup: no r.u partials per 256 rows for the operator's early test -- one launch in hundreds)
    // embedded BA window: the keyframe-block factorisation as the PCG's preconditioner.  On a communicator only with sharded_kft = 1 (a
    // sharded window reduces hierarchically: the factorisation's u replaces the update's after the all-reduced scalars, as on one GPU)
    if (d.sk_pcg && s.sk_pose && d.use_lds && (d.sh_on ? c->opt.sharded_kft == 1 : !d.hier) && c->opt.embedded_solver != 2) {
        NRS_TRY(kft_setup(c, e, s, g.pose_grp_ptr));
        mark("keyframe-block factorisation plan");
    }
    NRS_TRY(engine_reset(c, e));
    guard.keep = true;
    *out = e;
    return NRS_OK;
}

void engine_stats(const Engine* e, int64_t stats[5]) {
    stats[0] = e->d.n_rows; stats[1] = e->pack_rows; stats[2] = e->d.ss_nnz; stats[3] = e->d.sd_nnz; stats[4] = (int64_t)e->arena_bytes;
}

void engine_destroy(nrs_ctx* c, Engine* e) {
    if (!e) return;
    (void)hipStreamSynchronize(c->stream);
    nd_engine_free(c, e->nd);
    delete e->kft;
    delete e;
}

int engine_update_flags(nrs_ctx* c, Engine* e, const uint8_t* rflag, const uint8_t* pose_fixed,
                        const uint8_t* sp_active, const uint8_t* dm_active) {
    // (checked before anything is touched: a rejected call leaves the engine as it was)
    if (e->d.plain) return c->fail(NRS_ERR_STATE, "masks on a plain BA window: not supported (its partial slots are per slice)");
    if (rflag)
        for (int v = 0; v < e->d.M; ++v) e->h_rflag[e->vrow[v]] = rflag[v];
    if (pose_fixed) e->h_pose_fixed.assign(pose_fixed, pose_fixed + e->d.K);
    e->d.ec_on = 0;                                                // masks / fixed vertices: chi2 comes from the incidence records
    NRS_TRY(push_masks(c, e, sp_active, dm_active));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    if (e->nd) {                                                   // the direct solver's plan is built on the free rows: a changed fixed set needs a new one
        bool same = e->nd->sig.size() == (size_t)e->d.M + 1 && e->nd->sig[e->d.M] == e->h_pose_fixed[0];
        for (int v = 0; v < e->d.M && same; ++v) same = e->nd->sig[v] == (e->h_rflag[e->vrow[v]] & RF_FIXED);
        if (!same) NRS_TRY(nd_engine_setup(c, e, e->nd));
        e->d.sk_pcg = (e->d.sk_n > 0 && !e->nd->on) ? 1 : 0;
        if (e->d.sk_pcg) e->d.ecd = 0;
    }
    return NRS_OK;
}

int engine_reset(nrs_ctx* c, Engine* e) {
    Dev& d = e->d;
    e->cur = 0;
    e->pred_iters = 0; e->pred_peek = 0; e->first_trial_accepted = false;   // batch-size predictors start fresh, as in a new engine
    NRS_HIP(c, hipMemcpyAsync(d.pose[0], d.pose_init, sizeof(Pose) * d.K, hipMemcpyDeviceToDevice, c->stream));
    const size_t o = 3 * (size_t)d.row_lo, n = 3 * (size_t)(d.row_hi - d.row_lo);                  // (the rows this engine holds: all of them on one GPU)
    NRS_HIP(c, hipMemcpyAsync(d.xl[0] + o, d.xl_init + o, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(d.xl[1] + o, d.xl_init + o, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
    return NRS_OK;
}

}  // namespace nrs

namespace nrs {
int engine_skin_set_active(nrs_ctx* c, Engine* e, const uint8_t* active) {
    if (e->d.sk_n <= 0) return NRS_OK;
    std::vector<uint8_t> act((size_t)e->d.sk_n, 0);                // (slots are pose-grouped and padded: padding stays inactive)
    for (size_t i = 0; i < e->sk_slot.size(); ++i) if (e->sk_slot[i] >= 0) act[e->sk_slot[i]] = active[i];
    NRS_HIP(c, hipMemcpyAsync(const_cast<uint8_t*>(e->d.sk_active), act.data(), act.size(), hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    return NRS_OK;
}
// embedded BA window: the skinned points at the current estimate, X0 + sum_k om_k (x_{n_k} - x_start_{n_k}), summed over k in order:
// k_skin_positions (nrs_engine_skin.hpp), one thread per held slot, into a zeroed vector of the WINDOW's observations (caller order; a
// sliced list starts at sk_base in it).  Sharded: COLLECTIVE -- a rank evaluates the observations it holds from its own rows (the only rows
// they reach), zeros elsewhere, and the vector is summed over the ranks where it stands: every rank returns the same bits.
int engine_skin_positions(nrs_ctx* c, Engine* e, double* xyz) {
    const Dev& d = e->d;
    if (!d.sk_pcg) return c->fail(NRS_ERR_STATE, "no skinned observations on this window");
    const size_t m = 3 * (size_t)e->sk_total;
    if (m == 0) return NRS_OK;
    NRS_TRY(c->ensure(c->gather_ws, 2 * sizeof(double) * m));
    double* in = c->gather_ws.as<double>();
    NRS_HIP(c, hipMemsetAsync(in, 0, sizeof(double) * m, c->stream));
    hipLaunchKernelGGL(k_skin_positions, dim3(d.sk_nblk), dim3(BLK), 0, c->stream, d, d.xl[e->cur], e->sk_base, e->sk_total, in);
    NRS_HIP(c, hipGetLastError());
    const double* res = in;
    if (d.sh_on) { NRS_TRY(c->comm->allreduce(c, in, in + m, m)); res = in + m; }
    NRS_HIP(c, hipMemcpyAsync(xyz, res, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    c->gather_ws.reset();
    return NRS_OK;
}
int engine_skin_stats(const Engine* e, int64_t out[3]) {
    if (e->d.sk_n <= 0) return NRS_ERR_STATE;
    int64_t held = 0;
    for (int s : e->sk_slot) held += s >= 0;
    out[0] = held; out[1] = e->d.sk_n; out[2] = (int64_t)e->sk_bytes;
    return NRS_OK;
}
int engine_skin_chi2(nrs_ctx* c, Engine* e, double* chi) {
    const Dev& d = e->d;
    if (d.sk_n <= 0) return NRS_OK;
    hipLaunchKernelGGL((k_skin<false>), dim3(d.sk_nblk), dim3(BLK), 0, c->stream, d, d.pose[e->cur], d.xl[e->cur]);
    NRS_HIP(c, hipGetLastError());
    {                                                              // (slots are pose-grouped and padded: back to the caller's order)
        std::vector<double> h((size_t)d.sk_n);
        NRS_HIP(c, hipMemcpyAsync(h.data(), d.sk_chi, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
        NRS_HIP(c, hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < e->sk_slot.size(); ++i) chi[i] = e->sk_slot[i] >= 0 ? h[e->sk_slot[i]] : 0.0;
    }
    return NRS_OK;
}
}  // namespace nrs
