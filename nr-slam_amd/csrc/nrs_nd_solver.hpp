// Host side of the direct solver (kernels: nrs_nd_kernels.hpp): a plan with its device arrays (NdSolver), their upload and the
// launches of one factorise + solve.  Part of nrs_engine.hip (one translation unit).
#pragma once
#include "nrs_nd_kernels.hpp"

namespace nrs {

// One device buffer laid out as arrays at 256-byte-aligned offsets, with a host image of its leading arrays that goes up in one
// copy: take() hands out the offsets, put() fills the image, at() turns an offset into a device pointer.  (The nd uploads only:
// the other staging images of the engine pad differently on purpose.)
struct NdStage {
    size_t off = 0;                  // bytes handed out so far
    char* img = nullptr;             // host image (set once its length is known)
    char* base = nullptr;            // device buffer (set once it is large enough)
    size_t take(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; }
    void put(size_t o, const void* src, size_t bytes) const { if (bytes) memcpy(img + o, src, bytes); }
    template <class T> T* at(size_t o) const { return reinterpret_cast<T*>(base + o); }
};

struct NdSolver {
    NdSolver() = default;
    NdSolver(NdSolver&&) = delete;   // `buf` may point at `own`: a solver stays where it was made (cache slots are held by pointer)
    NdSolver& operator=(NdSolver&&) = delete;
    NdPlan plan;
    NdDev dev;
    DevBuf own;                      // everything the kernels read: plan arrays, entry values, assembly areas, L, x ...
    DevBuf* buf = &own;              // ... in the solver's own buffer (the tap) or in the context's (engines: reused from frame to frame)
    std::vector<size_t> lvl_shm_fac;
    std::vector<char> h_stage;       // host image of the plan arrays (one upload)
    int epoch = 0;                   // solves so far (the flags of the single-launch back pass count them)
    int chained = 0;                 // ... of which with the single-launch factorisation (its per-front counters count those)
    int chain_from = 0;              // the levels from here up run as ONE launch (their workgroups are resident at once); n_levels: none
    size_t shm_back_all = 0;
    bool attr_set = false;
    double* d_ev = nullptr;
    const NdEnt* d_ent = nullptr;
    int n_alt = 0;                   // further sets of everything a solve WRITES (factor, assembly areas, unknowns, per-front words): speculative LM trials
    size_t alt_stride = 0;           // ... each this many bytes behind the one before (set before nd_upload; nd_alt_dev)
};

// the device view of solve set j >= 0 of the alternates (same plan and entry values, its own factor storage); the caller points out_rows /
// out_pose / flags at its own vectors
static NdDev nd_alt_dev(const NdSolver& S, int j) {
    NdDev D = S.dev;
    const size_t shift = (size_t)(j + 1) * S.alt_stride;
    D.Lp = reinterpret_cast<double*>(reinterpret_cast<char*>(D.Lp) + shift); D.A = reinterpret_cast<double*>(reinterpret_cast<char*>(D.A) + shift);
    D.xn = reinterpret_cast<double*>(reinterpret_cast<char*>(D.xn) + shift);
    D.done = reinterpret_cast<int*>(reinterpret_cast<char*>(D.done) + shift); D.fcnt = reinterpret_cast<int*>(reinterpret_cast<char*>(D.fcnt) + shift);
    return D;
}

// the image's workgroup and front descriptors (hw: one per workgroup, hl: the fronts level by level), and where the chained form starts
static void nd_fill_descriptors(nrs_ctx* c, NdSolver& S, NdWgD* hw, NdFrontD* hl) {
    const NdPlan& P = S.plan;
    // (device copies of the descriptor: cmap_off, the host reference's gather map, holds the front's own index)
    // (pad: how many workgroups write into this front's assembly slots in one factorisation -- its children's (I, J) pairs)
    // the top of the tree in one launch: the highest levels whose workgroups are resident at once (one per CU), when that spares at
    // least one launch; a front's counter then counts the tiles of its children INSIDE that launch (the others are complete before it)
    std::vector<int> need(P.fr.size(), 0), lvl_of(P.fr.size(), 0);
    for (int l = 0; l < P.n_levels; ++l)
        for (int i = P.lvl_ptr[l]; i < P.lvl_ptr[l + 1]; ++i) lvl_of[P.lvl_fronts[i]] = l;
    S.chain_from = P.n_levels;
    while (S.chain_from > 0 && P.lvl_wg_ptr[P.n_levels] - P.lvl_wg_ptr[S.chain_from - 1] <= c->prop.multiProcessorCount) --S.chain_from;
    // Measured with 512-thread workgroups (round 5): the launch boundaries are the cheaper hand-over at every size -- 155 us per factorise +
    // solve against 163 chained at 543 points (everything resident), 201 / 223 at 1013, 480 / 501 at 4446 (top seven levels chained) -- so
    // the chained form is opt-in (NRS_ND_CHAIN=1, read when a plan is uploaded; the tests hold it to the per-level form bit for bit)
    if (P.n_levels - S.chain_from < 2 || !c->dbg.is_set(SW_ND_CHAIN)) S.chain_from = P.n_levels;
    for (size_t f = 0; f < P.fr.size(); ++f)
        if (P.fr[f].par >= 0 && lvl_of[f] >= S.chain_from) need[P.fr[f].par] += P.fr[f].nR * (P.fr[f].nR + 1) / 2;
    for (size_t w = 0; w < P.wg.size() / 3; ++w) { hw[w] = NdWgD{P.fr[P.wg[3 * w]], P.wg[3 * w + 1], P.wg[3 * w + 2], need[P.wg[3 * w]]}; hw[w].F.cmap_off = P.wg[3 * w]; }
    for (size_t i = 0; i < P.lvl_fronts.size(); ++i) { hl[i] = P.fr[P.lvl_fronts[i]]; hl[i].cmap_off = P.lvl_fronts[i]; }
}
// dynamic LDS per level and of the back pass, the kernels' attributes; NRS_ERR_INVALID: a front or a boundary beyond the LDS
static int nd_lds_sizes(nrs_ctx* c, NdSolver& S) {
    const NdPlan& P = S.plan;
    // dynamic LDS per level: the largest panel / boundary of its fronts
    S.lvl_shm_fac.assign(P.n_levels, 0); S.shm_back_all = 8 * (size_t)nd_back_fixed_doubles(0);
    for (int l = 0; l < P.n_levels; ++l)
        for (int i = P.lvl_ptr[l]; i < P.lvl_ptr[l + 1]; ++i) {
            const NdFrontD& F = P.fr[P.lvl_fronts[i]];
            const int s16 = (F.s + 15) & ~15, nrow = s16 + ND_TB + (F.nR > 1 ? ND_TB : 0);
            S.lvl_shm_fac[l] = std::max(S.lvl_shm_fac[l], sizeof(double) * ((size_t)nrow * ND_LD + ND_S16 + 256) + 2 * 32);
            S.lvl_shm_fac[l] = std::max(S.lvl_shm_fac[l], sizeof(double) * ((size_t)2 * s16 * ND_LD + ND_S16 + 256) + 2 * 32);          // (the inverse workgroup)
            {
                const int ngb = F.s <= 64 ? 4 : 2;
                const size_t want = sizeof(double) * ((size_t)nd_back_fixed_doubles(F.b) + (size_t)std::max(0, F.b - ngb * ND_BACK_UR) * F.s);
                S.shm_back_all = std::max(S.shm_back_all, std::min(want, (size_t)160 * 1024));
                if (sizeof(double) * (size_t)nd_back_fixed_doubles(F.b) > 160 * 1024) return c->fail(NRS_ERR_INVALID, "direct solve: a front's boundary does not fit the LDS");
            }
        }
    if (!S.attr_set) {
        NRS_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_nd_level<256, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        NRS_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_nd_level<512, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        NRS_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_nd_level<256, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        NRS_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_nd_level<512, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        NRS_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_nd_back), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        NRS_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_nd_tile<256>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
        NRS_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_nd_tile<512>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
        S.attr_set = true;
    }
    for (int l = 0; l < P.n_levels; ++l)
        if (S.lvl_shm_fac[l] > 160 * 1024) return c->fail(NRS_ERR_INVALID, "direct solve: a front does not fit the LDS");
    return NRS_OK;
}
static int nd_upload(nrs_ctx* c, NdSolver& S) {
    const NdPlan& P = S.plan;
    NdStage G;
    const size_t o_seg = G.take(4 * std::max<size_t>(2, P.seg.size())), o_own = G.take(4 * P.own.size()), o_bnd = G.take(4 * std::max<size_t>(1, P.bnd.size())),
                 o_pm = G.take(2 * std::max<size_t>(1, P.pmap.size())), o_ent = G.take(sizeof(NdEnt) * P.ent.size()),
                 o_wg = G.take(sizeof(NdWgD) * (P.wg.size() / 3)), o_lf = G.take(sizeof(NdFrontD) * P.lvl_fronts.size()), o_ev = G.take(72 * P.ent.size() + 64),
                 o_L = G.take(8 * P.L_doubles), o_A = G.take(8 * std::max<size_t>(2, P.A_doubles) + 64), o_x = G.take(24 * (size_t)P.n_nodes), o_fl = G.take(64), o_dn = G.take(4 * P.fr.size()), o_fc = G.take(4 * P.fr.size());
    const size_t off1 = G.off;                                     // (one set ends here)
    S.alt_stride = off1 - o_L;
    NRS_TRY(c->ensure(*S.buf, off1 + (size_t)S.n_alt * S.alt_stride));
    char* base = G.base = S.buf->as<char>();
    // the plan's arrays go up in ONE copy from a staging image that lives as long as the solver (the copy is asynchronous)
    S.h_stage.assign(o_ev, 0);
    G.img = S.h_stage.data();
    G.put(o_seg, P.seg.data(), 4 * P.seg.size());
    G.put(o_own, P.own.data(), 4 * P.own.size());
    G.put(o_bnd, P.bnd.data(), 4 * P.bnd.size());
    G.put(o_pm, P.pmap.data(), 2 * P.pmap.size());
    G.put(o_ent, P.ent.data(), sizeof(NdEnt) * P.ent.size());
    nd_fill_descriptors(c, S, reinterpret_cast<NdWgD*>(S.h_stage.data() + o_wg), reinterpret_cast<NdFrontD*>(S.h_stage.data() + o_lf));
    NRS_HIP(c, hipMemcpyAsync(base, S.h_stage.data(), o_ev, hipMemcpyHostToDevice, c->stream));
    NdDev& D = S.dev;
    memset(&D, 0, sizeof(D));
    D.seg = G.at<const int>(o_seg); D.own = G.at<const int>(o_own); D.bnd = G.at<const int>(o_bnd);
    D.pmap = G.at<const int16_t>(o_pm); D.ent = G.at<const NdEnt>(o_ent);
    D.wg = G.at<const NdWgD>(o_wg); D.lvl_fr = G.at<const NdFrontD>(o_lf);
    S.d_ev = G.at<double>(o_ev); S.d_ent = D.ent;
    D.ev = S.d_ev;
    D.Lp = G.at<double>(o_L); D.A = G.at<double>(o_A); D.xn = G.at<double>(o_x);
    D.flags = G.at<int>(o_fl); D.done = G.at<int>(o_dn); D.fcnt = G.at<int>(o_fc);
    D.n_x3 = 3 * P.n_nodes; D.x_poll = c->dbg.is_set(SW_ND_BACK_FLAGS) ? 0 : 1;
    S.epoch = 0; S.chained = 0;
    for (int j = 0; j <= S.n_alt; ++j) {
        char* bj = base + (size_t)j * S.alt_stride;
        NRS_HIP(c, hipMemsetAsync(bj + o_fl, 0, off1 - o_fl, c->stream));          // (status words and the fronts' flags)
        // the assembly areas are zero wherever no child ever writes (the written pattern is the same in every factorisation)
        NRS_HIP(c, hipMemsetAsync(bj + o_A, 0, 8 * std::max<size_t>(2, P.A_doubles) + 64, c->stream));
    }
    return nd_lds_sizes(c, S);
}

// factorise (H + lam I) and solve: 2 x levels launches on the context's stream, no host synchronisation
// back_wait / back_record (speculative trials, several solves in flight on different streams): the back pass is the one launch whose workgroups
// wait for each other, which is safe for ONE such launch at a time -- its lowest unfinished workgroup is always resident or next in its XCD's
// queue -- and not for two: each can fill the CUs of an XCD with waiting workgroups while the workgroup the other's wait for sits in that XCD's
// queue behind them (measured: a 2 s stall ended by the spin bound, NRS_ERR_HIP).  So the back passes of a batch run one after the other:
// this one starts behind the event back_wait and records back_record.  The factorisation's launches wait for nobody and overlap freely.
static int nd_solve_enqueue(nrs_ctx* c, NdSolver& S, double lam, const NdDev* alt = nullptr, int* solve_id = nullptr, hipEvent_t back_wait = nullptr,
                            hipEvent_t back_record = nullptr) {   // alt: the arrays of another solve set (nd_alt_dev)
    const NdPlan& P = S.plan;
    NdDev dev = alt ? *alt : S.dev;
    const int epoch = ++S.epoch;
    dev.abort_id = epoch;
    if (solve_id) *solve_id = epoch;
    // One launch per level.  Opt-in (NRS_ND_CHAIN=1): the TOP of the tree in ONE launch, a front's workgroups waiting for the tiles of its
    // children inside that launch -- the highest levels whose workgroups are all resident at once (one per CU), the whole factorisation
    // for frames of <= ~800 points.  It paid with 256-thread workgroups at 543 points (176 -> 165 us per factorise + solve, round 4) and
    // does not with 512-thread ones (nd_upload); NRS_ND_LEVELS=1, and the phase clocks, put every level in a launch of its own regardless.
    // "Resident at once" is what makes the waits safe and is a property of the device, not a constant: one workgroup per CU (a panel
    // fills most of a CU's LDS), so the bound is the CU count of THIS device (256 on a whole MI355X, fewer in a partition mode).  The
    // no-deadlock argument: a front's workgroups wait only for workgroups of its children, which sit at SMALLER block indices, and the
    // dispatcher hands workgroups of a launch out in block-index order -- observed on every CDNA part, not promised by HIP; hence the
    // bounded spins in k_nd_level / k_nd_back (a wait that runs out raises flags[2] = 2 -> NRS_ERR_HIP, never a hang) and the
    // resident-at-once condition, under which the order does not matter at all.
    const bool per_level = c->dbg.is_set(SW_ND_LEVELS);     // (read per call: the tests switch it between solves)
    // 512 threads per workgroup unless NRS_ND_THREADS=256 (a level is one workgroup's latency: eight waves shorten its trailing updates,
    // its reads of the children's slots and its Schur tiles; same bits either way)
    const bool wide = !(c->dbg.is_set(SW_ND_THREADS) && c->dbg.int_of(SW_ND_THREADS) == 256);
    // 32-column panel steps (k_nd_level<.., true>) unless NRS_ND_STEP32=0; same bits as the 16-column form
    const bool step32 = !(c->dbg.is_set(SW_ND_STEP32) && c->dbg.int_of(SW_ND_STEP32) == 0);
    int first = 1;                                                 // (the first launch of the solve poisons xn)
    auto level = [&](int n, size_t shm, int wg0, int chained) {
        if (wide && step32) hipLaunchKernelGGL((k_nd_level<512, true>), dim3(n), dim3(512), shm, c->stream, dev, wg0, lam, epoch, chained, first);
        else if (wide) hipLaunchKernelGGL((k_nd_level<512, false>), dim3(n), dim3(512), shm, c->stream, dev, wg0, lam, epoch, chained, first);
        else if (step32) hipLaunchKernelGGL((k_nd_level<256, true>), dim3(n), dim3(256), shm, c->stream, dev, wg0, lam, epoch, chained, first);
        else hipLaunchKernelGGL((k_nd_level<256, false>), dim3(n), dim3(256), shm, c->stream, dev, wg0, lam, epoch, chained, first);
        first = 0;
    };
    const int chain_from = per_level || dev.clk || alt ? P.n_levels : S.chain_from;   // (the per-front counters of the chained form count one set's solves)
    {
        // a CROWDED level (more workgroups than CUs: they would run in rounds, one per CU, each factorising its front's panel for one
        // tile) runs as two launches: the diagonal and inverse workgroups factorise and leave their rows of L21, k_nd_tile makes the
        // off-diagonal tiles from them (NRS_ND_NO_SPLIT=1: one launch per level throughout; the bits are the same)
        const bool no_split = c->dbg.is_set(SW_ND_NO_SPLIT);
        for (int l = 0; l < chain_from; ++l) {
            const int n = P.lvl_wg_ptr[l + 1] - P.lvl_wg_ptr[l], nA = P.lvl_wg_split[l] - P.lvl_wg_ptr[l];
            if (!no_split && n > c->prop.multiProcessorCount && n > nA) {
                level(nA, S.lvl_shm_fac[l], P.lvl_wg_ptr[l], 0);
                if (wide) hipLaunchKernelGGL(k_nd_tile<512>, dim3(n - nA), dim3(512), sizeof(double) * ND_TILE_LDS + 64, c->stream, dev, P.lvl_wg_split[l]);
                else hipLaunchKernelGGL(k_nd_tile<256>, dim3(n - nA), dim3(256), sizeof(double) * ND_TILE_LDS + 64, c->stream, dev, P.lvl_wg_split[l]);
            } else level(n, S.lvl_shm_fac[l], P.lvl_wg_ptr[l], 0);
        }
        if (chain_from < P.n_levels) {                             // the levels above in one launch (all of them when the whole factorisation is resident at once)
            size_t shm = 0;
            for (int l = chain_from; l < P.n_levels; ++l) shm = std::max(shm, S.lvl_shm_fac[l]);
            level(P.lvl_wg_ptr[P.n_levels] - P.lvl_wg_ptr[chain_from], shm, P.lvl_wg_ptr[chain_from], ++S.chained);
        }
    }
    // (Measured and dropped: the back pass on a second stream next to the last factorisation level -- only roots live there -- so that
    // its workgroups stage their factors while the root is busy.  The two event waits cost more than the ~10 us of staging they hide:
    // 224 -> 245 us per solve at 543 points, 503 -> 525 at 2220.)
    if (back_wait) NRS_HIP(c, hipStreamWaitEvent(c->stream, back_wait, 0));
    hipLaunchKernelGGL(k_nd_back, dim3(P.n_fronts), dim3(256), S.shm_back_all, c->stream, dev, (int)P.wg.size() / 3, P.n_fronts, epoch, (int)(S.shm_back_all / 8));
    NRS_HIP(c, hipGetLastError());
    if (back_record) NRS_HIP(c, hipEventRecord(back_record, c->stream));
    return NRS_OK;
}

// leaf size of the dissection (nodes): ND_LEAFN unless NRS_ND_LEAF says otherwise (a tuning knob: part of the plan cache's key)
static int nd_leaf_n(const nrs_ctx* c) {
    if (c->dbg.is_set(SW_ND_LEAF)) return std::max(4, std::min(ND_LEAFN, c->dbg.int_of(SW_ND_LEAF)));
    return ND_LEAFN;
}
}  // namespace nrs
