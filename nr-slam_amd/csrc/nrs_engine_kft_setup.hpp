// Set-up of the keyframe-block factorisation (nrs_engine_kft.hpp): the driver of the host stages (nrs_kft_prep_host.hpp, plain C++), one
// device buffer.  Part of nrs_engine.hip.
#pragma once
#include "nrs_kft_prep_host.hpp"

namespace nrs {

// the window and the context's decisions as the stages read them (kb: the ranks' keyframe ranges, filled here)
static KftIn kft_in(const nrs_ctx* c, const Engine* e, const EngineSpec& s, const std::vector<int>& pose_grp_ptr, std::vector<int>& kb) {
    const Dev& d = e->d;
    KftIn in;
    in.K = d.K; in.n_rows = d.n_rows; in.pose_grp_ptr = pose_grp_ptr.data(); in.rflag = e->h_rflag.data(); in.pose_fixed = s.pose_fixed;
    in.M = s.M; in.lm_pose = s.lm_pose; in.vrow = e->vrow.data();
    in.n_sp = s.n_sp; in.sp_ij = s.sp_ij; in.sp_pos = e->sp_pos.empty() ? nullptr : e->sp_pos.data();
    in.n_dm = s.n_dm; in.dm_idx = s.dm_idx; in.dm_pos = e->dm_pos.data();
    in.n_skin = s.n_skin; in.sk_pose = s.sk_pose; in.sk_node = s.sk_node; in.sk_om = s.sk_om; in.sk_slot = e->sk_slot.data();
    in.sh = d.sh_on && d.sh_world > 1; in.world = d.sh_world; in.sh_k0 = d.sh_k0; in.sh_nk = d.sh_nk;
    kb.assign(d.sh_world + 1, 0);
    if (in.sh && in.K >= 1) shard_plan(in.K, pose_grp_ptr.data(), d.sh_world, kb.data());
    else kb[1] = in.K;
    in.kb = kb.data();
    in.embedded_solver = c->opt.embedded_solver;
    in.lds_cap = std::max(c->prop.sharedMemPerBlock, c->prop.sharedMemPerBlockOptin);
    in.step_lds = KFT_STEP_LDS; in.panel_lds = KFT_PANEL_LDS;
    in.threads = host_threads(c, (size_t)s.n_sp + 55 * (size_t)s.n_skin);
    return in;
}

// what the stages leave for one window
struct KftPrep {
    KftNum num; KftDims dim; KftShard sd; KftEdges ed; KftSkinIndex ix;
    std::vector<KftKfLists> kl; KftPairs pairs; KftCouplings cpl; KftLayout lay;
    std::vector<int> kb;
};

// the lists into their regions, the cleared regions, and a wait for both
static int kft_upload(nrs_ctx* c, const KftPrep& P, char* base) {
    for (const KftUpload& u : kft_uploads(P.num, P.kl, P.pairs, P.cpl, P.ed.bd_slot))
        if (u.bytes) NRS_HIP(c, hipMemcpyAsync(base + P.lay.off[u.r] + u.at, u.src, u.bytes, hipMemcpyHostToDevice, c->stream));
    for (const KftSpan& z : kft_zero_spans(P.lay)) NRS_HIP(c, hipMemsetAsync(base + z.off, 0, z.bytes, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    return NRS_OK;
}

// the dynamic-LDS limits of the sweep's kernels: per device, so once per context
static int kft_kernel_attributes(nrs_ctx* c) {
    if (c->kft_attr_done) return NRS_OK;
    NRS_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_kft_panel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)KFT_PANEL_LDS));
    NRS_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_kft_step<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)KFT_STEP_LDS));
    NRS_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_kft_step<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)KFT_STEP_LDS));
    NRS_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_kft_step<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)KFT_STEP_LDS));
    c->kft_attr_done = true;
    return NRS_OK;
}

// the device's view of the buffer
static void kft_dev_view(const KftIn& in, const KftPrep& P, char* base, KftDev& F) {
    const KftLayout& L = P.lay;
    const size_t ld = (size_t)P.dim.ld, n2 = ld * ld;
    memset(&F, 0, sizeof(F));
    F.K = in.K; F.ld = P.dim.ld; F.nb = P.dim.nb; F.m = in.K / 2; F.nfm = P.dim.nfm;
    F.k_lo = P.sd.k_lo; F.k_hi = P.sd.k_hi; F.row0 = P.sd.own_lo;
    // (A, z and xs are addressed by the GLOBAL keyframe index: the pointers are biased by the first block / vector held)
    F.A = L.at<double>(base, KR_A) - (size_t)P.sd.k_lo * n2; F.YT = L.at<double>(base, KR_YT);
    F.Bb = L.at<double>(base, KR_Bb); F.Cb = L.at<double>(base, KR_Cb); F.Pv = L.at<double>(base, KR_Pv);
    F.z = L.at<double>(base, KR_z) - (size_t)P.sd.zlo * ld; F.xs = L.at<double>(base, KR_xs) - (size_t)P.sd.zlo * ld; F.vb = L.at<double>(base, KR_vb);
    F.kf_nf = L.at<const int>(base, KR_kf_nf); F.kf_np = L.at<const int>(base, KR_kf_np);
    F.kf_row = L.at<const int>(base, KR_kf_row); F.row_ci = L.at<const int>(base, KR_row_ci);
    F.n_pp = (int)P.pairs.pp_id.size(); F.pp_id = L.at<const uint32_t>(base, KR_pp_id); F.pp_ptr = L.at<const int>(base, KR_pp_ptr);
    F.pe_src = L.at<const uint32_t>(base, KR_pe_src); F.pe_w = L.at<const double>(base, KR_pe_w);
    F.n_tp = (int)P.cpl.tp_key.size(); F.tp_ptr = L.at<const int>(base, KR_tp_ptr); F.te_src = L.at<const uint32_t>(base, KR_te_src);
    F.tp_val = L.at<double>(base, KR_tp_val);
    for (int dir = 0; dir < 2; ++dir) {
        F.cl_ptr[dir] = L.at<const int>(base, KR_cl_ptr0 + dir); F.cl_from[dir] = L.at<const int>(base, KR_cl_from0 + dir);
        F.cl_tp[dir] = L.at<const int>(base, KR_cl_tp0 + dir); F.cl_val[dir] = L.at<double>(base, KR_cl_val0 + dir);
    }
    F.bd_val = L.at<const double>(base, KR_bd_buf) + P.ed.bd_slot.size();
}

// ... and the host's
static void kft_host_view(const KftIn& in, const KftPrep& P, char* base, KftHost& H) {
    const KftLayout& L = P.lay;
    H.bytes = L.total;
    H.factor_bytes = L.off[KR_Bb] - L.off[KR_A];                   // (what was carved for the blocks and the two operands)
    H.kf_nb.resize(in.K);
    for (int k = 0; k < in.K; ++k) H.kf_nb[k] = std::max(1, (3 * P.num.kf_nf[k] + P.num.kf_np[k] + KFT_B - 1) / KFT_B);
    H.kf_nf = P.num.kf_nf;
    H.rows_own = P.sd.own_hi - P.sd.own_lo;
    H.sh = in.sh;
    H.kb = P.kb;
    H.r_m = kft_owner(in.kb, in.K / 2);
    H.handovers = in.sh ? in.world - 1 : 0;                        // (every rank boundary is crossed by one chain, once)
    H.n_bd = (int)P.ed.bd_slot.size();
    H.bd_slot = L.at<const int>(base, KR_bd_slot);
    H.bd_buf = L.at<double>(base, KR_bd_buf);
    H.pose_ws = in.sh ? L.at<double>(base, KR_pose_ws) : nullptr;
    H.rn = L.at<double>(base, KR_rn);
    H.on = true;
}

// ---- set-up (once per window): the stages in order.  A window that is not eligible -- whatever the reason -- and a rank that cannot hold
// its share both leave e->kft unset: the PCG stays block-Jacobi
static int kft_setup(nrs_ctx* c, Engine* e, const EngineSpec& s, const std::vector<int>& pose_grp_ptr) {
    StageTimer mark{c, "kft_setup", false};
    KftPrep P;
    const KftIn in = kft_in(c, e, s, pose_grp_ptr, P.kb);
    if (kft_window_reason(in) != KFT_ELIGIBLE) return NRS_OK;
    kft_number_rows(in, P.num);
    if (kft_limits(in, P.num.nf_max, P.dim) != KFT_ELIGIBLE) return NRS_OK;
    P.sd = kft_shard(in);
    bool fits = kft_factor_fits(P.sd.k_hi - P.sd.k_lo, P.dim.ld);
    kft_rows_of_nodes(in, P.dim.nfm, P.num);
    kft_vertex_table(in, P.num);
    if (kft_edges_reason(in, P.num) != KFT_ELIGIBLE) return NRS_OK;
    kft_edge_entries(in, P.num, P.sd, P.ed);
    // every check above is taken on the whole window, alike on every rank; what follows (memory, list sizes) is this rank's own.  Sharded,
    // a rank that cannot hold its share leaves e->kft unset, and engine_kft_agree -- after the upload's agreement -- drops the
    // factorisation on every rank (no collective here: a peer's set-up may have failed before this point)
    e->kft_wanted = in.sh;
    mark("edge entries");
    kft_index_by_keyframe(in, P.ed.pe, P.ix);
    kft_pair_lists(in, P.num, P.sd, P.ix, P.kl, [](int nt, auto&& fn) { parallel_for(nt, fn); });
    mark("pair lists");
    if (!kft_concat_pairs(P.kl, P.pairs)) fits = false;
    kft_coupling_pairs(P.ed.te, P.cpl);
    for (int dir = 0; dir < 2; ++dir) kft_coupling_lists(P.cpl, in.K, P.dim.nfm, dir, P.cpl.cl_ptr[dir], P.cpl.cl_from[dir], P.cpl.cl_tp[dir]);
    mark("coupling lists");
    P.lay = kft_layout(in, P.sd, P.dim, P.pairs, P.cpl, P.ed.bd_slot.size());
    if (fits && c->ensure(c->dba_kft, P.lay.total) != NRS_OK) {    // (no memory for the factor: block-Jacobi PCG, without a stale error behind)
        (void)hipGetLastError();
        c->err[0] = 0;
        fits = false;
    }
    if (!fits) { c->dba_kft.reset(); return NRS_OK; }
    mark("device buffer");
    char* base = c->dba_kft.as<char>();
    NRS_TRY(kft_upload(c, P, base));
    mark("uploads");
    std::unique_ptr<KftHost> H(new (std::nothrow) KftHost());
    if (!H) return c->fail(NRS_ERR_ALLOC, "out of host memory");
    kft_dev_view(in, P, base, H->d);
    NRS_TRY(kft_kernel_attributes(c));
    kft_host_view(in, P, base, *H);
    e->kft = H.release();
    return NRS_OK;
}

// Sharded windows: the window-wide checks of kft_setup chose the factorisation alike on every rank (kft_wanted), but a rank may not
// hold its share (memory, list sizes).  Called by every rank once the upload's own agreement has succeeded: one all-reduced flag, and
// the factorisation stays on every rank or on none -- every rank then calls the same collectives in the solve.
int engine_kft_agree(nrs_ctx* c, Engine* e) {
    if (!e || !e->kft_wanted || !c->comm || c->comm->world == 1) return NRS_OK;
    NRS_TRY(c->ensure(c->comm_flag, 2 * sizeof(double)));        // (already there: the upload's agreement used it)
    double* d = c->comm_flag.as<double>();
    double flag = e->kft && e->kft->on ? 0.0 : 1.0, sum = 0.0;
    NRS_HIP(c, hipMemcpyAsync(d, &flag, sizeof(double), hipMemcpyHostToDevice, c->stream));
    NRS_TRY(c->comm->allreduce(c, d, d + 1, 1));
    NRS_HIP(c, hipMemcpyAsync(&sum, d + 1, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    if (sum != 0.0) {                                              // some rank cannot hold its share: block-Jacobi PCG everywhere
        delete e->kft;
        e->kft = nullptr;
        c->dba_kft.reset();
    }
    return NRS_OK;
}

}  // namespace nrs
