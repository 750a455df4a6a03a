// The direct solver on its own (include/nrs.h nrs_debug_nd_solve): a plan from the caller's pairs, the caller's blocks as entry values,
// one factorise + solve, optionally timed, optionally with the kernels' phase clocks.  Part of nrs_engine.hip (one translation unit).
#pragma once
#include "nrs_nd_solver.hpp"

namespace nrs {
void nd_orient_pairs(const NdPlan& P, const int32_t* pairs, const double* Vp, std::vector<double>& out);   // nrs_host_build.cpp
void nd_stats(const NdPlan& P, int64_t* stats);

// NRS_ND_DBG: the phase clocks of one solve (8 per workgroup of the factorisation, then per front of the back pass; 100 MHz) as
// mean / max over the workgroups of every launch
static void nd_debug_report_clocks(nrs_ctx* c, const NdPlan& P, const std::vector<long long>& h) {
    const long long t00 = h[0];
    for (int l = 0; l < P.n_levels; ++l) {
        double mean[5] = {0, 0, 0, 0, 0}, mx[5] = {0, 0, 0, 0, 0}, mA = 0, mB = 0;
        long long lo = LLONG_MAX, hi = 0;
        const int a = P.lvl_wg_ptr[l], b2 = P.lvl_wg_ptr[l + 1];
        for (int w = a; w < b2; ++w) {
            const long long* q = &h[8 * (size_t)w];
            mA += (double)q[6] / 100.0 / (b2 - a); mB += (double)q[7] / 100.0 / (b2 - a);
            for (int k = 0; k < 5; ++k) { const double d = (double)(q[k + 1] - q[k]) / 100.0; mean[k] += d / (b2 - a); mx[k] = std::max(mx[k], d); }
            lo = std::min(lo, q[0]); hi = std::max(hi, q[5]);
        }
        fprintf(stderr, "[nrs] nd level %2d: %4d wg, span %6.1f us (from %7.1f) | mean / max us: entries %.1f/%.1f gather %.1f/%.1f factor %.1f/%.1f (A %.1f B %.1f) schur %.1f/%.1f store %.1f/%.1f\n", l, b2 - a,
                (double)(hi - lo) / 100.0, (double)(lo - t00) / 100.0, mean[0], mx[0], mean[1], mx[1], mean[2], mx[2], mA, mB, mean[3], mx[3], mean[4], mx[4]);
    }
    for (int l = P.n_levels - 1; l >= 0; --l) {
        double mean[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
        long long lo = LLONG_MAX, hi = 0;
        const int a = P.lvl_ptr[l], b2 = P.lvl_ptr[l + 1];
        for (int w = a; w < b2; ++w) {
            const long long* q = &h[8 * (P.wg.size() / 3 + (size_t)w)];
            if (q[3] == 0) continue;                            // (a root)
            if (b2 - a <= 2 && c->dbg.is_set(SW_ND_DBG2)) fprintf(stderr, "   front %d (s %d b %d nseg %d): start %.1f seg-loop-begin %.1f released %.1f gathered %.1f gemv %.1f end %.1f\n", w, P.fr[P.lvl_fronts[w]].s, P.fr[P.lvl_fronts[w]].b, P.fr[P.lvl_fronts[w]].n_seg, (q[0]-t00)/100.0, (q[5]-t00)/100.0, (q[4]-t00)/100.0, (q[1]-t00)/100.0, (q[2]-t00)/100.0, (q[3]-t00)/100.0);
            // (single launch: [4] = released by the parent; "loads" is then the gather of the boundary values only)
            for (int k = 0; k < 3; ++k) { const double d = (double)(q[k + 1] - (k == 0 && q[4] ? q[4] : q[k])) / 100.0; mean[k] += d / (b2 - a); mx[k] = std::max(mx[k], d); }
            lo = std::min(lo, q[4] ? q[4] : q[0]); hi = std::max(hi, q[3]);
        }
        if (hi == 0) continue;
        fprintf(stderr, "[nrs] nd back  %2d: %4d wg, span %6.1f us (from %7.1f) | mean / max us: loads %.1f/%.1f gemv %.1f/%.1f solve %.1f/%.1f\n", l, b2 - a,
                (double)(hi - lo) / 100.0, (double)(lo - t00) / 100.0, mean[0], mx[0], mean[1], mx[1], mean[2], mx[2]);
    }
}
// ... taken from one more solve, every level in a launch of its own
static int nd_debug_phase_clocks(nrs_ctx* c, NdSolver& S, double lam) {
    const size_t nw = S.plan.wg.size() / 3 + (size_t)S.plan.n_fronts;
    DevBuf buf;
    NRS_TRY(c->ensure(buf, sizeof(long long) * 8 * nw));
    long long* clk = buf.as<long long>();
    NRS_HIP(c, hipMemsetAsync(clk, 0, sizeof(long long) * 8 * nw, c->stream));
    S.dev.clk = clk;
    NRS_TRY(nd_solve_enqueue(c, S, lam));
    S.dev.clk = nullptr;
    std::vector<long long> h(8 * nw);
    NRS_HIP(c, hipMemcpyAsync(h.data(), clk, sizeof(long long) * 8 * nw, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    buf.reset();
    nd_debug_report_clocks(c, S.plan, h);
    return NRS_OK;
}

// include/nrs.h nrs_debug_nd_solve
int engine_nd_debug_solve(nrs_ctx* c, int n_nodes, const double* pos, const uint8_t* last, int n_pairs, const int* pairs, const double* Dn, const double* Vp,
                          const double* bn, double lam, int repeats, double* x, int64_t* stats, double* ms_per_solve) {
    NRS_HIP(c, hipSetDevice(c->device));
    NdSolver S;
    std::string err;
    if (!nd_build_plan(n_nodes, pos, last, n_pairs, pairs, S.plan, &err, nd_leaf_n(c), ND_SMAXN, true, 0, !c->dbg.is_set(SW_ND_NO_COVER))) return c->fail(NRS_ERR_INVALID, "direct solve: %s", err.c_str());
    nd_stats(S.plan, stats);
    struct Sync { nrs_ctx* c; ~Sync() { (void)hipStreamSynchronize(c->stream); } } sync{c};   // (S.own is freed right after it, when S goes)
    NRS_TRY(nd_upload(c, S));
    std::vector<double> V, ev(9 * S.plan.ent.size(), 0.0);
    nd_orient_pairs(S.plan, pairs, Vp, V);
    for (size_t e = 0; e < S.plan.ent.size(); ++e) {                // the blocks in entry order (what k_nd_values writes for an engine)
        const uint32_t kind = S.plan.ent[e].src >> ND_KIND_SHIFT, src = S.plan.ent[e].src & ND_SRC_MASK;
        const double* v = kind == 0 ? Dn + 9 * (size_t)src : kind == 1 ? V.data() + 9 * (size_t)src : bn + 3 * (size_t)src;
        for (int a = 0; a < (kind == 2 ? 3 : 9); ++a) ev[9 * e + a] = v[a];
    }
    NRS_HIP(c, hipMemcpyAsync(S.d_ev, ev.data(), 8 * ev.size(), hipMemcpyHostToDevice, c->stream));
    NRS_TRY(nd_solve_enqueue(c, S, lam));                          // (warm-up and the result)
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    if (repeats > 0) {
        NRS_HIP(c, hipEventRecord(c->ev0.get(), c->stream));
        for (int r = 0; r < repeats; ++r) NRS_TRY(nd_solve_enqueue(c, S, lam));
        NRS_HIP(c, hipEventRecord(c->ev1.get(), c->stream));
        NRS_HIP(c, hipEventSynchronize(c->ev1.get()));
        float ms = 0;
        NRS_HIP(c, hipEventElapsedTime(&ms, c->ev0.get(), c->ev1.get()));
        if (ms_per_solve) *ms_per_solve = ms / repeats;
    }
    if (c->dbg.is_set(SW_ND_DBG)) NRS_TRY(nd_debug_phase_clocks(c, S, lam));
    int fl[4] = {0, 0, 0, 0};
    NRS_HIP(c, hipMemcpyAsync(fl, S.dev.flags, sizeof(fl), hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(x, S.dev.xn, 24 * (size_t)n_nodes, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    if (!fl[0]) return c->fail(NRS_ERR_HIP, "direct solve: the last level did not report completion");
    if (fl[2] == 2) return c->fail(NRS_ERR_HIP, "direct solve: a wait for another workgroup's result timed out");
    return fl[2] ? c->fail(NRS_ERR_NUMERIC, "direct solve: the matrix is not positive definite") : NRS_OK;
}

}  // namespace nrs
