// Kernel-variant dispatch of the engine (included into nrs_engine.hip): every launcher states its condition -> template-argument
// mapping once.  The runtime lane count (Dev::T, written by lanes_per_row / dev_init only: 1, 2, 4, 8 or 16) becomes a compile-time constant
// through with_lanes; variants that exist for one lane count only sit behind `if constexpr`: nothing is instantiated that is not launched.
#pragma once
#include <type_traits>

namespace nrs {

// HIP-event timing when profiling is on.  An event pair around ONE launch of a 20 us kernel reads 4-5 us high (the gaps
// between the events and the kernel); the two kernels the roofline lines are about -- both idempotent: they read the state
// and write factors / products -- are therefore launched PROFILE_REPS times back to back inside one pair and the time is
// divided, which is also how the operator runs in the solve (launch after launch) and what the rocprofv3 trace shows.
constexpr int PROFILE_REPS = 4;
struct Timer {
    nrs_ctx* c; double* acc; int64_t* cnt; int reps;
    Timer(nrs_ctx* c_, double* a, int64_t* n, int reps_ = 1) : c(c_), acc(a), cnt(n), reps(reps_) { if (c->opt.profile) (void)hipEventRecord(c->ev0.get(), c->stream); }
    ~Timer() {
        if (!c->opt.profile) return;
        (void)hipEventRecord(c->ev1.get(), c->stream);
        (void)hipEventSynchronize(c->ev1.get());
        float ms = 0;
        (void)hipEventElapsedTime(&ms, c->ev0.get(), c->ev1.get());
        *acc += ms / reps;
        *cnt += 1;
    }
};

// f(std::integral_constant<int, T>) for the engine's lane count
template <class F>
static int with_lanes(nrs_ctx* c, int T, F&& f) {
    switch (T) {
        case 1: f(std::integral_constant<int, 1>{}); return NRS_OK;
        case 2: f(std::integral_constant<int, 2>{}); return NRS_OK;
        case 4: f(std::integral_constant<int, 4>{}); return NRS_OK;
        case 8: f(std::integral_constant<int, 8>{}); return NRS_OK;
        case 16: f(std::integral_constant<int, 16>{}); return NRS_OK;
    }
    return c->fail(NRS_ERR_STATE, "no kernels for %d lanes per row", T);
}

using KLin = void (*)(Dev, const double*, int);                    // k_reg / k_lin_plain
using KOp = void (*)(Dev, double, int, int, double);               // k_spmv_f

template <bool LIN> static int launch_reg(nrs_ctx* c, const Dev& d, const double* xl);
}  // namespace nrs

#include "nrs_engine_probes.hpp"

namespace nrs {

// the lineariser of a plain BA window at lanes = 2 (the two-kernel path's default), camera model CAM: temporal partners by row
// (tp), 4-byte damper headers (h4: implies tp) and on those the factors the operator re-forms instead (rc) or non-temporal streams (nt)
template <int CAM>
static KLin lin_plain2_kernel(const Dev& d, int cls) {
    if (!d.h4) return d.tp_ok ? k_lin_plain<2, 4, CAM, true> : k_lin_plain<2, 4, CAM, false>;
    switch (rc_of(d, cls)) {                                       // (the operator re-forms the factors: nothing stored per incidence)
        case 0: break;
        case 1: return k_lin_plain<2, 4, CAM, true, 0, true, true, false>;
        case 2: return k_lin_plain<2, 4, CAM, true, 0, true, false, true>;
        default: return k_lin_plain<2, 4, CAM, true, 0, true, true, true>;
    }
    if (d.nt) return k_lin_plain<2, 4, CAM, true, 0, true, false, false, 4, true>;   // (streams beyond the Infinity Cache: non-temporal accesses)
    return k_lin_plain<2, 4, CAM, true, 0, true>;
}

template <int T>
static KLin lin_plain_kernel(nrs_ctx* c, const Dev& d, int cls) {
    NRS_PROBE(if constexpr (T == 2) if (KLin k = lin_exp_kernel(c, d)) return k;)
    if constexpr (T == 2) return d.cam.model == 0 ? lin_plain2_kernel<0>(d, cls) : lin_plain2_kernel<1>(d, cls);
    else if constexpr (T == 8) return d.tp_ok ? k_lin_plain<8, 4, -1, true> : k_lin_plain<8>;
    else return k_lin_plain<T>;
}

template <bool LIN, bool LDS>
static int launch_reg2(nrs_ctx* c, const Dev& d, const double* xl, size_t shm, int n, int cls) {
    KLin k = nullptr;
    NRS_TRY(with_lanes(c, d.T, [&](auto L) {
        constexpr int T = decltype(L)::value;
        if constexpr (LIN && LDS) {
            if (d.plain) { k = lin_plain_kernel<T>(c, d, cls); return; }            // plain BA window: the specialised pass
            if (d.dform) { k = k_reg<T, true, true, true>; return; }                // temporal-difference dampers (two-kernel path: T = 2 unless overridden)
        }
        k = k_reg<T, LIN, LDS>;
    }));
    hipLaunchKernelGGL(k, dim3(((n + 7) / 8) * 8), dim3(BLK), shm, c->stream, d, xl, cls);
    return NRS_OK;
}

template <bool LIN>
static int launch_reg(nrs_ctx* c, const Dev& d, const double* xl) {
    if (!d.use_lds) return launch_reg2<LIN, false>(c, d, xl, 0, d.n_regblk, 0);
    for (int cls = 0; cls < 2; ++cls) {
        if (d.sh_nt[cls] == 0) continue;
        size_t shm = (LIN && d.dform) ? sizeof(double) * 9 * (size_t)(d.tile_rows + d.cap_h[cls] + 1)
                                      : sizeof(double) * 3 * (size_t)(d.tile_rows + d.cap_h[cls]) * (d.X0 ? 2 : 1);
        if (LIN) shm = std::max(shm, sizeof(double) * 4 * 64 * 8);        // the pose-block product reuses the staging area: 4 KB per wave
        NRS_TRY((launch_reg2<LIN, true>(c, d, xl, shm, d.sh_nt[cls], cls)));   // (LIN: the linearisation point is d.lin_pose / xl)
    }
    return NRS_OK;
}

// the stored-block operator of the gather fallback
static int launch_spmv_gather(nrs_ctx* c, const Dev& d, double lam, int it) {
    return with_lanes(c, d.T, [&](auto L) { hipLaunchKernelGGL((k_spmv<decltype(L)::value, false>), dim3(((d.n_regblk + 7) / 8) * 8), dim3(BLK), 0, c->stream, d, lam, it); });
}

// the factored operator: temporal-difference dampers, or at lanes = 2 on a plain window the forms that go with the lineariser's
// (lin_plain2_kernel), or the generic one
template <int T>
static KOp spmv_f_kernel(const Dev& d, int cls) {
    if (d.dform) return k_spmv_f<T, true>;
    if constexpr (T == 2) {
        if (d.plain && d.tp_ok) {
            if (!d.h4) return k_spmv_f<2, false, true>;
            switch (rc_of(d, cls)) {
                case 0: break;
                case 1: return k_spmv_f<2, false, true, true, true, false>;
                case 2: return k_spmv_f<2, false, true, true, false, true>;
                default: return k_spmv_f<2, false, true, true, true, true>;
            }
            return d.nt ? k_spmv_f<2, false, true, true, false, false, true> : k_spmv_f<2, false, true, true>;
        }
    }
    return k_spmv_f<T, false>;
}

// with_skin_op (embedded BA window): k_skin_op's workgroups ride behind the operator's in the same launch (k_spmv_f_skin) where the
// operator is the generic k_spmv_f<T, false>; *merged tells whether they did (the caller launches k_skin_op on its own otherwise)
static int launch_spmv(nrs_ctx* c, const Dev& d0, double lam, int it, double tol2, bool with_skin_op = false, bool* merged = nullptr) {
    if (merged) *merged = false;
    if (!d0.use_lds) return launch_spmv_gather(c, d0, lam, it);
    Dev d = d0;
    NRS_PROBE(PhaseClocks clocks(c, spmv_clocks_wanted(c, d, it), d, (size_t)d.n_rows / (64 / d.T), "k_spmv_f", "wave", {"stage", "springs", "dampers", "row", "reduce"});)
    for (int cls = 0; cls < 2; ++cls) {
        const int n = d.sh_nt[cls] + d.sh_ntb[cls];
        if (n == 0) continue;
        const dim3 g(((n + 7) / 8) * 8), b(BLK);
        const size_t shm = d.dform ? sizeof(double) * 3 * (3 * (size_t)(d.tile_rows + d.cap_h[cls] + 1) + d.tile_rows + d.cap_s[cls] + 1)
                                   : sizeof(double) * 3 * (size_t)(2 * d.tile_rows + d.cap_h[cls] + ((rc_of(d, cls) & 2) ? d.cap_h[cls] : d.cap_s[cls]) + 2);
        const bool last_cls = cls == 1 || d.sh_nt[1] + d.sh_ntb[1] == 0;
        if (!d.dform && with_skin_op && last_cls && !(d.T == 2 && d.plain && d.tp_ok) && !c->dbg.is_set(SW_SKIN_OP_OWN_LAUNCH)) {
            NRS_TRY(with_lanes(c, d.T, [&](auto L) { hipLaunchKernelGGL((k_spmv_f_skin<decltype(L)::value>), dim3(g.x + d.sk_nblk), b, shm, c->stream, d, lam, cls, it, tol2, (int)g.x); }));
            if (merged) *merged = true;
            continue;
        }
        NRS_TRY(with_lanes(c, d.T, [&](auto L) { hipLaunchKernelGGL(spmv_f_kernel<decltype(L)::value>(d, cls), g, b, shm, c->stream, d, lam, cls, it, tol2); }));
    }
    return NRS_OK;
}

}  // namespace nrs
