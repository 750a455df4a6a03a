// Probes of the engine's launch path (included by nrs_engine_launch.hpp).  The solver's functions hold one line per probe:
// NRS_PROBE(...) hooks, which vanish from the product build (make PROBES=1 compiles them in), and the call of check_fused_launch
// (NRS_CHECK_FUSED, always compiled: tools/flake_probe.py runs it on the product build).
#pragma once

#ifdef NRS_DEBUG_PROBES
#define NRS_PROBE(...) __VA_ARGS__
#else
#define NRS_PROBE(...)
#endif

namespace nrs {

#ifdef NRS_DEBUG_PROBES
// Phase clocks of ONE launch (100 MHz wall clock): the kernel's waves / tiles stamp Dev::dbg_clk, 8 words per record; the constructor
// hands a zeroed buffer to a Dev copy, the destructor waits for the stream and prints the mean length of each phase
struct PhaseClocks {
    nrs_ctx* c; DevBuf mem; long long* buf = nullptr; size_t n_rec;
    const char *kernel, *unit;                                     // the printed line's kernel name and what a record is ("wave", "tile")
    std::vector<const char*> phases;                               // record words k .. k + 1 bound phase k
    // (on: the probe's condition; the buffer goes to d, a Dev copy of the launch to be timed)
    PhaseClocks(nrs_ctx* c_, bool on, Dev& d, size_t n_rec_, const char* kernel_, const char* unit_, std::vector<const char*> phases_)
        : c(c_), n_rec(n_rec_), kernel(kernel_), unit(unit_), phases(std::move(phases_)) {
        if (!on || c->ensure(mem, sizeof(long long) * 8 * n_rec) != NRS_OK) return;
        buf = mem.as<long long>();
        (void)hipMemsetAsync(buf, 0, sizeof(long long) * 8 * n_rec, c->stream);
        d.dbg_clk = buf;
    }
    PhaseClocks(const PhaseClocks&) = delete;
    ~PhaseClocks() {
        if (!buf) return;
        (void)hipStreamSynchronize(c->stream);
        std::vector<long long> h(8 * n_rec);
        (void)hipMemcpy(h.data(), buf, sizeof(long long) * 8 * n_rec, hipMemcpyDeviceToHost);
        mem.reset();
        const size_t np = phases.size();
        std::vector<double> acc(np, 0.0);
        long long t_min = LLONG_MAX, t_max = 0;
        size_t n = 0;
        for (size_t i = 0; i < n_rec; ++i) {
            const long long* q = &h[8 * i];
            if (!q[0] || !q[np]) continue;
            for (size_t k = 0; k < np; ++k) acc[k] += (double)(q[k + 1] - q[k]);
            t_min = std::min(t_min, q[0]); t_max = std::max(t_max, q[np]);
            ++n;
        }
        if (!n) return;
        fprintf(stderr, "[nrs] %s phases (us per %s, mean over %zu %ss):", kernel, unit, n, unit);
        for (size_t k = 0; k < np; ++k) fprintf(stderr, " %s %.2f", phases[k], acc[k] / n / 100.0);
        fprintf(stderr, " | launch span %.1f us\n", (double)(t_max - t_min) / 100.0);
    }
};

// NRS_SPMV_DBG=1: one operator launch (compact headers, PCG iteration 3), per wave
static bool spmv_clocks_wanted(nrs_ctx* c, const Dev& d, int it) {
    static bool done = false;
    if (!(d.h4 && it == 3 && !done && c->dbg.is_set(SW_SPMV_DBG))) return false;
    return done = true;
}

// NRS_LIN_DBG=1: one extra lineariser launch of a plain window (idempotent), per wave: where a wave's time goes
template <bool LIN>
static int lin_clocks_once(nrs_ctx* c, const Dev& d, const double* xl) {
    static bool done = false;
    if (!LIN || !d.plain || !c->dbg.is_set(SW_LIN_DBG) || done) return NRS_OK;
    done = true;
    Dev dd = d;
    PhaseClocks p(c, true, dd, (size_t)d.n_rows / (64 / d.T), "k_lin_plain", "wave", {"stage", "springs", "dampers", "reproj", "tail"});
    if (!p.buf) return c->fail(NRS_ERR_ALLOC, "%s: no memory for the phase clocks", SWITCHES[SW_LIN_DBG].name);
    return launch_reg<LIN>(c, dd, xl);
}

// NRS_PCG_DBG=1: fused iteration 20 of a problem with the coarse level, per tile; the timed launch is the real one of the iteration
// (returns whether it went out)
static bool pcg_clocks_once(nrs_ctx* c, const Dev& d, double lam, int it, double tol2, double peek_tol2, int pub) {
    static bool done = false;
    if (!(d.fused && it == 20 && d.coarse && c->dbg.is_set(SW_PCG_DBG)) || done) return false;
    done = true;
    Dev dd = d;
    PhaseClocks p(c, true, dd, (size_t)d.n_regblk, "k_pcg_fused<8,true>", "tile",
                  {"loads+pose", "coarse products", "scalars+corrections", "update+stage", "operator", "reduce+store"});
    if (!p.buf) return false;
    const size_t shm = sizeof(double) * (6 * (size_t)(d.tile_rows + d.max_halo) + 12 * (size_t)d.n_regblk + 16 * CO_MAX);
    (void)hipStreamSynchronize(c->stream);
    hipLaunchKernelGGL((k_pcg_fused<8, true>), dim3(((d.n_regblk + 7) / 8) * 8), dim3(BLK), shm, c->stream, dd, lam, it, tol2, peek_tol2, pub);
    return true;
}

// NRS_LIN_EXP=<n>: timing experiments on the lanes = 2 pinhole lineariser (wrong results for 1..5): a piece of the pass removed
static KLin lin_exp_kernel(nrs_ctx* c, const Dev& d) {
    if (!(d.cam.model == 0 && d.tp_ok && c->dbg.is_set(SW_LIN_EXP))) return nullptr;
    switch (c->dbg.int_of(SW_LIN_EXP)) {
        case 1: return k_lin_plain<2, 4, 0, true, 1>;
        case 2: return k_lin_plain<2, 4, 0, true, 2>;
        case 3: return k_lin_plain<2, 4, 0, true, 3>;
        case 4: return k_lin_plain<2, 4, 0, true, 4>;
        // round 5 (4-byte damper headers throughout; 6..9 compute right results): 5 half the damper slots,
        // 6 non-temporal streams, 7 two waves per SIMD with 8-slot batches, 8 the same with 10, 9 three waves with 6
        case 5: return k_lin_plain<2, 4, 0, true, 5, true>;
        case 6: return k_lin_plain<2, 4, 0, true, 0, true, false, false, 4, true>;
        case 7: return k_lin_plain<2, 2, 0, true, 0, true, false, false, 8>;
        case 8: return k_lin_plain<2, 2, 0, true, 0, true, false, false, 10>;
        case 9: return k_lin_plain<2, 3, 0, true, 0, true, false, false, 6>;
        case 10: return k_lin_plain<2, 2, 0, true, 0, true, false, false, 8, true>;
        default: return k_lin_plain<2, 4, 0, true, 0, true>;
    }
}
#endif  // NRS_DEBUG_PROBES

// NRS_CHECK_FUSED=1 (tools/flake_probe.py: run-to-run variation of the single-launch iteration): the fused launch of an iteration goes
// out twice from the same state and must leave the same bits in every array it writes
static int check_fused_launch(nrs_ctx* c, const Dev& d, dim3 g, size_t shm, double lam, int it, double tol2, double peek_tol2, int pub) {
    const dim3 bb(BLK);
    struct Arr { void* p; size_t bytes; const char* name; };
    const size_t nv = sizeof(double) * 3 * (size_t)d.n_rows, np6 = sizeof(double) * 6 * (size_t)d.K, npart = sizeof(double) * NPART * (size_t)d.n_regblk;
    const Arr arr[] = {{d.rv, nv, "r0"}, {d.rv2, nv, "r1"}, {d.sv, nv, "s0"}, {d.sv2, nv, "s1"}, {d.wv, nv, "w0"}, {d.wv2, nv, "w1"}, {d.xv, nv, "x"},
                       {d.pv, nv, "p"}, {d.uv3, nv, "u"}, {d.rp, np6, "rp0"}, {d.rp2, np6, "rp1"}, {d.sp, np6, "sp0"}, {d.sp2, np6, "sp1"},
                       {d.up, np6, "up0"}, {d.up2, np6, "up1"}, {d.pp, np6, "pp"}, {d.xp, np6, "xp"}, {d.part_spmv, npart, "part0"},
                       {d.part_spmv2, npart, "part1"}, {d.scal, sizeof(double) * SC_N, "scal"}, {d.flags, sizeof(int) * 8, "flags"}};
    size_t total = 0;
    for (const Arr& a : arr) total += (a.bytes + 255) & ~(size_t)255;
    NRS_TRY(c->ensure(c->fused_snap, total));                      // (kept in the context: an owner with static storage would free after the runtime is gone)
    char* snap = c->fused_snap.as<char>();
    std::vector<char> h1(total), h2(total);
    auto gather = [&](char* dst, hipMemcpyKind kind) -> int {
        size_t o = 0;
        for (const Arr& a : arr) { NRS_HIP(c, hipMemcpyAsync(dst + o, a.p, a.bytes, kind, c->stream)); o += (a.bytes + 255) & ~(size_t)255; }
        NRS_HIP(c, hipStreamSynchronize(c->stream));
        return NRS_OK;
    };
    NRS_TRY(gather(snap, hipMemcpyDeviceToDevice));
    hipLaunchKernelGGL((k_pcg_fused<8, false>), g, bb, shm, c->stream, d, lam, it, tol2, peek_tol2, pub);
    NRS_TRY(gather(h1.data(), hipMemcpyDeviceToHost));
    { size_t o = 0; for (const Arr& a : arr) { NRS_HIP(c, hipMemcpyAsync(a.p, snap + o, a.bytes, hipMemcpyDeviceToDevice, c->stream)); o += (a.bytes + 255) & ~(size_t)255; } }
    hipLaunchKernelGGL((k_pcg_fused<8, false>), g, bb, shm, c->stream, d, lam, it, tol2, peek_tol2, pub);
    NRS_TRY(gather(h2.data(), hipMemcpyDeviceToHost));
    size_t o = 0;
    bool any = false;
    for (const Arr& a : arr) {
        if (memcmp(h1.data() + o, h2.data() + o, a.bytes) != 0) {
            any = true;
            const size_t nel = a.bytes / 8;
            size_t ndiff = 0, first = 0, last = 0;
            for (size_t el = 0; el < nel; ++el)
                if (memcmp(h1.data() + o + 8 * el, h2.data() + o + 8 * el, 8) != 0) { if (!ndiff) first = el; last = el; ++ndiff; }
            double v1, v2; memcpy(&v1, h1.data() + o + 8 * first, 8); memcpy(&v2, h2.data() + o + 8 * first, 8);
            fprintf(stderr, "[nrs] fused launch it %d: array %s differs in %zu elements, first %zu (tile %zu) last %zu (tile %zu): %.6g / %.6g\n", it, a.name, ndiff, first,
                    first / 3 / (size_t)d.tile_rows, last, last / 3 / (size_t)d.tile_rows, v1, v2);
        }
        o += (a.bytes + 255) & ~(size_t)255;
    }
    if (any) {
        const size_t o_fl = total - 256, o_sc = o_fl - ((sizeof(double) * SC_N + 255) & ~(size_t)255);
        const int* f1 = reinterpret_cast<const int*>(h1.data() + o_fl); const int* f2 = reinterpret_cast<const int*>(h2.data() + o_fl);
        const double* s1 = reinterpret_cast<const double*>(h1.data() + o_sc); const double* s2 = reinterpret_cast<const double*>(h2.data() + o_sc);
        fprintf(stderr, "[nrs]    flags after run 1: %d %d %d %d | run 2: %d %d %d %d ; scal gamma0 %.6g/%.6g slot0 %.6g %.6g / %.6g %.6g slot1 %.6g %.6g / %.6g %.6g\n", f1[0], f1[1], f1[2], f1[3], f2[0], f2[1], f2[2], f2[3],
                s1[SC_GAMMA0], s2[SC_GAMMA0], s1[SC_SLOT0], s1[SC_SLOT0 + 1], s2[SC_SLOT0], s2[SC_SLOT0 + 1], s1[SC_SLOT1], s1[SC_SLOT1 + 1], s2[SC_SLOT1], s2[SC_SLOT1 + 1]);
    }
    return NRS_OK;
}

}  // namespace nrs
