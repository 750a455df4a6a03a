// Parity tap of the keyframe-block factorisation (included at the end of nrs_engine.hip: it uses the engine's evaluation).
#pragma once

namespace nrs {

// Parity tap (include/nrs.h nrs_debug_kft): linearise at the current estimate, assemble / factorise the keyframe blocks at `lam`, then
//   what 0: info[0..6) = {on, K, ld, nb, m, factor bytes >> 20}, then nf_k, np_k per keyframe          (out_i, 6 + 2 K ints)
//   what 1: the ASSEMBLED diagonal block A_k (ld x ld, compact order: node copies by row, then the pose)  (out_d)
//   what 2: the coupling T_k as a dense ld x ld matrix (rows: keyframe k, columns: keyframe k + 1)       (out_d)
//   what 3: u = M^-1 r for r given in solver order (6 K pose entries, then 3 per vertex); u in the same order (in_d -> out_d)
//   what 4: per vertex its (keyframe, compact node) pair, -1 for a fixed vertex                          (out_i, 2 M ints)
//   what 5: this rank's share {first own keyframe, own keyframes, m, rank of m, factor KiB held, hand-overs per factorisation}  (out_i, 6)
// Sharded (a communicator): what 1 / 2 / 3 linearise and assemble, so every rank calls them together; what 1 / 2 return the block of an
// own keyframe (NRS_ERR_INVALID on the other ranks), what 3 returns the complete u on every rank.
int engine_kft_debug(nrs_ctx* c, Engine* e, double lam, int what, int k, const double* in_d, double* out_d, int32_t* out_i) {
    Dev& d = e->d;
    KftHost* H = e->kft;
    if (what == 0) {
        out_i[0] = H && H->on ? 1 : 0;
        if (!out_i[0]) return NRS_OK;
        out_i[1] = H->d.K; out_i[2] = H->d.ld; out_i[3] = H->d.nb; out_i[4] = H->d.m; out_i[5] = (int32_t)(H->bytes >> 20);
        NRS_HIP(c, hipMemcpy(out_i + 6, H->d.kf_nf, 4 * (size_t)H->d.K, hipMemcpyDeviceToHost));
        NRS_HIP(c, hipMemcpy(out_i + 6 + H->d.K, H->d.kf_np, 4 * (size_t)H->d.K, hipMemcpyDeviceToHost));
        return NRS_OK;
    }
    if (!H || !H->on) return c->fail(NRS_ERR_STATE, "no keyframe-block factorisation on this window");
    const KftDev& F = H->d;
    const size_t n2 = (size_t)F.ld * F.ld;
    if (what == 5) {
        out_i[0] = F.k_lo; out_i[1] = F.k_hi - F.k_lo; out_i[2] = F.m; out_i[3] = H->r_m;
        out_i[4] = (int32_t)(H->factor_bytes >> 10); out_i[5] = H->handovers;
        return NRS_OK;
    }
    if (what == 4) {
        std::vector<int> rc((size_t)d.n_rows);
        NRS_HIP(c, hipMemcpy(rc.data(), F.row_ci, 4 * rc.size(), hipMemcpyDeviceToHost));
        std::vector<int> gp((size_t)d.n_groups);
        NRS_HIP(c, hipMemcpy(gp.data(), d.grp_pose, 4 * gp.size(), hipMemcpyDeviceToHost));
        for (int v = 0; v < d.M; ++v) { out_i[2 * v] = gp[e->vrow[v] / ROW_ALIGN]; out_i[2 * v + 1] = rc[e->vrow[v]]; }
        return NRS_OK;
    }
    NRS_TRY(evaluate<true>(c, e, e->cur));
    NRS_TRY(wait_published(c, e->h_flags, c->seq, c->stream));
    if (what == 1 || what == 2) {
        NRS_TRY(kft_assemble(c, e, H, lam));
        NRS_HIP(c, hipStreamSynchronize(c->stream));
        if (k < F.k_lo || k >= F.k_hi) return c->fail(NRS_ERR_INVALID, "keyframe out of range (or not held by this rank)");
        if (what == 1) { NRS_HIP(c, hipMemcpy(out_d, F.A + (size_t)k * n2, 8 * n2, hipMemcpyDeviceToHost)); return NRS_OK; }
        std::vector<int> ptr((size_t)F.K * (F.nfm + 1)), from((size_t)F.n_tp + 1), tp((size_t)F.n_tp + 1);
        std::vector<double> tv((size_t)F.n_tp + 1);
        NRS_HIP(c, hipMemcpy(ptr.data(), F.cl_ptr[1], 4 * ptr.size(), hipMemcpyDeviceToHost));
        NRS_HIP(c, hipMemcpy(from.data(), F.cl_from[1], 4 * (size_t)F.n_tp, hipMemcpyDeviceToHost));
        NRS_HIP(c, hipMemcpy(tp.data(), F.cl_tp[1], 4 * (size_t)F.n_tp, hipMemcpyDeviceToHost));
        NRS_HIP(c, hipMemcpy(tv.data(), F.tp_val, 8 * (size_t)F.n_tp, hipMemcpyDeviceToHost));
        std::fill(out_d, out_d + n2, 0.0);
        for (int a = 0; a < F.nfm; ++a)                            // dir 1 at keyframe k by its node a: the nodes b of keyframe k + 1
            for (int q = ptr[(size_t)k * (F.nfm + 1) + a]; q < ptr[(size_t)k * (F.nfm + 1) + a + 1]; ++q)
                for (int cc = 0; cc < 3; ++cc) out_d[(size_t)(3 * a + cc) * F.ld + 3 * from[q] + cc] = tv[tp[q]];
        return NRS_OK;
    }
    if (what == 3) {
        NRS_HIP(c, hipMemsetAsync(d.flags, 0, sizeof(int) * 8, c->stream));
        NRS_TRY(kft_factor(c, e, H, lam));
        std::vector<double> rv(3 * (size_t)d.n_rows, 0.0);
        for (int v = 0; v < d.M; ++v) for (int a = 0; a < 3; ++a) rv[3 * (size_t)e->vrow[v] + a] = in_d[6 * (size_t)d.K + 3 * (size_t)v + a];
        const size_t o = 3 * (size_t)d.row_lo, nr = 3 * (size_t)(d.row_hi - d.row_lo);   // (the rows this engine holds: all of them on one GPU)
        NRS_HIP(c, hipMemcpyAsync(d.rv + o, rv.data() + o, 8 * nr, hipMemcpyHostToDevice, c->stream));
        NRS_HIP(c, hipMemcpyAsync(d.rp, in_d, 8 * 6 * (size_t)d.K, hipMemcpyHostToDevice, c->stream));
        NRS_HIP(c, hipMemsetAsync(d.uv3 + o, 0, 8 * nr, c->stream));
        NRS_HIP(c, hipMemsetAsync(d.up, 0, 8 * 6 * (size_t)d.K, c->stream));
        NRS_TRY(kft_apply(c, H, d.rv, d.rp, d.uv3, d.up, d.flags));
        NRS_HIP(c, hipGetLastError());
        NRS_HIP(c, hipMemcpyAsync(rv.data() + o, d.uv3 + o, 8 * nr, hipMemcpyDeviceToHost, c->stream));
        NRS_HIP(c, hipMemcpyAsync(out_d, d.up, 8 * 6 * (size_t)d.K, hipMemcpyDeviceToHost, c->stream));
        int fl[8];
        NRS_HIP(c, hipMemcpyAsync(fl, d.flags, sizeof(fl), hipMemcpyDeviceToHost, c->stream));
        NRS_HIP(c, hipStreamSynchronize(c->stream));
        for (int v = 0; v < d.M; ++v) for (int a = 0; a < 3; ++a) out_d[6 * (size_t)d.K + 3 * (size_t)v + a] = rv[3 * (size_t)e->vrow[v] + a];
        if (H->sh) {                                               // the complete u on every rank: own node copies here, the poses from rank 0, summed
            const int r_lo = F.row0, r_hi = F.row0 + H->rows_own;
            const size_t n = 6 * (size_t)d.K + 3 * (size_t)d.M;
            if (c->comm->rank != 0) std::fill(out_d, out_d + 6 * (size_t)d.K, 0.0);
            for (int v = 0; v < d.M; ++v)
                if (e->vrow[v] < r_lo || e->vrow[v] >= r_hi) for (int a = 0; a < 3; ++a) out_d[6 * (size_t)d.K + 3 * (size_t)v + a] = 0.0;
            NRS_TRY(c->ensure(c->gather_ws, 2 * sizeof(double) * n));
            double* g = c->gather_ws.as<double>();
            NRS_HIP(c, hipMemcpyAsync(g, out_d, 8 * n, hipMemcpyHostToDevice, c->stream));
            NRS_TRY(c->comm->allreduce(c, g, g + n, n));
            NRS_HIP(c, hipMemcpyAsync(out_d, g + n, 8 * n, hipMemcpyDeviceToHost, c->stream));
            NRS_HIP(c, hipStreamSynchronize(c->stream));
            c->gather_ws.reset();
            int bad = fl[2], any = 0;                              // (a pivot failure on any rank fails every rank)
            NRS_TRY(c->ensure(c->gather_ws, 2 * sizeof(double)));
            double fv = bad ? 1.0 : 0.0, fs = 0.0;
            g = c->gather_ws.as<double>();
            NRS_HIP(c, hipMemcpyAsync(g, &fv, 8, hipMemcpyHostToDevice, c->stream));
            NRS_TRY(c->comm->allreduce(c, g, g + 1, 1));
            NRS_HIP(c, hipMemcpyAsync(&fs, g + 1, 8, hipMemcpyDeviceToHost, c->stream));
            NRS_HIP(c, hipStreamSynchronize(c->stream));
            c->gather_ws.reset();
            any = fs != 0.0;
            fl[2] = any;
        }
        if (fl[2]) return c->fail(NRS_ERR_NUMERIC, "keyframe-block factorisation: a pivot that is not positive");
        return NRS_OK;
    }
    return c->fail(NRS_ERR_INVALID, "nrs_debug_kft: unknown request");
}

}  // namespace nrs
