// Embedded-deformation mode of the single-frame engine (N2; SURVEY.md 8d: "other points interpolate from <= 11 nodes with
// normalised weights"): observations of points that carry no vertex.  Part of nrs_engine.hip (one translation unit).
//
// The reference has no such edge; it is ReprojectionErrorWithDeformation (reprojection_error_with_deformation.cc:37-68: residual
// z - pi(T (X0 + delta)), fp32 projection and projection Jacobian, information 1 / 0.5^2, Huber sqrt(5.99), OPT:203-204,236) with
// delta = sum_k omega_k delta_{n_k}, the interpolation rule of the reference's own skinning (stage 2 of
// CameraPoseAndDeformationOptimization, OPT:476-553, spatial_regularizer_fixed.cc:32-43) turned into a differentiable one: the
// Jacobian with respect to node k is omega_k times the reference's 2 x 3 block.  oracle/embedded_oracle.py states the mode; with
// every point a node nothing of this file runs and the solve is the parity-mode one, bit for bit.
//
// One thread per observation: residual, Huber, and -- at a linearisation -- its three dense pieces (J_l^T w J_l, -J_l^T w r,
// J_p^T w J_l), which k_nd_values folds into the direct solver's blocks through fixed-order lists (node diagonal blocks, node-node
// pairs of every observation's node set, pose-node blocks, gradients): no atomics on values, bit-reproducible.
#pragma once

namespace nrs {


// Embedded BA windows: the skinned points at the estimate xl, one thread per slot: X0 + sum_k om_k (x_k - x_start_k) over the slot's node
// rows, k = 0 .. 10 in order with the pads skipped and no contraction -- the expression, the order and the roundings of the host loop this
// replaces.  Slot i holds observation sk_src[i] of the engine's list, which starts at `base` in the window's list of `total`; out is the
// window's vector (zeroed by the caller: observations held by other ranks stay 0 for the sum over the ranks).
__global__ __launch_bounds__(BLK) void k_skin_positions(Dev P, const double* __restrict__ xl, int base, int total, double* __restrict__ out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= P.sk_n) return;
    const int src = P.sk_src[i];
    if (src < 0 || base + src >= total) return;                    // (padding)
    double x[3] = {P.sk_X0[3 * (size_t)i], P.sk_X0[3 * (size_t)i + 1], P.sk_X0[3 * (size_t)i + 2]};
    for (int k = 0; k < SK_MAX; ++k) {
        const int row = P.sk_row[(size_t)k * P.sk_n + i];
        if (row < 0) continue;
        const double om = P.sk_om[(size_t)k * P.sk_n + i];
        for (int a2 = 0; a2 < 3; ++a2) {
            const double dx = P.sk_base ? xl[3 * (size_t)row + a2] - P.sk_base[3 * (size_t)row + a2] : xl[3 * (size_t)row + a2];
            x[a2] += om * dx;
        }
    }
    double* o = out + 3 * ((size_t)base + src);
    o[0] = x[0]; o[1] = x[1]; o[2] = x[2];
}

template <bool LIN>
__global__ __launch_bounds__(BLK) void k_skin(Dev P, const Pose* __restrict__ poses, const double* __restrict__ xl) {
    __shared__ double lds[4 * 28];
    const int tid = threadIdx.x, i = blockIdx.x * BLK + tid;
    double acc[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = 0;
    if (LIN && i == 0) *P.sk_maxdiag = 0.0;
    const int kp = P.sk_blk_pose ? P.sk_blk_pose[blockIdx.x] : 0;  // (a workgroup's observations share a pose)
    if (i < P.sk_n) {
        const Pose Tcw = poses[kp];
        double R[9];
        quat_to_R(Tcw.q, R);
        double x0 = P.sk_X0[3 * (size_t)i], x1 = P.sk_X0[3 * (size_t)i + 1], x2 = P.sk_X0[3 * (size_t)i + 2];
#pragma unroll
        for (int k = 0; k < SK_MAX; ++k) {
            const int row = P.sk_row[(size_t)k * P.sk_n + i];       // (node lists slot-major inside a k: coalesced)
            const double om = P.sk_om[(size_t)k * P.sk_n + i];
            if (row >= 0 && P.sk_base) {                           // BA form: the node's displacement from where the window started
                x0 += om * (xl[3 * (size_t)row] - P.sk_base[3 * (size_t)row]); x1 += om * (xl[3 * (size_t)row + 1] - P.sk_base[3 * (size_t)row + 1]);
                x2 += om * (xl[3 * (size_t)row + 2] - P.sk_base[3 * (size_t)row + 2]);
            } else if (row >= 0) { x0 += om * xl[3 * (size_t)row]; x1 += om * xl[3 * (size_t)row + 1]; x2 += om * xl[3 * (size_t)row + 2]; }
        }
        const double px = R[0] * x0 + R[1] * x1 + R[2] * x2 + Tcw.t[0];
        const double py = R[3] * x0 + R[4] * x1 + R[5] * x2 + Tcw.t[1];
        const double pz = R[6] * x0 + R[7] * x1 + R[8] * x2 + Tcw.t[2];
        float u, v;
        project_f32(P.cam, (float)px, (float)py, (float)pz, u, v);
        const double r0 = (double)P.sk_uv[2 * (size_t)i] - (double)u, r1 = (double)P.sk_uv[2 * (size_t)i + 1] - (double)v;
        const double e = P.info_reproj * (r0 * r0 + r1 * r1);
        P.sk_chi[i] = e;
        const bool active = P.sk_active[i] != 0;
        double rho0, rho1;
        huber(e, P.delta_reproj, rho0, rho1);
        if (active) acc[27] = rho0;
        if (LIN) {
            double* rec = P.sk_rec + 27 * (size_t)i;
            if (active) {
                float Jf[6];
                projection_jacobian_f32(P.cam, (float)px, (float)py, (float)pz, Jf);
                const double w = rho1 * P.info_reproj, pm = P.pose_fixed[kp] ? 0.0 : 1.0;
                double Jp[2][6], Jl[2][3];
#pragma unroll
                for (int rr = 0; rr < 2; ++rr) {
                    const double j0 = -(double)Jf[3 * rr], j1 = -(double)Jf[3 * rr + 1], j2 = -(double)Jf[3 * rr + 2];
                    Jp[rr][0] = pm * (-j1 * pz + j2 * py);
                    Jp[rr][1] = pm * (j0 * pz - j2 * px);
                    Jp[rr][2] = pm * (-j0 * py + j1 * px);
                    Jp[rr][3] = pm * j0; Jp[rr][4] = pm * j1; Jp[rr][5] = pm * j2;
                    Jl[rr][0] = j0 * R[0] + j1 * R[3] + j2 * R[6];
                    Jl[rr][1] = j0 * R[1] + j1 * R[4] + j2 * R[7];
                    Jl[rr][2] = j0 * R[2] + j1 * R[5] + j2 * R[8];
                }
                rec[0] = w * (Jl[0][0] * Jl[0][0] + Jl[1][0] * Jl[1][0]);
                rec[1] = w * (Jl[0][0] * Jl[0][1] + Jl[1][0] * Jl[1][1]);
                rec[2] = w * (Jl[0][0] * Jl[0][2] + Jl[1][0] * Jl[1][2]);
                rec[3] = w * (Jl[0][1] * Jl[0][1] + Jl[1][1] * Jl[1][1]);
                rec[4] = w * (Jl[0][1] * Jl[0][2] + Jl[1][1] * Jl[1][2]);
                rec[5] = w * (Jl[0][2] * Jl[0][2] + Jl[1][2] * Jl[1][2]);
#pragma unroll
                for (int c = 0; c < 3; ++c) rec[6 + c] = -w * (Jl[0][c] * r0 + Jl[1][c] * r1);
#pragma unroll
                for (int p = 0; p < 6; ++p)
#pragma unroll
                    for (int c = 0; c < 3; ++c) rec[9 + 3 * p + c] = w * (Jp[0][p] * Jl[0][c] + Jp[1][p] * Jl[1][c]);
                int k = 0;
#pragma unroll
                for (int p = 0; p < 6; ++p)
#pragma unroll
                    for (int q = p; q < 6; ++q) { acc[k] = w * (Jp[0][p] * Jp[0][q] + Jp[1][p] * Jp[1][q]); ++k; }
#pragma unroll
                for (int p = 0; p < 6; ++p) acc[21 + p] = -w * (Jp[0][p] * r0 + Jp[1][p] * r1);
            } else {
#pragma unroll
                for (int k = 0; k < 27; ++k) rec[k] = 0.0;
            }
            if (P.sk_pcg) {                                        // PCG form: the operator's 24 values once more, value-major (k_skin_op reads them coalesced)
#pragma unroll
                for (int k = 0; k < 6; ++k) P.sk_recT[(size_t)k * P.sk_n + i] = rec[k];
#pragma unroll
                for (int k = 0; k < 18; ++k) P.sk_recT[(size_t)(6 + k) * P.sk_n + i] = rec[9 + k];
            }
        }
    }
    block_sum_store<28>(acc, lds, tid, P.sk_part + (size_t)blockIdx.x * 32);
}

// ---- embedded BA windows (N2b): K poses, the skinned observations act through the PCG path -------------------------------------------
// Per linearisation, behind the lineariser and k_pose_sums (which WRITE D, b_l, H_pp, b_p): what the observations add to them.
//   k_skin_rows : a node row's diagonal block += sum om^2 J_l^T w J_l, its gradient += sum om (-J_l^T w r) over its list
//   k_skin_pose : H_pp / b_p of a pose += the block sums k_skin left (its blocks in order)
// Per PCG iteration, behind k_spmv_f:  H u of the observations' blocks, with s_o = sum_k om_k u_{n_k}:
//   k_skin_op      (per observation): g_o = A_o s_o + B_o^T u_p; block sums of B_o s_o (pose rows), of (B_o^T u_p) . s_o (the
//                                     observations' share of the cross term u_l . H_lp u_p) and of g_o . s_o (their share of w.u)
//   per node row                    : w_row += sum om g_o -- by k_pcg_update<true> for the rows it updates (k_skin_op_rows where the
//                                     update is the generic kernel)
// k_pcg_update / k_reduce_partials add the block sums in (fixed order): every scalar of the iteration is known after the FIRST launch
// (k_spmv_f_skin), so the row pass needs no reduction of its own and the iteration is two launches.  SK_RL lanes per list, combined by the fixed butterfly of
// sub_sum_t.  Both kernels are bound by the number of cache lines a wave's loads touch (one wave per SIMD at this size): the
// per-observation operands are value-major (sk_recT, sk_row, sk_om: a load instruction of 64 observations touches 4 lines, not 64),
// g_o is 3 values in a 32-byte slot (two 16-byte loads per list entry).

__device__ inline void sk_atomic_max(double* addr, double v) {     // v >= 0: the bit patterns of non-negative doubles order like integers
    atomicMax(reinterpret_cast<unsigned long long*>(addr), (unsigned long long)__double_as_longlong(v));
}

__global__ __launch_bounds__(BLK) void k_skin_rows(Dev P) {
    const int tid = threadIdx.x, j = blockIdx.x * SK_RPB + tid / SK_RL, t = tid % SK_RL;
    double D[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
    const bool live = j < P.sk_nrl && !(P.rflag[P.sk_rl_row[min(j, P.sk_nrl - 1)]] & RF_FIXED);   // (a fixed row is an identity row: nothing is added to it)
    if (live)
        for (int q = P.sk_rl_ptr[j] + t; q < P.sk_rl_ptr[j + 1]; q += SK_RL) {
            const double om = P.sk_rl_om[q];
            const double* rec = P.sk_rec + 27 * (size_t)P.sk_rl_obs[q];
            const double o2 = om * om;
#pragma unroll
            for (int k = 0; k < 6; ++k) D[k] += o2 * rec[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) b[k] += om * rec[6 + k];
        }
#pragma unroll
    for (int k = 0; k < 6; ++k) D[k] = sub_sum_t<SK_RL>(D[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = sub_sum_t<SK_RL>(b[k]);
    if (live && t == 0) {
        const size_t row = (size_t)P.sk_rl_row[j];
        double* Dr = P.D + 6 * row;
        double dd[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) { dd[k] = Dr[k] + D[k]; Dr[k] = dd[k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) P.bl[3 * row + k] += b[k];
        sk_atomic_max(P.sk_maxdiag, fmax(fabs(dd[0]), fmax(fabs(dd[3]), fabs(dd[5]))));
    }
}

// (27 sh_nk threads from pose sh_k0: the poses this engine owns -- every pose on one GPU.  A rank of a sharded window leaves the other
// poses alone: their H_pp still hold the last all-reduced values, which must neither be added to nor enter the max diagonal.)
__global__ __launch_bounds__(BLK) void k_skin_pose(Dev P) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= 27 * P.sh_nk) return;
    const int k = P.sh_k0 + i / 27, cc = i % 27;
    double s = 0;
    for (int b = P.sk_pose_blk[k]; b < P.sk_pose_blk[k + 1]; ++b) s += P.sk_part[(size_t)b * 32 + cc];
    if (cc < 21) {
        const double v = P.Hpp[21 * k + cc] + s;
        P.Hpp[21 * k + cc] = v;
        if (cc == 0 || cc == 6 || cc == 11 || cc == 15 || cc == 18 || cc == 20) sk_atomic_max(P.sk_maxdiag, fabs(v));
    } else P.bp[6 * k + (cc - 21)] += s;
}

__device__ __forceinline__ void skin_op_body(const Dev& P, const int it, const int blk) {
    __shared__ double lds[4 * 8];
    const int tid = threadIdx.x, i = blk * BLK + tid;
    double q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int done = P.flags[0];                                   // (read beside the first operands, not before them)
    if (i < P.sk_n) {
        const int kp = P.sk_blk_pose[blk];
        const double* up = ((it & 1) ? P.up2 : P.up) + 6 * kp;
        const size_t n = (size_t)P.sk_n;
        double s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int k = 0; k < SK_MAX; ++k) {
            const int row = P.sk_row[k * n + i];
            const double om = P.sk_om[k * n + i];
            if (row >= 0) { s0 += om * P.uv3[3 * (size_t)row]; s1 += om * P.uv3[3 * (size_t)row + 1]; s2 += om * P.uv3[3 * (size_t)row + 2]; }
        }
        const double* rec = P.sk_recT + i;                         // A_o (6), B_o (18), value-major
        const double A0 = rec[0], A1 = rec[n], A2 = rec[2 * n], A3 = rec[3 * n], A4 = rec[4 * n], A5 = rec[5 * n];
        const double a0 = A0 * s0 + A1 * s1 + A2 * s2, a1 = A1 * s0 + A3 * s1 + A4 * s2, a2 = A2 * s0 + A4 * s1 + A5 * s2;
        double g0 = 0, g1 = 0, g2 = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            const double b0 = rec[(6 + 3 * p) * n], b1 = rec[(7 + 3 * p) * n], b2 = rec[(8 + 3 * p) * n], u = up[p];
            g0 += b0 * u; g1 += b1 * u; g2 += b2 * u;
            q[p] = b0 * s0 + b1 * s1 + b2 * s2;
        }
        q[6] = g0 * s0 + g1 * s1 + g2 * s2;                        // (B_o^T u_p) . s_o
        q[7] = (a0 + g0) * s0 + (a1 + g1) * s1 + (a2 + g2) * s2;   // g_o . s_o = sum over the observation's rows of u_row . (om g_o): its share of w.u
        if (!done) {
            double* g = P.sk_g + 4 * (size_t)i;
            g[0] = a0 + g0; g[1] = a1 + g1; g[2] = a2 + g2;
        } else {                                                   // (the solve has finished: nothing is added any more)
#pragma unroll
            for (int p = 0; p < 8; ++p) q[p] = 0;
        }
    }
    block_sum<8>(q, lds, tid & 63, tid >> 6);
    if (tid == 0) {
#pragma unroll
        for (int p = 0; p < 8; ++p) P.sk_opart[(size_t)blk * 8 + p] = q[p];
    }
}
__global__ __launch_bounds__(BLK) void k_skin_op(Dev P, int it) { skin_op_body(P, it, (int)blockIdx.x); }
// The operator of the regularisers and the observations' pass in ONE launch: the two read u and write different things (w's rows /
// sk_g and the block sums), so the first n_op workgroups are k_spmv_f's and the rest k_skin_op's -- one launch and one kernel's
// chain of dependent loads less per PCG iteration (both are latency-bound at a BA window's size).  Same bodies, same bits.
template <int T>
__global__ __launch_bounds__(BLK, 4) void k_spmv_f_skin(Dev P, double lam, int cls, int it, double tol2, int n_op) {
    if ((int)blockIdx.x < n_op) spmv_f_body<T, false>(P, lam, cls, it, tol2, (int)blockIdx.x);
    else skin_op_body(P, it, (int)blockIdx.x - n_op);
}

// The row pass in a launch of its own (large windows on the hierarchical reduction, NRS_SKIN_ROWS_OWN_LAUNCH=1): w_row += sum om g_o.
// Otherwise k_pcg_update<true> does it for the rows it is about to update.  The rows' shares of the dot products are k_skin_op's.
__global__ __launch_bounds__(BLK) void k_skin_op_rows(Dev P) {
    const int tid = threadIdx.x, r = P.sh_vb0 * BLK + blockIdx.x * SK_RPB + tid / SK_RL, t = tid % SK_RL;   // (the own rows, sh_nvb * BLK / SK_RPB workgroups)
    const int done = P.flags[0], q0 = P.sk_row_q[2 * (size_t)r], q1 = P.sk_row_q[2 * (size_t)r + 1];
    const uint8_t rf = P.rflag[r];
    const double w0 = P.wv[3 * (size_t)r], w1 = P.wv[3 * (size_t)r + 1], w2 = P.wv[3 * (size_t)r + 2];
    const bool live = !done && q1 > q0 && !(rf & RF_FIXED);       // (a fixed row is an identity row: nothing is added to it)
    double a[3] = {0, 0, 0};
    if (live) skin_row_gather(P, q0, q1, t, a);
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = sub_sum_t<SK_RL>(a[k]);
    if (live && t == 0) { P.wv[3 * (size_t)r] = w0 + a[0]; P.wv[3 * (size_t)r + 1] = w1 + a[1]; P.wv[3 * (size_t)r + 2] = w2 + a[2]; }
}

// ---- embedded mode: set-up of the skinned observations of an engine whose rows are packed (engine_create; device arrays in a buffer of the
// context).  A BA window (N2b: sk_pose given, K poses) solves by the PCG with the observations applied as hyper-edges; a single-frame
// engine (N2a) by the direct solver when it takes the frame (k_nd_values folds them into its blocks) and by the same PCG form when it
// does not.
// Slots: observations grouped by pose (caller order inside a pose: K = 1 keeps the caller's order), every pose's padded to BLK;
// per node row the list of the observations that reach it, in slot order.
// A rank of a sharded window (communicator) holds the observations of its OWN keyframes [sh_k0, sh_k0 + sh_nk) only: they reach
// node copies of their own keyframe (checked below), so everything they read or write is rank-local and no halo row is needed;
// their pose blocks and chi2 join the all-reduced packets once (k_finalize_pack).  Observations held elsewhere: sk_slot = -1.
// A SLICED list (s.sk_total > 0: the rank's share of a window whose lists were built on its device) holds nothing else: every entry
// must be the rank's own, and the keyframe range it was cut for must be the one this set-up arrived at.
static int skin_setup(nrs_ctx* c, Engine* e, const EngineSpec& s, Arena* arena) {
    Dev& d = e->d;
    const bool ba_form = s.sk_pose != nullptr;
    if (d.fused || (d.sh_on && !ba_form) || !s.sk_uv || !s.sk_X0 || !s.sk_node || !s.sk_om) return c->fail(NRS_ERR_INVALID, "skinned observations: two-kernel PCG path");
    if (!ba_form && !(arena == &c->arena_trk && s.K == 1)) return c->fail(NRS_ERR_INVALID, "skinned observations without a pose index: single-frame tracking engines only");
    const size_t n_in = (size_t)s.n_skin;
    const bool sliced = s.sk_total > 0;
    if (sliced && (!ba_form || !d.sh_on || s.sk_base < 0 || s.n_skin < 0 || (int64_t)s.sk_base + s.n_skin > s.sk_total))
        return c->fail(NRS_ERR_INVALID, "skinned observations: a sliced list needs a sharded BA window and a slice inside the window's list");
    if (sliced && (s.sk_k0 != d.sh_k0 || s.sk_k1 != d.sh_k0 + d.sh_nk))
        return c->fail(NRS_ERR_STATE, "skinned observations: the list was cut for keyframes [%d, %d), the rank owns [%d, %d)", s.sk_k0, s.sk_k1, d.sh_k0, d.sh_k0 + d.sh_nk);
    std::vector<int> pose0;
    if (!ba_form) pose0.assign(n_in, 0);
    const int* sk_pose = ba_form ? s.sk_pose : pose0.data();
    const int own_k0 = d.sh_k0, own_k1 = d.sh_k0 + d.sh_nk;    // (the whole window on one GPU)
    auto held = [&](size_t i) { return sk_pose[i] >= own_k0 && sk_pose[i] < own_k1; };
    std::vector<int> cnt(s.K + 1, 0), pose_blk(s.K + 1, 0);
    for (size_t i = 0; i < n_in; ++i) {
        if (sk_pose[i] < 0 || sk_pose[i] >= s.K) return c->fail(NRS_ERR_INVALID, "skinned observation: pose index out of range");
        if (held(i)) cnt[sk_pose[i] + 1]++;
        else if (sliced) return c->fail(NRS_ERR_INVALID, "skinned observation: a sliced list holds an observation of keyframe %d, outside the rank's [%d, %d)", sk_pose[i], own_k0, own_k1);
    }
    for (int k = 0; k < s.K; ++k) pose_blk[k + 1] = pose_blk[k] + (cnt[k + 1] + BLK - 1) / BLK;
    if (d.sh_on && pose_blk[s.K] == 0)                         // (a rank whose keyframes have none: one empty block of its first pose, so that every launch has a grid)
        for (int k = own_k0; k < s.K; ++k) pose_blk[k + 1]++;
    const size_t nblk = (size_t)pose_blk[s.K], n = nblk * BLK;
    std::vector<int> next(s.K), blk_pose(nblk);
    for (int k = 0; k < s.K; ++k) { next[k] = pose_blk[k] * BLK; for (int b2 = pose_blk[k]; b2 < pose_blk[k + 1]; ++b2) blk_pose[b2] = k; }
    e->sk_slot.assign(n_in, -1);
    std::vector<float> uv(2 * n, 0.f);
    std::vector<double> X0(3 * n, 0.0), om(SK_MAX * n, 0.0);
    std::vector<int> rows(SK_MAX * n, -1), src(n, -1);
    std::vector<uint8_t> act(n, 0);
    std::vector<int> rl_cnt(d.n_rows + 1, 0);
    for (size_t i = 0; i < n_in; ++i) {
        if (!held(i)) continue;
        const size_t sl = (size_t)next[sk_pose[i]]++;
        e->sk_slot[i] = (int)sl;
        src[sl] = (int)i;
        uv[2 * sl] = s.sk_uv[2 * i]; uv[2 * sl + 1] = s.sk_uv[2 * i + 1];
        for (int k = 0; k < 3; ++k) X0[3 * sl + k] = s.sk_X0[3 * i + k];
        act[sl] = 1;
        for (int k = 0; k < SK_MAX; ++k) {
            const int v = s.sk_node[SK_MAX * i + k];
            if (v < 0) continue;
            if (s.lm_pose[v] != sk_pose[i]) return c->fail(NRS_ERR_INVALID, "skinned observation: a node copy of another keyframe");
            rows[(size_t)k * n + sl] = e->vrow[v];              // (11 x n, node-slot-major: the kernels read them coalesced)
            om[(size_t)k * n + sl] = s.sk_om[SK_MAX * i + k];
            rl_cnt[e->vrow[v] + 1]++;
        }
    }
    // row lists (CSR over the rows that are reached), entries in slot order
    std::vector<int> rl_row, rl_ptr(1, 0), row_list(d.n_rows, -1);
    for (int r = 0; r < d.n_rows; ++r)
        if (rl_cnt[r + 1] > 0) { row_list[r] = (int)rl_row.size(); rl_row.push_back(r); rl_ptr.push_back(rl_ptr.back() + rl_cnt[r + 1]); }
    const size_t n_ent = (size_t)rl_ptr.back(), nrl = rl_row.size();
    if (d.sh_on) {                                             // a rank's per-row arrays may be row-limited (biased pointers, ArenaPlan::get_rows):
        const int own_lo = d.sh_g0 * ROW_ALIGN, own_hi = (d.sh_g0 + d.sh_ng) * ROW_ALIGN;   // no launch may reach a row it does not own
        for (size_t q = 0; q < rows.size(); ++q)
            if (rows[q] >= 0 && (rows[q] < own_lo || rows[q] >= own_hi)) return c->fail(NRS_ERR_INVALID, "skinned observation: node row %d outside the rank's rows [%d, %d)", rows[q], own_lo, own_hi);
        for (size_t l = 0; l < nrl; ++l)
            if (rl_row[l] < own_lo || rl_row[l] >= own_hi) return c->fail(NRS_ERR_INVALID, "skinned observations: row list %d outside the rank's rows [%d, %d)", rl_row[l], own_lo, own_hi);
    }
    std::vector<int> rl_obs(n_ent + 1), fill(rl_ptr.begin(), rl_ptr.end() - 1);
    std::vector<double> rl_om(n_ent + 1);
    for (size_t sl = 0; sl < n; ++sl)
        for (int k = 0; k < SK_MAX; ++k) {
            const int r = rows[(size_t)k * n + sl];
            if (r < 0) continue;
            const int q = fill[row_list[r]]++;
            rl_obs[q] = (int)sl; rl_om[q] = om[(size_t)k * n + sl];
        }
    auto al = [](size_t b2) { return (b2 + 255) & ~(size_t)255; };
    const size_t o_uv = 0, o_X0 = o_uv + al(8 * n), o_row = o_X0 + al(24 * n), o_om = o_row + al(4 * SK_MAX * n), o_act = o_om + al(8 * SK_MAX * n),
                 o_bp = o_act + al(n), o_pb = o_bp + al(4 * nblk), o_rr = o_pb + al(4 * (s.K + 1)), o_rp = o_rr + al(4 * (nrl + 1)), o_ro = o_rp + al(4 * (nrl + 1)),
                 o_rw = o_ro + al(4 * (n_ent + 1)), o_rec = o_rw + al(8 * (n_ent + 1)), o_part = o_rec + al(8 * 27 * n), o_chi = o_part + al(8 * 32 * nblk),
                 o_md = o_chi + al(8 * n), o_g = o_md + 256, o_op = o_g + al(8 * 4 * n), o_rq = o_op + al(8 * 8 * nblk), o_src = o_rq + al(8 * (size_t)d.n_rows), o_recT = o_src + al(4 * n),
                 o_dop = o_recT + al(8 * 24 * n), o_spec = o_dop + (d.use_lds ? 0 : al(8 * 6 * (size_t)d.n_rows)),
                 spec_stride = al(8 * 32 * nblk) + al(8 * n), total = o_spec + (size_t)e->n_spec * spec_stride;   // (shadow sets of sk_part / sk_chi: speculative trials)
    DevBuf& buf = arena == &c->arena_trk ? c->nd_skin : c->dba_skin;
    NRS_TRY(c->ensure(buf, total));
    e->sk_bytes = total;
    char* sb = buf.as<char>();
    auto up = [&](size_t off, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(sb + off, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess; };
    NRS_HIP(c, up(o_uv, uv.data(), 8 * n)); NRS_HIP(c, up(o_X0, X0.data(), 24 * n)); NRS_HIP(c, up(o_row, rows.data(), 4 * SK_MAX * n));
    NRS_HIP(c, up(o_om, om.data(), 8 * SK_MAX * n)); NRS_HIP(c, up(o_act, act.data(), n)); NRS_HIP(c, up(o_bp, blk_pose.data(), 4 * nblk));
    NRS_HIP(c, up(o_pb, pose_blk.data(), 4 * (size_t)(s.K + 1))); NRS_HIP(c, up(o_rr, rl_row.data(), 4 * nrl)); NRS_HIP(c, up(o_rp, rl_ptr.data(), 4 * (nrl + 1)));
    NRS_HIP(c, up(o_ro, rl_obs.data(), 4 * n_ent)); NRS_HIP(c, up(o_rw, rl_om.data(), 8 * n_ent));
    NRS_HIP(c, hipMemsetAsync(sb + o_rec, 0, total - o_rec, c->stream));
    std::vector<int> row_q(2 * (size_t)d.n_rows, 0);           // per row: its list's range (k_pcg_update<true> / k_skin_op_rows go by rows)
    for (size_t l = 0; l < nrl; ++l) { row_q[2 * (size_t)rl_row[l]] = rl_ptr[l]; row_q[2 * (size_t)rl_row[l] + 1] = rl_ptr[l + 1]; }
    NRS_HIP(c, up(o_rq, row_q.data(), 8 * (size_t)d.n_rows));
    NRS_HIP(c, up(o_src, src.data(), 4 * n));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    d.sk_n = (int)n; d.sk_nblk = (int)nblk; d.sk_pcg = 1;      // (a single-frame engine on the direct solver switches sk_pcg off below)
    d.sk_uv = reinterpret_cast<const float*>(sb + o_uv); d.sk_X0 = reinterpret_cast<const double*>(sb + o_X0);
    d.sk_row = reinterpret_cast<const int*>(sb + o_row); d.sk_om = reinterpret_cast<const double*>(sb + o_om);
    d.sk_active = reinterpret_cast<const uint8_t*>(sb + o_act);
    d.sk_blk_pose = reinterpret_cast<const int*>(sb + o_bp); d.sk_pose_blk = reinterpret_cast<const int*>(sb + o_pb);
    d.sk_nrl = (int)nrl; d.sk_rl_row = reinterpret_cast<const int*>(sb + o_rr); d.sk_rl_ptr = reinterpret_cast<const int*>(sb + o_rp);
    d.sk_rl_obs = reinterpret_cast<const int*>(sb + o_ro); d.sk_rl_om = reinterpret_cast<const double*>(sb + o_rw);
    d.sk_rec = reinterpret_cast<double*>(sb + o_rec); d.sk_part = reinterpret_cast<double*>(sb + o_part);
    d.sk_chi = reinterpret_cast<double*>(sb + o_chi); d.sk_maxdiag = reinterpret_cast<double*>(sb + o_md);
    d.sk_g = reinterpret_cast<double*>(sb + o_g); d.sk_opart = reinterpret_cast<double*>(sb + o_op); d.sk_row_q = reinterpret_cast<const int*>(sb + o_rq);
    d.sk_recT = reinterpret_cast<double*>(sb + o_recT); d.sk_src = reinterpret_cast<const int*>(sb + o_src);
    d.D_op = d.use_lds ? nullptr : reinterpret_cast<double*>(sb + o_dop);
    for (int j = 0; j < e->n_spec; ++j) {
        e->spec[j].sk_part = reinterpret_cast<double*>(sb + o_spec + (size_t)j * spec_stride);
        e->spec[j].sk_chi = reinterpret_cast<double*>(sb + o_spec + (size_t)j * spec_stride + al(8 * 32 * nblk));
    }
    d.sk_base = ba_form ? d.xl_init : nullptr;                 // (tracking form: the rows ARE the deformations, X0 + sum om x)
    e->sk_total = s.sk_window(); e->sk_base = sliced ? s.sk_base : 0;
    if (!ba_form) {                                            // (the direct solver's plan reads them; a BA window's positions come from k_skin_positions)
        e->sk_vert.assign(s.sk_node, s.sk_node + SK_MAX * n_in);
        e->sk_om.assign(s.sk_om, s.sk_om + SK_MAX * n_in);
    }
    return NRS_OK;
}

}  // namespace nrs
