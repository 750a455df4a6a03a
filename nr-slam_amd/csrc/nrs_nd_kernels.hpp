// Direct solve of a2's single-frame system (H + lambda I) x = b: multifrontal Cholesky on the nested-dissection plan of
// nrs_nd_plan.hpp, dense fronts on v_mfma_f64_16x16x4.  Part of nrs_engine.hip (one translation unit).
//
// Reference: LinearSolverEigen::solve (third_party/g2o/g2o/solvers/eigen/linear_solver_eigen.h:92-136) -- a sparse Cholesky of
// the whole system per LM trial, `not positive definite` reported as a failed solve -- as CameraPoseAndDeformationOptimization
// drives it (modules/optimization/g2o_optimization.cc:148-557, block_solver.hpp:329-341: no Schur ordering, nothing marginalised).
//
// Factorisation: one launch per tree level (leaves first).  A workgroup is (front f, boundary row blocks I >= J): it assembles
// the front's own block F11 (<= 96 x 96) and the two 48-row blocks of F21 in LDS -- original entries, then the children's Schur
// complements by dense reads of the slots they wrote in THIS front's index space, in a fixed order (no atomics:
// bit-reproducible) -- factorises the tall panel [F11; F21_I; F21_J] by 16-column steps (diagonal block in one wave and panel
// rows one per thread, both on DPP row broadcasts; trailing update on the matrix cores), and leaves the tile
// U_IJ = F22_IJ - L21_I L21_J^T (matrix cores) in the parent's slot.  F11 is factorised redundantly by every workgroup of a
// front: it is the latency of the level either way, and the tiles of a large boundary then spread over the CUs without a second
// launch.  The right-hand side is one more boundary row, so the forward substitution rides along.  One more workgroup per front
// factorises [F11; I] and leaves (L11^-1)^T behind the factor.
// Back pass: ONE launch (k_nd_back), a workgroup per front, top-down: factors staged on chip, then ancestor by ancestor
// (the unknowns above are polled where they land: xn is poisoned at the start of a solve) x_own = (L11^-1)^T (y - L21^T x_bnd) as
// two matrix-vector products.
// Values: k_nd_values turns a linearisation into the plan's entry blocks (engines only).
// This file is the device code; around it: nrs_nd_solver.hpp (upload and launches), nrs_nd_debug.hpp (the solver on its own),
// nrs_nd_prep_host.hpp (the set-up's host stages, no HIP) and nrs_engine_nd.hpp (plan cache, plan thread, the two set-up phases).
#pragma once
#include <type_traits>
#include "nrs_nd_plan.hpp"

namespace nrs {

constexpr int ND_LD = 97;            // LDS leading dimension (doubles): odd, so the column-strided operand reads of the MFMAs are conflict-free
constexpr int ND_S16 = 96;
typedef double nd_v4d __attribute__((ext_vector_type(4)));
constexpr unsigned long long ND_POISON = 0x7FF8A5A5DEADBEEFull;   // "not written yet" in xn: a NaN payload no arithmetic produces

struct NdWgD { NdFrontD F; int I, J, pad; };          // one workgroup of k_nd_level: its front and its (I >= J) pair of row blocks
struct NdDev {
    const int* own; const int* bnd; const int* seg; const int16_t* pmap; const NdEnt* ent; const NdWgD* wg; const NdFrontD* lvl_fr;
    const double* ev;                // 9 doubles per original entry (plan order): the blocks of the current linearisation
    double* A;                       // assembly areas: every front's Schur complement lands in its parent's index space
    double* Lp; double* xn;
    const int* node_out;             // engine: node -> 3 doubles at out_rows + o (o >= 0) or out_pose - 1 - o (o < 0); null: xn only
    double* out_rows; double* out_pose;
    int* done;                       // per front: the solve (epoch) whose back substitution has written its unknowns (single-launch back pass)
    int* fcnt;                       // per front: Schur tiles its children have delivered, over all solves (single-launch factorisation)
    int* flags;                      // [0] done [1] iterations [2] not positive definite (the engine's PCG flags, or a scratch word block)
    int n_x3;                        // 3 x nodes: the length of xn
    int x_poll;                      // back pass: 1 = a front reads its boundary's unknowns by polling the VALUES (xn is poisoned when a solve starts and every
                                     // unknown is written once), 0 = by its ancestors' done flags (NRS_ND_BACK_FLAGS=1: the round-4 hand-over)
    const int* abort; int abort_id;  // speculative trials (engine_optimize): a solve whose id the host has written to *abort is not needed any more -- the
                                     // remaining workgroups of its FACTORISATION return at once (null: never); they wait for nobody, so a stale read only costs time
    long long* clk;                  // NRS_ND_DBG: 8 phase clocks (100 MHz) per workgroup of the factorisation, then per front of the back substitution; else null
};
static_assert(std::is_trivially_copyable_v<NdDev>, "passed to kernels by value: plain pointers, never an owner");

// value of lane K of the caller's 16-lane row, in every lane of the row: DPP row_newbcast (a plain VALU move, no SGPR round trip)
template <int K>
__device__ inline double nd_rowbcast(double v) { return __builtin_amdgcn_update_dpp(v, v, 0x150 + K, 0xf, 0xf, false); }
// a += (lane K's nl of this 16-lane row) * l in ONE instruction: the DPP form of v_fmac_f64 (gfx90a+ encode row_newbcast on the
// fp64 ALU).  Measured on gfx950 (tools/micro/diag_probe.hip), per 16 x 16 block: v_readlane + FMA 5100 cycles, v_mov_b64_dpp +
// FMA 4480, this form 3350.
template <int K>
__device__ inline void nd_fmac_bcast(double& a, double nl, double l) {
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(a) : "v"(nl), "v"(l), "n"(K));
}

// a -= (lane K's ls of this 16-lane row) * l: the negation rides on the DPP operand (src0 neg modifier), so no negated copy is made
template <int K>
__device__ inline void nd_fmacn_bcast(double& a, double ls, double l) {
    asm("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(a) : "v"(ls), "v"(l), "n"(K));
}

// Cholesky of one 16 x 16 diagonal block of the panel, one wave: lane (i = lane & 15) of every 16-lane row holds row i (the four
// rows of the wave work redundantly, so every broadcast stays inside a row).  Column j: the pivot reaches the lanes by a row
// broadcast, a[k] -= l_ij l_kj by the DPP FMA.  Leaves the block in W (lower triangle) and 1 / diag in dinv.  The wave is ISSUE-bound
// here (tools/micro/diag_probe.hip: pinning the next column's pivot chain between this column's independent updates buys 8 %, a
// shorter chain 13 %): ten VALU operations per pivot -- a bad pivot is replaced by changing its high word only (any value in
// [1, 2) will do: one select instead of two), no negated copy of the column -- 3350 -> 2900 cycles per block.
template <int J, int K>
__device__ inline void nd_diag_cols_upd(double (&a)[16], double l) {
    if constexpr (K < 16) {
        nd_fmacn_bcast<K>(a[K], l, l);
        nd_diag_cols_upd<J, K + 1>(a, l);
    }
}
template <int J>
__device__ inline void nd_diag_cols(double (&a)[16], double (&rr)[16], int& bad) {
    if constexpr (J < 16) {
        double ajj = nd_rowbcast<J>(a[J]);
        const bool ok = ajj > 0.0;
        bad |= !ok;
        ajj = __hiloint2double(ok ? __double2hiint(ajj) : 0x3FF00000, __double2loint(ajj));
        const double r = fast_rsqrt_pos(ajj);
        double l = a[J] * r;                                       // (lane J: a_jj r = sqrt(a_jj))
        asm volatile("s_nop 1" : "+v"(l));                         // (a VALU result read through DPP needs two wait states)
        a[J] = l; rr[J] = r;
        nd_diag_cols_upd<J, J + 1>(a, l);
        nd_diag_cols<J + 1>(a, rr, bad);
    }
}

__device__ __forceinline__ void nd_diag_factor(double* W, double* dinv, int k0, int lane, int& bad) {
    const int i = lane & 15;
    double a[16], rr[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) a[j] = W[(k0 + i) * ND_LD + k0 + j];
    nd_diag_cols<0>(a, rr, bad);
    if (lane < 16) {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j <= i) W[(k0 + i) * ND_LD + k0 + j] = a[j];
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) dinv[k0 + j] = rr[j];
    }
}

// step B of the panel factorisation for one row held in x: x <- x L_kk^-T, L_kk row (lane & 15) in lk (see k_nd_level)
template <int P, int Q>
__device__ inline void nd_b_upd(double (&x)[16], const double (&lk)[16], double xp) {
    if constexpr (Q < 16) {
        nd_fmacn_bcast<Q>(x[Q], lk[P], xp);                        // x[Q] -= (lane Q's L[Q][P]) * x[P]
        nd_b_upd<P, Q + 1>(x, lk, xp);
    }
}
template <int P>
__device__ inline void nd_b_cols(double (&x)[16], const double (&lk)[16], const double (&di)[16]) {
    if constexpr (P < 16) {
        x[P] *= di[P];
        nd_b_upd<P, P + 1>(x, lk, x[P]);
        nd_b_cols<P + 1>(x, lk, di);
    }
}

// the solved unknowns of a front go to the node vector and, for an engine, straight into its step vectors; the two index loads
// (node of the unknown, its output slot) are requested at kernel start (NdOut) so that no memory round trip follows the solve
struct NdOut { int node[2], o[2]; };
__device__ __forceinline__ NdOut nd_out_request(const NdDev& N, const NdFrontD& F, int lane) {
    NdOut r;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int q = lane + 64 * h;
        r.node[h] = N.own[F.own_off + (q < F.s ? q / 3 : 0)];
        r.o[h] = N.node_out ? N.node_out[r.node[h]] : 0;
    }
    return r;
}
__device__ __forceinline__ void nd_store_x(const NdDev& N, const NdFrontD& F, const NdOut& r, int lane, double x0, double x1) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int q = lane + 64 * h;
        if (q >= F.s) continue;
        const double xv = h ? x1 : x0;
        if (N.x_poll) __hip_atomic_store(N.xn + 3 * (size_t)r.node[h] + q % 3, xv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a reader polls this very word)
        else N.xn[3 * (size_t)r.node[h] + q % 3] = xv;
        if (N.node_out) { if (r.o[h] >= 0) N.out_rows[r.o[h] + q % 3] = xv; else N.out_pose[-1 - r.o[h] + q % 3] = xv; }
    }
}

// trailing update of the panel factorisation on the matrix cores: C_rb,cb -= P_rb P_cb^T for the block columns cb in [cb_lo, cb_hi) and
// the row blocks rb >= cb, P = the 16 columns at k0; the tiles are dealt round-robin to the waves w0 .. w0 + nw - 1 (this wave: widx)
// (KB: the panel is KB consecutive 16-column blocks at k0 -- two of them in the 32-column steps, applied in column order: the same
// sequence of matrix-core operations on a tile as two single-block updates one after the other)
template <int KB = 1>
__device__ __forceinline__ void nd_update(double* W, int lane, int k0, int cb_lo, int cb_hi, int nrt, int widx, int nw, int skip_first = 0) {
    if (widx < 0 || widx >= nw) return;
    int cnt = 0;
#pragma unroll 1
    for (int cb = cb_lo; cb < cb_hi; ++cb)
#pragma unroll 1
        for (int rb = cb + (cb == cb_lo ? skip_first : 0); rb < nrt; ++rb, ++cnt) {      // (skip_first: the diagonal tile of the first column is somebody else's)
            if (cnt % nw != widx) continue;
            nd_v4d c;
            double av[4 * KB], bv[4 * KB];
#pragma unroll
            for (int g = 0; g < 4; ++g) c[g] = W[(16 * rb + (lane >> 4) + 4 * g) * ND_LD + 16 * cb + (lane & 15)];
#pragma unroll
            for (int kk = 0; kk < 4 * KB; ++kk) {
                av[kk] = -W[(16 * rb + (lane & 15)) * ND_LD + k0 + 4 * kk + (lane >> 4)];
                bv[kk] = W[(16 * cb + (lane & 15)) * ND_LD + k0 + 4 * kk + (lane >> 4)];
            }
#pragma unroll
            for (int kk = 0; kk < 4 * KB; ++kk) c = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kk], bv[kk], c, 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 4; ++g) W[(16 * rb + (lane >> 4) + 4 * g) * ND_LD + 16 * cb + (lane & 15)] = c[g];
        }
}

// step B of the panel factorisation for the panel row `row` against the diagonal block at k0 (one row per calling thread; the store is
// predicated by `live`): see k_nd_level
__device__ __forceinline__ void nd_b_row(double* W, const double* dinv, int k0, int row, bool live, int lane) {
    const int li = lane & 15;
    double x[16], lk[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) { x[q] = W[row * ND_LD + k0 + q]; lk[q] = W[(k0 + li) * ND_LD + k0 + q]; }
    double di[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) di[q] = dinv[k0 + q];
    nd_b_cols<0>(x, lk, di);
    if (live) {
#pragma unroll
        for (int q = 0; q < 16; ++q) W[row * ND_LD + k0 + q] = x[q];
    }
}

// NTH threads per workgroup: 256, or 512 (two waves per SIMD: seven waves instead of three on the trailing updates next to the diagonal
// block, one pass over the children's slots instead of two, a Schur tile per wave); which wave computes a tile does not change its bits
template <int NTH, bool W32 = false>
__global__ __launch_bounds__(NTH) void k_nd_level(NdDev N, int wg0, double lam, int epoch, int chained, int first) {   // first: the first launch of a solve (poisons xn for the back pass)   // chained: 0 = one launch per level, else the count of single-launch factorisations so far
    extern __shared__ double sm[];
    constexpr int NW = NTH / 64, NT3 = (9 + NW - 1) / NW;          // waves; Schur tiles (of nine) per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const NdWgD wd = N.wg[wg0 + blockIdx.x];                        // (front descriptor inlined: one scalar round trip)
    const int I = wd.I, J = wd.J;
    const NdFrontD& F = wd.F;
    const int s = F.s, s16 = (s + 15) & ~15, b1 = F.b + 1, m = s + F.b;
    // I < 0: the front's INVERSE workgroup.  Its panel is [F11; identity]: the factorisation leaves e_j^T L11^-T = row j of
    // (L11^-1)^T under F11, which the back pass multiplies with instead of substituting (no dependent chain on its critical path)
    const bool inv = I < 0;
    const int rI = inv ? 0 : min(ND_TB, b1 - ND_TB * I);           // rows of block I (the last block is partial; J < I is always full)
    const bool two = !inv && J != I;
    const int cJ = two ? ND_TB : rI;
    const int nrow = inv ? 2 * s16 : s16 + ND_TB + (two ? ND_TB : 0);
    const int rowI0 = s16, rowJ0 = two ? s16 + ND_TB : s16;
    double* W = sm;
    double* dinv = W + (size_t)nrow * ND_LD;
    int16_t* pmi = reinterpret_cast<int16_t*>(dinv + ND_S16 + 256);   // (256 doubles unused)           // parent node positions of the nodes of blocks I and J
    int16_t* pmj = pmi + 16;
    auto stamp = [&](int k) { if (N.clk && tid == 0) N.clk[8 * (size_t)(wg0 + blockIdx.x) + k] = wall_clock64(); };
    stamp(0);
    if (N.abort && *N.abort == N.abort_id) return;                 // (a discarded speculative trial drains)
    if (first && N.x_poll)                                         // (nothing reads xn before the back pass of this solve, launches later)
        for (int i = blockIdx.x * NTH + tid; i < N.n_x3; i += gridDim.x * NTH) reinterpret_cast<unsigned long long*>(N.xn)[i] = ND_POISON;
    // ---- requests first: this thread's original entries (descriptor and values: one round trip) and the Schur complements the
    // children left in this front's assembly slots (dense, in this front's own index space: contiguous 16-byte loads)
    auto entry_row = [&](const NdEnt& E) {                         // W row of an entry's first row, -1: not in this workgroup's blocks
        const int fr_row = 3 * (int)E.r;
        if (fr_row < s) return fr_row;
        if (inv) return -1;
        const int rb = fr_row - s;
        if (rb >= ND_TB * I && rb < ND_TB * I + ND_TB) return rowI0 + rb - ND_TB * I;
        if (two && rb >= ND_TB * J && rb < ND_TB * J + ND_TB) return rowJ0 + rb - ND_TB * J;
        return -1;
    };
    constexpr int NE = 512 / NTH;
    NdEnt En[NE];
    double ev[NE][9];
#pragma unroll
    for (int u = 0; u < NE; ++u) {
        const int e = F.ent_off + min(tid + NTH * u, F.n_ent - 1);
        En[u] = N.ent[e];
        const double* v = N.ev + 9 * (size_t)e;
#pragma unroll
        for (int a = 0; a < 9; ++a) ev[u][a] = v[a];
    }
    if (inv) { if (tid < 32) pmi[tid] = -1; }
    else if (tid < 16) { const int np = 16 * I + tid; pmi[tid] = np <= F.b / 3 ? N.pmap[F.pmap_off + np] : (int16_t)-1; }
    else if (tid < 32) { const int np = 16 * J + tid - 16; pmj[tid - 16] = np <= F.b / 3 ? N.pmap[F.pmap_off + np] : (int16_t)-1; }
    const size_t slot = (size_t)(m + 1) * F.ldA;
    const double* A0 = N.A + F.A_off;
    nd_v4d acc[NT3];
#pragma unroll
    for (int q = 0; q < NT3; ++q) acc[q] = nd_v4d{0.0, 0.0, 0.0, 0.0};
    if (chained && wd.pad > 0) {                                   // (pad: the tiles this front's children deliver INSIDE this launch, per solve)
        // every level in one launch: wait until the children's workgroups (smaller block indices: dispatched before this one, so a full
        // chip cannot deadlock; bounded all the same) have delivered their tiles -- wd.pad of them per solve -- then read past stale lines
        if (tid == 0) {
            const int want = chained * wd.pad;
            int spins = 0;
            while (__hip_atomic_load(N.fcnt + F.cmap_off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > (1 << 23)) { N.flags[2] = 2; break; }
            }
        }
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    if (F.n_ch > 0) {                                              // F22 tile (I, J): straight into the accumulators of the matrix cores
        // (the children wrote every element once, at (larger, smaller) of its two positions here: a diagonal tile's upper half is
        // read at its mirror position)
        auto tile_off = [&](int r, int cc) {
            const int fr = s + ND_TB * I + r, fc = s + ND_TB * J + cc;
            return (size_t)max(fr, fc) * F.ldA + min(fr, fc);
        };
        double tv[2][NT3][4];
#pragma unroll
        for (int t3 = 0; t3 < NT3; ++t3) {
            const int t = wave + NW * t3, ti = t / 3, tj = t - 3 * ti;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int r = 16 * ti + (lane >> 4) + 4 * g, cc = 16 * tj + (lane & 15);
                const bool in = t < 9 && r < rI && cc < cJ && ND_TB * J + cc < F.b;
                const size_t o = in ? tile_off(r, cc) : 0;
                tv[0][t3][g] = A0[o];
                tv[1][t3][g] = A0[(F.n_ch > 1 ? slot : 0) + o];
                if (!in) { tv[0][t3][g] = 0.0; tv[1][t3][g] = 0.0; }
            }
        }
#pragma unroll
        for (int t3 = 0; t3 < NT3; ++t3)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[t3][g] = tv[0][t3][g] + (F.n_ch > 1 ? tv[1][t3][g] : 0.0);
        for (int k = 2; k < F.n_ch; ++k)                           // (more than two children: a separator whose halves fell apart)
#pragma unroll
            for (int t3 = 0; t3 < NT3; ++t3) {
                const int t = wave + NW * t3, ti = t / 3, tj = t - 3 * ti;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int r = 16 * ti + (lane >> 4) + 4 * g, cc = 16 * tj + (lane & 15);
                    if (t < 9 && r < rI && cc < cJ && ND_TB * J + cc < F.b) acc[t3][g] += A0[k * slot + tile_off(r, cc)];
                }
            }
    }
    if (F.n_ch == 0) {                                             // a leaf: the panel starts from zero (and the unit diagonals below)
        double2* W2 = reinterpret_cast<double2*>(W);
        for (int i = tid; i < (nrow * ND_LD) >> 1; i += NTH) W2[i] = make_double2(0.0, 0.0);
        __syncthreads();
        if (tid < s16 - s) W[(s + tid) * ND_LD + s + tid] = 1.0;   // padding columns: unit diagonal
        if (inv && tid < s) W[(s16 + tid) * ND_LD + tid] = 1.0;
    } else {
        // panel rows of this workgroup <- sum of the children's slots: W row wr = ty + RG i is front row fr; thread (tx, ty) takes the column
        // pairs 2 tx + 32 j.  The pass writes EVERY element of the panel (rows < nrow, columns < 96) -- zero where no slot element
        // belongs, one on the unit diagonals of the padding columns and of the inverse workgroup's identity -- so nothing is zeroed
        // first and no barrier stands between these loads and the requests above: one memory round trip for entries, tile and panel
        constexpr int RG = NTH / 16;
        const int tx = tid & 15, ty = tid >> 4;
#pragma unroll 1
        for (int i0 = 0; RG * i0 < nrow; i0 += 6) {
            double2 v0[6][3], v1[6][3];
            bool ok[6][3], ok2[6][3];                               // (second column of the pair: only below the row's limit)
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int wr = ty + RG * (i0 + i);
                int fr = -1, lim = s;                              // columns [0, lim) of front row fr
                if (wr < s16) { if (wr < s) { fr = wr; lim = wr + 1; } }
                else if (wr < s16 + ND_TB) { if (wr - s16 < rI) fr = s + ND_TB * I + wr - s16; }
                else if (two && wr < nrow) fr = s + ND_TB * J + wr - s16 - ND_TB;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int q = 2 * tx + 32 * j;
                    ok[i][j] = fr >= 0 && q < lim;
                    ok2[i][j] = fr >= 0 && q + 1 < lim;
                    const size_t o = ok[i][j] ? (size_t)fr * F.ldA + q : 0;
                    v0[i][j] = *reinterpret_cast<const double2*>(A0 + o);
                    v1[i][j] = *reinterpret_cast<const double2*>(A0 + (F.n_ch > 1 ? slot : 0) + o);
                }
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int wr = ty + RG * (i0 + i);
                if (wr >= nrow) continue;
                // the one of this row: padding columns' unit diagonal (rows s .. s16), the identity under F11 (inverse workgroup)
                const int one = wr >= s && wr < s16 ? wr : (inv && wr >= s16 && wr - s16 < s ? wr - s16 : -1);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int q = 2 * tx + 32 * j;
                    double* d = W + wr * ND_LD + q;
                    d[0] = ok[i][j] ? v0[i][j].x + (F.n_ch > 1 ? v1[i][j].x : 0.0) : (q == one ? 1.0 : 0.0);
                    d[1] = ok2[i][j] ? v0[i][j].y + (F.n_ch > 1 ? v1[i][j].y : 0.0) : (q + 1 == one ? 1.0 : 0.0);
                }
            }
        }
        for (int k = 2; k < F.n_ch; ++k) {
            __syncthreads();
            for (int idx = tid; idx < nrow * 48; idx += NTH) {
                const int wr = idx / 48, q = 2 * (idx - 48 * wr);
                int fr = -1, lim = s;
                if (wr < s16) { if (wr < s) { fr = wr; lim = wr + 1; } }
                else if (wr < s16 + ND_TB) { if (wr - s16 < rI) fr = s + ND_TB * I + wr - s16; }
                else if (two) fr = s + ND_TB * J + wr - s16 - ND_TB;
                if (fr < 0 || q >= lim) continue;
                const double2 v = *reinterpret_cast<const double2*>(A0 + k * slot + (size_t)fr * F.ldA + q);
                W[wr * ND_LD + q] += v.x;
                if (q + 1 < lim) W[wr * ND_LD + q + 1] += v.y;
            }
        }
        __syncthreads();
    }
    stamp(1);
    {
        auto put_entry = [&](const NdEnt& E, const double* v, int wr) {
            const uint32_t kind = E.src >> ND_KIND_SHIFT;
            double* dst = W + (size_t)wr * ND_LD + 3 * (int)E.c;
            if (kind == 2) { dst[0] += v[0]; dst[1] += v[1]; dst[2] += v[2]; return; }
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int j = 0; j < 3; ++j) dst[a * ND_LD + j] += v[3 * a + j] + ((kind == 0 && a == j) ? lam : 0.0);
        };
#pragma unroll
        for (int u = 0; u < NE; ++u) {
            const int wr = tid + NTH * u < F.n_ent ? entry_row(En[u]) : -1;
            if (wr >= 0) put_entry(En[u], ev[u], wr);
        }
        for (int e = tid + NTH * NE; e < F.n_ent; e += NTH) {      // (fronts with more than 512 entries)
            const NdEnt E = N.ent[F.ent_off + e];
            const int wr = entry_row(E);
            if (wr < 0) continue;
            double t9[9];
            for (int a = 0; a < 9; ++a) t9[a] = N.ev[9 * (size_t)(F.ent_off + e) + a];
            put_entry(E, t9, wr);
        }
    }
    __syncthreads();
    stamp(2);
    // ---- panel factorisation of [F11; F21_I; F21_J] by 16-column steps.  Per step: (A) wave 0 factorises the diagonal block
    // while waves 1..3 apply the PREVIOUS panel to the block columns behind the next one; (B) every thread solves one panel row
    // against the block; (C) the next step's block column is updated by all four waves.  Every piece of code appears once.
    const int nb = s16 >> 4, nrt = nrow >> 4;
    int bad = 0;
    long long tA = 0, tB = 0, tq = 0;                              // (NRS_ND_DBG: time of wave 0 in steps A and B)
    if constexpr (W32) {
        // 32-column steps (round 5): blocks a and b = a + 1 per step.  Wave 0 runs the chain that cannot be shortened -- the diagonal block
        // of a, the sixteen panel rows of block b against it, their product into the diagonal block of b, the diagonal block of b --
        // and the other waves do everything else next to it: (P1) the two panels of the step before into block columns a and b, (P2) the
        // rows below block b against block a, (P3) those rows' product into block column b and the two panels of the step before into
        // the columns behind b, (P4, all waves) the rows against block b.  Four barriers per 32 columns as before, but the chain no longer waits for the rows and their products between its
        // two diagonal blocks.  Every tile sees the same operations in the same order as in the 16-column form: the same bits.
#pragma unroll 1
        for (int a = 0; a < nb; a += 2) {
            const int ka = 16 * a, b = a + 1, kbb = 16 * b;
            const bool pair = b < nb;
            if (N.clk) tq = wall_clock64();
            if (wave == 0) {                                       // P1
                if (a > 0) nd_update<2>(W, lane, ka - 32, a, a + 1, a + 1, 0, 1);
                nd_diag_factor(W, dinv, ka, lane, bad);
            } else if (a > 0) nd_update<2>(W, lane, ka - 32, a, min(a + 2, nb), nrt, wave - 1, NW - 1, 1);   // (block columns a and b only: the columns behind them get theirs in P3, next to the chain's second diagonal block)
            __syncthreads();
            if (N.clk) { const long long t = wall_clock64(); tA += t - tq; tq = t; }
            if (!pair) {                                           // (an odd last block: its rows, and done)
                if (ka + 16 + 64 * wave < nrow) nd_b_row(W, dinv, ka, min(ka + 16 + tid, nrow - 1), ka + 16 + tid < nrow, lane);
                __syncthreads();
                if (N.clk) tB += wall_clock64() - tq;
                break;
            }
            if (wave == 0) {                                       // P2: rows of block b against block a, then their product into (b, b)
                nd_b_row(W, dinv, ka, kbb + (lane & 15), lane < 16, lane);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                nd_update<1>(W, lane, ka, b, b + 1, b + 1, 0, 1);
            } else {
                const int row = kbb + 16 + (tid - 64);
                if (kbb + 16 + 64 * (wave - 1) < nrow) nd_b_row(W, dinv, ka, min(row, nrow - 1), row < nrow, lane);
            }
            __syncthreads();
            if (N.clk) { const long long t = wall_clock64(); tB += t - tq; tq = t; }
            if (wave == 0) nd_diag_factor(W, dinv, kbb, lane, bad);                                   // P3
            else {
                nd_update<1>(W, lane, ka, b, b + 1, nrt, wave - 1, NW - 1, 1);
                if (a > 0) nd_update<2>(W, lane, ka - 32, a + 2, nb, nrt, wave - 1, NW - 1, 0);
            }
            __syncthreads();
            if (N.clk) { const long long t = wall_clock64(); tA += t - tq; tq = t; }
            if (kbb + 16 + 64 * wave < nrow) nd_b_row(W, dinv, kbb, min(kbb + 16 + tid, nrow - 1), kbb + 16 + tid < nrow, lane);   // P4
            __syncthreads();
            if (N.clk) tB += wall_clock64() - tq;
        }
    } else
#pragma unroll 1
    for (int kb = 0; kb < nb; ++kb) {
        const int k0 = 16 * kb;
        if (N.clk) tq = wall_clock64();
        // (wave 0: the previous panel's update of THIS diagonal block, then its factorisation (A); waves 1..3 meanwhile apply the
        // previous panel to everything else right of it -- the rest of this block column included: only B is done by all four)
        if (wave == 0) {
            if (kb > 0) nd_update(W, lane, k0 - 16, kb, kb + 1, kb + 1, 0, 1);
            nd_diag_factor(W, dinv, k0, lane, bad);
        } else if (kb > 0) nd_update(W, lane, k0 - 16, kb, nb, nrt, wave - 1, NW - 1, 1);
        __syncthreads();
        if (N.clk) { const long long t = wall_clock64(); tA += t - tq; tq = t; }
        if (k0 + 16 + 64 * wave < nrow) {                          // (wave-uniform: the waves beyond the panel's rows stay out of the VALU's way)
            // (B) one panel row per thread: x L_kk^T = a, column by column.  L_kk sits in registers, row (lane & 15) in every 16-lane
            // row of the wave, and L[q][p] reaches the FMA through a DPP row broadcast: no LDS read inside the substitution
            // (it was 136 broadcast reads per thread: 1.07 -> 0.4 us per step).  Every lane computes; only the store is predicated.
            const int row = min(k0 + 16 + tid, nrow - 1), li = lane & 15;
            double x[16], lk[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) { x[q] = W[row * ND_LD + k0 + q]; lk[q] = W[(k0 + li) * ND_LD + k0 + q]; }
            double di[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) di[q] = dinv[k0 + q];
            nd_b_cols<0>(x, lk, di);
            if (k0 + 16 + tid < nrow) {
#pragma unroll
                for (int q = 0; q < 16; ++q) W[row * ND_LD + k0 + q] = x[q];
            }
        }
        __syncthreads();
        if (N.clk) tB += wall_clock64() - tq;
    }
    stamp(3);
    if (N.clk && tid == 0) { N.clk[8 * (size_t)(wg0 + blockIdx.x) + 6] = tA; N.clk[8 * (size_t)(wg0 + blockIdx.x) + 7] = tB; }
    // ---- Schur tile: U_IJ = F22_IJ - L21_I L21_J^T (k outermost: the wave's tiles advance together, operands of four k-steps in flight),
    // written into the parent's assembly slot at the parent's positions of its rows and columns (the lower one of the two)
    if (F.par >= 0 && !inv) {
        int ti[NT3], tj[NT3];
#pragma unroll
        for (int t3 = 0; t3 < NT3; ++t3) { const int t = min(wave + NW * t3, 8); ti[t3] = t / 3; tj[t3] = t - 3 * ti[t3]; }
        const bool last = wave + NW * (NT3 - 1) < 9;                // (tiles 0..8 over the waves: wave 0 has one more than the others)
#pragma unroll 1
        for (int k4 = 0; k4 < (s16 >> 4); ++k4) {
            double av[NT3][4], bv[NT3][4];
#pragma unroll
            for (int t3 = 0; t3 < NT3; ++t3)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    av[t3][kk] = -W[(rowI0 + 16 * ti[t3] + (lane & 15)) * ND_LD + 16 * k4 + 4 * kk + (lane >> 4)];
                    bv[t3][kk] = W[(rowJ0 + 16 * tj[t3] + (lane & 15)) * ND_LD + 16 * k4 + 4 * kk + (lane >> 4)];
                }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
                for (int t3 = 0; t3 < NT3 - 1; ++t3) acc[t3] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t3][kk], bv[t3][kk], acc[t3], 0, 0, 0);
                if (last) acc[NT3 - 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[NT3 - 1][kk], bv[NT3 - 1][kk], acc[NT3 - 1], 0, 0, 0);
            }
        }
        double* Ap = N.A + F.pA_off;
#pragma unroll
        for (int t3 = 0; t3 < NT3; ++t3) {
            if (wave + NW * t3 >= 9) break;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int r = 16 * ti[t3] + (lane >> 4) + 4 * g, cc = 16 * tj[t3] + (lane & 15);
                const int Cc = ND_TB * J + cc;
                if (r < rI && cc < cJ && Cc < F.b && (two || r >= cc)) {         // (a diagonal tile: its lower half)
                    const int PR = 3 * (int)pmi[r / 3] + r % 3, PC = 3 * (int)(two ? pmj : pmi)[cc / 3] + cc % 3;
                    Ap[(size_t)max(PR, PC) * F.pldA + min(PR, PC)] = acc[t3][g];  // ONE store per element: the parent reads lower positions only
                }
            }
        }
    }
    stamp(4);
    if (chained && !inv && F.par >= 0) {                           // this tile is in the parent's slot: count it (release: the stores first)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(N.fcnt + F.par, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (inv) {                                                     // (L11^-1)^T, upper triangular, behind the panel
        const int tx = tid & 31, ty = tid >> 5;
        double* LT = N.Lp + F.L_off + (size_t)(m + 2) * s;
        for (int r = ty; r < s; r += NTH / 32)
            for (int q = tx; q < s; q += 32) LT[(size_t)r * s + q] = q >= r ? W[(s16 + r) * ND_LD + q] : 0.0;
    }
    // ---- the factor: block I's rows of L21 (and y^T) by the DIAGONAL workgroups (I, I) -- those run in every form of a level, also when its
    // off-diagonal tiles come from k_nd_tile, which reads these rows back -- L11 and 1 / diag by (0, 0)
    if (J == I && !inv) {
        const int tx = tid & 31, ty = tid >> 5;
        double* L = N.Lp + F.L_off;
        for (int r = ty; r < rI; r += NTH / 32)
            for (int q = tx; q < s; q += 32) L[(size_t)(s + ND_TB * I + r) * s + q] = W[(rowI0 + r) * ND_LD + q];
        if (I == 0) {
            for (int p = ty; p < s; p += NTH / 32)
                for (int q = tx; q < s; q += 32) L[(size_t)p * s + q] = q <= p ? W[p * ND_LD + q] : 0.0;
            if (tid < s) L[(size_t)(m + 1) * s + tid] = dinv[tid];
            if (bad && lane == 0) N.flags[2] = 1;                  // (wave 0 saw the pivots)
        }
    }
    stamp(5);
}

// ---- the off-diagonal Schur tiles of a CROWDED level (more workgroups than CUs) in a launch of their own: U_IJ = F22_IJ - L21_I L21_J^T from the
// rows of L21 the diagonal workgroups (I, I), (J, J) of the launch before left in the factor -- instead of every (I, J) workgroup factorising
// the front's panel again for its one tile (13 us of panel for 4.4 us of tile, three rounds of workgroups at one per CU on the lowest level of
// a 4.4k-point frame).  Same operands, same matrix-core sequence, same accumulation order as k_nd_level's tile: the same bits.  LDS: two
// 48-row blocks (74 KB), two workgroups per CU.
constexpr int ND_TILE_LDS = 2 * ND_TB * ND_LD;                     // doubles
template <int NTH>
__global__ __launch_bounds__(NTH) void k_nd_tile(NdDev N, int wg0) {
    extern __shared__ double sm[];
    constexpr int NW = NTH / 64, NT3 = (9 + NW - 1) / NW;          // waves; tiles (of nine) per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const NdWgD wd = N.wg[wg0 + blockIdx.x];
    if (N.abort && *N.abort == N.abort_id) return;
    const int I = wd.I, J = wd.J;
    const NdFrontD& F = wd.F;
    const int s = F.s, s16 = (s + 15) & ~15, b1 = F.b + 1, m = s + F.b;
    const int rI = min(ND_TB, b1 - ND_TB * I), cJ = ND_TB;          // (J < I: a full block)
    double* LI = sm;
    double* LJ = sm + ND_TB * ND_LD;
    int16_t* pmi = reinterpret_cast<int16_t*>(sm + ND_TILE_LDS);
    int16_t* pmj = pmi + 16;
    auto stamp = [&](int k) { if (N.clk && tid == 0) N.clk[8 * (size_t)(wg0 + blockIdx.x) + k] = wall_clock64(); };
    stamp(0);
    if (tid < 16) { const int np = 16 * I + tid; pmi[tid] = np <= F.b / 3 ? N.pmap[F.pmap_off + np] : (int16_t)-1; }
    else if (tid < 32) { const int np = 16 * J + tid - 16; pmj[tid - 16] = np <= F.b / 3 ? N.pmap[F.pmap_off + np] : (int16_t)-1; }
    // requests first: the two row blocks of the factor (contiguous: rows of s doubles), then the children's slots of this tile
    const double* L = N.Lp + F.L_off;
    const double* srcI = L + (size_t)(s + ND_TB * I) * s;
    const double* srcJ = L + (size_t)(s + ND_TB * J) * s;
    constexpr int NL = (ND_TB * ND_S16 + NTH - 1) / NTH;           // values per thread and block at most (18 on 256 threads)
    double vi[NL], vj[NL];
#pragma unroll
    for (int u = 0; u < NL; ++u) {
        const int i = tid + NTH * u;
        vi[u] = i < rI * s ? srcI[i] : 0.0;
        vj[u] = i < cJ * s ? srcJ[i] : 0.0;
    }
    const size_t slot = (size_t)(m + 1) * F.ldA;
    const double* A0 = N.A + F.A_off;
    nd_v4d acc[NT3];
#pragma unroll
    for (int q = 0; q < NT3; ++q) acc[q] = nd_v4d{0.0, 0.0, 0.0, 0.0};
    if (F.n_ch > 0) {                                              // F22 tile (I, J) of the children, as in k_nd_level
        auto tile_off = [&](int r, int cc) {
            const int fr = s + ND_TB * I + r, fc = s + ND_TB * J + cc;
            return (size_t)max(fr, fc) * F.ldA + min(fr, fc);
        };
        double tv[2][NT3][4];
#pragma unroll
        for (int t3 = 0; t3 < NT3; ++t3) {
            const int t = wave + NW * t3, ti = t / 3, tj = t - 3 * ti;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int r = 16 * ti + (lane >> 4) + 4 * g, cc = 16 * tj + (lane & 15);
                const bool in = t < 9 && r < rI && cc < cJ && ND_TB * J + cc < F.b;
                const size_t o = in ? tile_off(r, cc) : 0;
                tv[0][t3][g] = A0[o];
                tv[1][t3][g] = A0[(F.n_ch > 1 ? slot : 0) + o];
                if (!in) { tv[0][t3][g] = 0.0; tv[1][t3][g] = 0.0; }
            }
        }
#pragma unroll
        for (int t3 = 0; t3 < NT3; ++t3)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[t3][g] = tv[0][t3][g] + (F.n_ch > 1 ? tv[1][t3][g] : 0.0);
        for (int k = 2; k < F.n_ch; ++k)
#pragma unroll
            for (int t3 = 0; t3 < NT3; ++t3) {
                const int t = wave + NW * t3, ti = t / 3, tj = t - 3 * ti;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int r = 16 * ti + (lane >> 4) + 4 * g, cc = 16 * tj + (lane & 15);
                    if (t < 9 && r < rI && cc < cJ && ND_TB * J + cc < F.b) acc[t3][g] += A0[k * slot + tile_off(r, cc)];
                }
            }
    }
    // into LDS at the panel's leading dimension; what the matrix cores read beyond the blocks (columns s .. s16, rows rI .. 48 of a partial
    // block I) is zero.  (row = i / s by a float reciprocal: (i + 0.5) / s is never closer than 0.5 / 96 to an integer)
    const float invs = 1.0f / (float)s;
#pragma unroll
    for (int u = 0; u < NL; ++u) {
        const int i = tid + NTH * u;
        const int r = __float2int_rz(((float)i + 0.5f) * invs), q = i - r * s;
        if (i < rI * s) LI[r * ND_LD + q] = vi[u];
        if (i < cJ * s) LJ[r * ND_LD + q] = vj[u];
    }
    for (int i = tid; i < ND_TB * (s16 - s); i += NTH) {            // pad columns of both blocks
        const int r = i / (s16 - s), q = s + i % (s16 - s);
        LI[r * ND_LD + q] = 0.0; LJ[r * ND_LD + q] = 0.0;
    }
    for (int i = tid; i < (ND_TB - rI) * s; i += NTH) LI[(rI + i / s) * ND_LD + i % s] = 0.0;   // rows below a partial block I
    __syncthreads();
    stamp(1); stamp(2); stamp(3);
    if (F.par >= 0) {
        int ti[NT3], tj[NT3];
#pragma unroll
        for (int t3 = 0; t3 < NT3; ++t3) { const int t = min(wave + NW * t3, 8); ti[t3] = t / 3; tj[t3] = t - 3 * ti[t3]; }
        const bool last = wave + NW * (NT3 - 1) < 9;
#pragma unroll 1
        for (int k4 = 0; k4 < (s16 >> 4); ++k4) {
            double av[NT3][4], bv[NT3][4];
#pragma unroll
            for (int t3 = 0; t3 < NT3; ++t3)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    av[t3][kk] = -LI[(16 * ti[t3] + (lane & 15)) * ND_LD + 16 * k4 + 4 * kk + (lane >> 4)];
                    bv[t3][kk] = LJ[(16 * tj[t3] + (lane & 15)) * ND_LD + 16 * k4 + 4 * kk + (lane >> 4)];
                }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
                for (int t3 = 0; t3 < NT3 - 1; ++t3) acc[t3] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t3][kk], bv[t3][kk], acc[t3], 0, 0, 0);
                if (last) acc[NT3 - 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[NT3 - 1][kk], bv[NT3 - 1][kk], acc[NT3 - 1], 0, 0, 0);
            }
        }
        double* Ap = N.A + F.pA_off;
#pragma unroll
        for (int t3 = 0; t3 < NT3; ++t3) {
            if (wave + NW * t3 >= 9) break;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int r = 16 * ti[t3] + (lane >> 4) + 4 * g, cc = 16 * tj[t3] + (lane & 15);
                const int Cc = ND_TB * J + cc;
                if (r < rI && cc < cJ && Cc < F.b) {
                    const int PR = 3 * (int)pmi[r / 3] + r % 3, PC = 3 * (int)pmj[cc / 3] + cc % 3;
                    Ap[(size_t)max(PR, PC) * F.pldA + min(PR, PC)] = acc[t3][g];
                }
            }
        }
    }
    stamp(4); stamp(5);
}

// back substitution, x_own = L11^-T (y - L21^T x_bnd), all levels in ONE launch: one workgroup per front (roots included: no
// boundary, nothing to wait for), top-down in block order.  A workgroup first brings everything that does not depend on the unknowns above it on chip -- (L11^-1)^T into LDS, L21
// into registers (the first 32 rows per thread group) and LDS (as many further rows as fit), y, output indices.  Its boundary is
// sorted by owner (NdFrontD::seg_off: the parent's unknowns first, the root's last), and the owners finish root first: the
// workgroup takes the segments from the far end, waits for each owner's unknowns (round 5: every thread polls the values it stages --
// agent-scope atomic loads past the caches -- until they are no longer the poison of this solve; NRS_ND_BACK_FLAGS=1: the owner's
// flag, release / acquire at agent scope) and adds that owner's part of L21^T x_bnd -- so whatever does not fit on chip (the tail of a large
// boundary: the oldest ancestors) is read from global memory while the nearer ancestors are still busy, and what is left when the
// parent publishes is its own segment out of registers / LDS, the product with (L11^-1)^T and the publication: ~5 us per level,
// no triangular solve, no global read of the factor on the critical path.  A workgroup only waits for one with a smaller block
// index (dispatched before it), so a full chip cannot deadlock; the wait is bounded all the same.
constexpr int ND_BACK_UR = 32;
__host__ __device__ inline int nd_back_fixed_doubles(int b) { return ND_S16 * ND_LD + 512 + 128 + ((b + 1) & ~1) + ((b / 3 + 2) >> 1); }
__global__ __launch_bounds__(256) void k_nd_back(NdDev N, int clk0, int n_fronts, int epoch, int lds_doubles) {
    extern __shared__ double sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = n_fronts - 1 - (int)blockIdx.x;
    const NdFrontD F = N.lvl_fr[li];                                // (descriptors in level order)
    const int s = F.s, b = F.b, m = s + b;
    if (blockIdx.x == 0 && tid == 0) { N.flags[1] = 1; __threadfence(); N.flags[0] = 1; }   // (read by the host after the launch has completed)
    // (no abort test in this launch: its workgroups wait for each other, and a discarded solve's back pass that lost some of them was measured
    // to fault; it runs to its end on whatever the drained factorisation left -- 60 us, nobody reads the result)
    double* Ls = sm;                                               // (L11^-1)^T, [s][ND_LD]
    double* part = Ls + ND_S16 * ND_LD;                            // [4][128]
    double* tv = part + 512;                                       // [128]: y - L21^T x_bnd
    double* xb = tv + 128;                                         // [b]
    int* bnode = reinterpret_cast<int*>(xb + ((b + 1) & ~1));      // [b / 3]: nodes of the boundary
    double* L21s = xb + ((b + 1) & ~1) + ((b / 3 + 2) >> 1);
    const double* L = N.Lp + F.L_off;
    auto stamp = [&](int k) { if (N.clk && tid == 0) N.clk[8 * (size_t)(clk0 + li) + k] = wall_clock64(); };
    stamp(0);
    // column q of L21 per thread, its rows dealt to 256 / SQ thread groups
    const int SQ = s <= 64 ? 64 : 128, ng = 256 / SQ;
    const int q = tid & (SQ - 1), g = tid / SQ;
    const int nreg = min(b, ng * ND_BACK_UR);                       // rows [0, nreg): registers; [nreg, nreg + nl): LDS; the rest (huge boundaries): global
    const int nl = max(0, min(b - nreg, (lds_doubles - nd_back_fixed_doubles(b)) / s));
    NdOut xo = {};
    if (wave == 0) xo = nd_out_request(N, F, lane);
    const double yq = tid < s ? L[(size_t)m * s + tid] : 0.0;
    for (int i = tid; i < b / 3; i += 256) bnode[i] = N.bnd[F.bnd_off + i];
    const double* Lq = L + (size_t)s * s + min(q, s - 1);
    double lr[ND_BACK_UR];
#pragma unroll
    for (int u = 0; u < ND_BACK_UR; ++u) lr[u] = Lq[(size_t)max(min(g + u * ng, b - 1), 0) * s];     // (a root has no boundary: the value is not used)
    {
        // (all requests of a staging step in flight together: a plain copy loop waits for every load before the next goes out --
        // 36 + 40 dependent round trips, 70 us for a front with a boundary of 70 nodes)
        const int tx = tid & 31, ty = tid >> 5;
        const double* LT = L + (size_t)(m + 2) * s;
        double v[12][3];
#pragma unroll
        for (int i = 0; i < 12; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int r = ty + 8 * i, p = tx + 32 * j;
                v[i][j] = (r < s && p < s && p >= r) ? LT[(size_t)r * s + p] : 0.0;
            }
#pragma unroll
        for (int i = 0; i < 12; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int r = ty + 8 * i, p = tx + 32 * j;
                if (r < s && p < s) Ls[r * ND_LD + p] = v[i][j];
            }
        const double* L2 = L + (size_t)(s + nreg) * s;              // (rows are contiguous; s is a multiple of 3, the panel offset of 2 doubles: 8-byte accesses)
        const int n = nl * s;
#pragma unroll 1
        for (int i0 = tid; i0 < n; i0 += 256 * 20) {
            double w[20];
#pragma unroll
            for (int u = 0; u < 20; ++u) w[u] = L2[min(i0 + 256 * u, n - 1)];
#pragma unroll
            for (int u = 0; u < 20; ++u) if (i0 + 256 * u < n) L21s[i0 + 256 * u] = w[u];
        }
    }
    stamp(5);
    double a8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int2* seg = reinterpret_cast<const int2*>(N.seg) + F.seg_off;
#pragma unroll 1
    for (int sg = F.n_seg - 1; sg >= 0; --sg) {
        const int2 S2 = seg[sg];
        const int r0 = sg > 0 ? seg[sg - 1].y : 0, r1 = S2.y;
        if (N.x_poll) {
            // every thread polls the unknowns it stages until they are there: no flag, no fence -- one memory round trip between an
            // ancestor's store and this front's products instead of three (its fence + flag, this front's poll, then the loads)
            if (sg == 0) stamp(4);
            for (int i = r0 + tid; i < r1; i += 256) {
                const double* src = N.xn + 3 * (size_t)bnode[i / 3] + i % 3;
                double v = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                int spins = 0;
                while ((unsigned long long)__double_as_longlong(v) == ND_POISON) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > (1 << 22)) { N.flags[2] = 2; break; }   // (cannot happen: ancestors are dispatched first; never hang the device)
                    v = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                xb[i] = v;
            }
            __syncthreads();
        } else {
        if (tid == 0) {
            int spins = 0;
            while (__hip_atomic_load(N.done + S2.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) {   // (plain polls: one acquire at the end)
                __builtin_amdgcn_s_sleep(1);
                if (++spins > (1 << 23)) { N.flags[2] = 2; break; }  // (cannot happen: ancestors are dispatched first; never hang the device)
            }
        }
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");         // (every thread, behind the barrier, as in k_nd_level: what the ancestor published is visible to all of them)
        if (sg == 0) stamp(4);
        for (int i = r0 + tid; i < r1; i += 256) xb[i] = __hip_atomic_load(N.xn + 3 * (size_t)bnode[i / 3] + i % 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        }
        if (sg == 0) stamp(1);
        if (q < s) {
            if (r0 < nreg) {
#pragma unroll
                for (int u = 0; u < ND_BACK_UR; ++u) { const int r = g + u * ng; if (r >= r0 && r < r1) a8[u & 7] += lr[u] * xb[r]; }
            }
            // this thread's rows in [max(r0, nreg), r1): r = g (mod ng)
            int r = max(r0, nreg);
            r += (g - r % ng + ng) % ng;
            const int e1 = min(r1, nreg + nl);
            for (; r + 3 * ng < e1; r += 4 * ng) {
#pragma unroll
                for (int u = 0; u < 4; ++u) a8[u] += L21s[(r + u * ng - nreg) * s + q] * xb[r + u * ng];
            }
            for (; r < e1; r += ng) a8[0] += L21s[(r - nreg) * s + q] * xb[r];
            for (; r < r1; r += 24 * ng) {                         // (rows beyond the chip: 24 requests in flight per thread)
                double l24[24];
#pragma unroll
                for (int u = 0; u < 24; ++u) l24[u] = Lq[(size_t)min(r + u * ng, b - 1) * s];
#pragma unroll
                for (int u = 0; u < 24; ++u) if (r + u * ng < r1) a8[u & 7] += l24[u] * xb[r + u * ng];
            }
        }
    }
    if (F.n_seg == 0) { stamp(4); stamp(1); }                      // (a root: nothing to wait for)
    {
        const double acc = ((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]));
        if (q < 128) {
            for (int gg = g; gg < 4; gg += ng) part[gg * 128 + q] = gg == g ? acc : 0.0;    // (unused group slots: zero)
        }
    }
    __syncthreads();
    if (tid < s) tv[tid] = yq - ((part[tid] + part[128 + tid]) + (part[256 + tid] + part[384 + tid]));
    __syncthreads();
    stamp(2);
    {
        // x = (L11^-1)^T t: row q2 per thread, the columns split over two thread halves (stride ND_LD: conflict-free)
        const int q2 = tid & 127, h = tid >> 7;
        double a0 = 0, a1 = 0;
        if (q2 < s) {
            const double* row = Ls + q2 * ND_LD;
            int p = h;
            for (; p + 2 < s; p += 4) { a0 += row[p] * tv[p]; a1 += row[p + 2] * tv[p + 2]; }
            for (; p < s; p += 2) a0 += row[p] * tv[p];
        }
        __syncthreads();                                           // (part is reused)
        part[h * 128 + q2] = a0 + a1;
    }
    __syncthreads();
    if (wave == 0) {
        const double x0 = lane < s ? part[lane] + part[128 + lane] : 0.0;          // unknowns 0..63 and 64..127 of the front, two per lane
        const double x1 = lane + 64 < s ? part[lane + 64] + part[128 + lane + 64] : 0.0;
        nd_store_x(N, F, xo, lane, x0, x1);
        if (!N.x_poll) {
            __threadfence();                                       // (this wave wrote the unknowns: its release publishes them)
            if (lane == 0) __hip_atomic_store(N.done + F.cmap_off, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    stamp(3);
}

// ---- entry values: a2's single-frame engines (K = 1) on the direct path ------------------------------------------------
// Nodes = the free rows (3 unknowns each) + the two halves of the pose block when the pose is free.  Per linearisation
// k_nd_values turns what the lineariser left (row diagonal blocks D, gradients, H_pp / b_p, the per-incidence factors of the
// springs and dampers, the 32-byte reprojection factors of the rows) into explicit blocks: the pair block of two coupled rows
// is -(sum qc v v^T + sum s I) over the edges that join them (v = x_i - x_j at the linearisation point, exactly what the
// factored operator of the PCG path applies), a pose-row block is J_p^T w J_l rebuilt from the row's fp32 projection Jacobian.
struct NdVals {                      // (NdPairD: nrs_nd_plan.hpp, next to NdEnt -- the host stage that fills it has no HIP)
    const int* node_row;             // node -> row (>= 0) or -1 - half
    const NdPairD* pair;
    const int* src;                  // (incidence slot << 1) | (0 spring, 1 damper)
    const NdEnt* ent;                // the plan's original entries; ev: 9 doubles each
    double* ev;
    int n_ent;
    // embedded mode: per entry the skinned observations that add to it (fixed order) with their weight products
    const int* ske_ptr; const int* ske_pt; const double* ske_coef;
};
static_assert(std::is_trivially_copyable_v<NdVals>, "passed to kernels by value: plain pointers, never an owner");

__device__ inline int nd_hpp_idx(int r, int cc) { return r * 6 - (r * (r - 1)) / 2 + (cc - r); }   // H_pp packed upper-triangular (r <= cc)

// one thread per original entry of the plan: its 3 x 3 block (or its 3 right-hand-side values) of the current linearisation.
// SK (embedded mode): ND_SKL lanes per entry -- all of them form the entry's own part (same addresses: one fetch), each adds up
// every ND_SKL-th skinned observation of the entry's list (a node is reached by ~N * 11 / M observations: ~100 at 5k x 500, a
// serial chain of dependent fetches for one thread) and the partial sums meet in a fixed butterfly: bit-reproducible
constexpr int ND_SKL = 8;
template <bool SK>
__global__ __launch_bounds__(256) void k_nd_values(Dev P, NdVals V) {
    const int tid = blockIdx.x * 256 + threadIdx.x;
    const int i = SK ? tid / ND_SKL : tid, sub = SK ? tid % ND_SKL : 0;
    if (i >= V.n_ent) return;
    const NdEnt E = V.ent[i];
    const uint32_t kind = E.src >> ND_KIND_SHIFT, idx = E.src & ND_SRC_MASK;
    double o[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int form = 0;                    // how the skinned observations add to this entry: 0 symmetric block (A), 1 gradient (c), 2 pose-row block (B_p), 3 none
    int half = 0;
    if (kind != 1) {
        const int row = V.node_row[idx];
        form = kind == 2 ? 1 : 0;
        if (row >= 0) {
            if (kind == 2) { o[0] = P.bl[3 * (size_t)row]; o[1] = P.bl[3 * (size_t)row + 1]; o[2] = P.bl[3 * (size_t)row + 2]; }
            else {
                const double* D = P.D + 6 * (size_t)row;
                o[0] = D[0]; o[1] = D[1]; o[2] = D[2]; o[3] = D[1]; o[4] = D[3]; o[5] = D[4]; o[6] = D[2]; o[7] = D[4]; o[8] = D[5];
            }
        } else {
            const int h = -1 - row;                                // half of the pose block (pose 0)
            form = 3;
            if (kind == 2) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    o[a] = P.bp[3 * h + a];
                    for (int b = 0; b < P.sk_nblk; ++b) o[a] += P.sk_part[(size_t)b * 32 + 21 + 3 * h + a];
                }
            } else {
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        const int k = nd_hpp_idx(3 * h + min(a, b), 3 * h + max(a, b));
                        o[3 * a + b] = P.Hpp[k];
                        for (int q = 0; q < P.sk_nblk; ++q) o[3 * a + b] += P.sk_part[(size_t)q * 32 + k];
                    }
            }
        }
    } else {
        const NdPairD q = V.pair[idx];
        if (q.kind == 0) {
            double v[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v[k] = P.lin_xl[3 * (size_t)q.a + k] - P.lin_xl[3 * (size_t)q.b + k];
                if (P.X0) v[k] = (P.lin_xl[3 * (size_t)q.a + k] + P.X0[3 * (size_t)q.a + k]) - (P.lin_xl[3 * (size_t)q.b + k] + P.X0[3 * (size_t)q.b + k]);
            }
            double qc = 0, sd = 0;
            for (int k = 0; k < q.nsrc; ++k) {
                const int sv = V.src[q.src0 + k];
                if (sv & 1) sd += P.d_s[sv >> 1]; else qc += P.s_qc[sv >> 1];
            }
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) o[3 * a + b] = -(qc * v[a] * v[b] + (a == b ? sd : 0.0));     // (symmetric: either orientation)
        } else if (q.kind == 1) {
            // H_{pose half, row} = J_p^T w J_l, J_l = -J R, J_p = -J [-[X_c]x | I] (reprojection_error_with_deformation.cc:52-68), as row_factored() forms them;
            // the pose is eliminated last, so the block's rows are the pose half's components
            form = 2; half = q.a;
            const RowRec rc = P.rowrec[q.b];
            const Pose Tcw = P.lin_pose[0];
            double R[9];
            quat_to_R(Tcw.q, R);
            double xs[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) xs[k] = P.lin_xl[3 * (size_t)q.b + k] + (P.X0 ? P.X0[3 * (size_t)q.b + k] : 0.0);
            const double px = R[0] * xs[0] + R[1] * xs[1] + R[2] * xs[2] + Tcw.t[0];
            const double py = R[3] * xs[0] + R[4] * xs[1] + R[5] * xs[2] + Tcw.t[1];
            const double pz = R[6] * xs[0] + R[7] * xs[1] + R[8] * xs[2] + Tcw.t[2];
            double Jl[2][3], Jp[2][3];
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const double j0 = -(double)rc.J[3 * rr], j1 = -(double)rc.J[3 * rr + 1], j2 = -(double)rc.J[3 * rr + 2];
                if (q.a == 0) { Jp[rr][0] = -j1 * pz + j2 * py; Jp[rr][1] = j0 * pz - j2 * px; Jp[rr][2] = -j0 * py + j1 * px; }
                else { Jp[rr][0] = j0; Jp[rr][1] = j1; Jp[rr][2] = j2; }
                Jl[rr][0] = j0 * R[0] + j1 * R[3] + j2 * R[6];
                Jl[rr][1] = j0 * R[1] + j1 * R[4] + j2 * R[7];
                Jl[rr][2] = j0 * R[2] + j1 * R[5] + j2 * R[8];
            }
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) o[3 * a + b] = rc.w * (Jp[0][a] * Jl[0][b] + Jp[1][a] * Jl[1][b]);
        } else {
            form = 3;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) {                       // rows: the second half of the pose block
                    const int k = nd_hpp_idx(b, 3 + a);
                    o[3 * a + b] = P.Hpp[k];
                    for (int q2 = 0; q2 < P.sk_nblk; ++q2) o[3 * a + b] += P.sk_part[(size_t)q2 * 32 + k];
                }
        }
    }
    if (SK) {                                                      // the skinned observations that reach this entry: every ND_SKL-th, in list order
        double p[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        const int t1 = form != 3 ? V.ske_ptr[i + 1] : 0;
        for (int t = form != 3 ? V.ske_ptr[i] + sub : 0; t < t1; t += ND_SKL) {
            const double* rec = P.sk_rec + 27 * (size_t)V.ske_pt[t];
            const double cf = V.ske_coef[t];
            if (form == 0) {
                p[0] += cf * rec[0]; p[1] += cf * rec[1]; p[2] += cf * rec[2]; p[3] += cf * rec[1]; p[4] += cf * rec[3]; p[5] += cf * rec[4];
                p[6] += cf * rec[2]; p[7] += cf * rec[4]; p[8] += cf * rec[5];
            } else if (form == 1) { p[0] += cf * rec[6]; p[1] += cf * rec[7]; p[2] += cf * rec[8]; }
            else {
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) p[3 * a + b] += cf * rec[9 + 3 * (3 * half + a) + b];
            }
        }
#pragma unroll
        for (int off = 1; off < ND_SKL; off <<= 1)                  // (x + y on both partners: every lane ends with the same bits)
#pragma unroll
            for (int a = 0; a < 9; ++a) p[a] += __shfl_xor(p[a], off, 64);
#pragma unroll
        for (int a = 0; a < 9; ++a) o[a] += p[a];
        if (sub != 0) return;
    }
    double* out = V.ev + 9 * (size_t)i;
#pragma unroll
    for (int a = 0; a < 9; ++a) out[a] = o[a];
    if (P.sk_n > 0 && kind == 2) {
        // the gradient with the skinned observations' part goes back into the engine's vectors: computeScale = x . (lambda x + b)
        // (optimization_algorithm_levenberg.cpp:167-174, k_apply) is over the whole b
        const int row = V.node_row[idx];
        double* g = row >= 0 ? P.bl + 3 * (size_t)row : P.bp + 3 * (-1 - row);
        g[0] = o[0]; g[1] = o[1]; g[2] = o[2];
    }
    if (P.sk_n > 0 && kind == 0)                                   // lambda_0 = 1e-5 max |diag H| (optimization_algorithm_levenberg.cpp:153-165) sees the added blocks
        atomicMax(reinterpret_cast<unsigned long long*>(P.sk_maxdiag), (unsigned long long)__double_as_longlong(fmax(fabs(o[0]), fmax(fabs(o[4]), fabs(o[8])))));
}

}  // namespace nrs
