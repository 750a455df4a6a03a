// Window-edge construction on the device (part of nrs_engine.hip): the edge lists of LocalDeformableBundleAdjustment from the caller's
// neighbour lists or from the resident graph's, for nrs_dba_solve_window and nrs_dba_solve_window_rg; nrs_engine_embwin.hpp walks the
// same lists (WinDev, WinLists) for embedded windows.  The scratch plans: nrs_devpack_host.hpp.
#pragma once
#include <rocprim/rocprim.hpp>
#include "nrs_devpack_host.hpp"

namespace nrs {

// ---- edge construction of LocalDeformableBundleAdjustment on the device (OPT:927-1137; the host form is nrs_dba_build_edges,
// csrc/nrs_host_build.cpp, whose output this reproduces index for index).  One WAVE per landmark l = (keyframe k, map point p):
// it walks p's ordered neighbour list as the reference does (stop after more than 10 regularisers or at the first BAD
// connection, OPT:1033-1050; a duplicate counts as a regulariser too, so the walked prefix of a point does not depend on any
// other point), 64 contiguous entries at a time as k_rg_walk does: the regularisers before an entry are a prefix count over the
// lanes, the entry at which the sequential loop breaks is the first lane that sees it.  The reference's per-keyframe hash sets
// (SpatialPoint / TemporalPoint, OPT:980-981) keep the FIRST of the two walks that propose a pair: the pair {p, o} is a duplicate
// here iff o comes earlier in the keyframe and o's own walk reaches p (each lane follows the walk of its own o).
// The lists come in one of two layouts (WinLists): the caller's CSR (nrs_dba_solve_window), or the fixed-stride prefixes
// k_rg_get_edges leaves on the device, found through a point -> list-row table (nrs_dba_solve_window_rg).  A prefix may be CUT
// (count > stride): a walk RAN OFF when it comes to the end of a cut prefix without having met a BAD entry and with no more than 10
// regularisers counted -- the entries behind the prefix could still add to it.  (With more than 10 counted, the next entry would
// end the walk before it had any effect, whatever it is; a list that is complete never runs off.)
struct WinLists {
    const int* rowptr;                                               // CSR: the list of p is [rowptr[p], rowptr[p + 1]); null: fixed stride
    const int *row, *count;                                          // fixed stride: row[p] = list row of p (-1: not in the window), count[row] = FULL length
    int stride;
    const int *col, *status;
    const float *w, *d0;
    __device__ void range(int p, int64_t& lo, int& n, bool& cut) const {
        if (rowptr) { lo = rowptr[p]; n = rowptr[p + 1] - rowptr[p]; cut = false; return; }
        const int r = row[p], c = count[r];
        lo = (int64_t)r * stride; n = min(c, stride); cut = c > stride;
    }
};
struct WinDev {
    int n_kf, n_points;
    const int *kf_rowptr, *kf_pt, *lm_k;                             // lm_k[l] = keyframe of landmark l
    WinLists L;
    const int* cur;                                                  // n_kf x n_points: landmark of (k, p) or -1
};

// (a cut prefix that ends before p is reached: false -- o's own walk has then run off and is flagged by the count pass)
__device__ inline bool win_walk_reaches(const WinDev& W, int k, int o, int p, bool damper) {
    const int* cur = W.cur + (size_t)k * W.n_points;
    const int* nxt = damper ? W.cur + (size_t)(k + 1) * W.n_points : nullptr;
    int64_t lo; int n; bool cut;
    W.L.range(o, lo, n, cut);
    int n_reg = 0;
    for (int64_t e = lo; e < lo + n; ++e) {
        if (n_reg > 10 || W.L.status[e] == NRS_GRAPH_BAD) return false;
        const int x = W.L.col[e];
        if (cur[x] < 0 || (damper && nxt[x] < 0)) continue;
        if (x == p) return true;
        ++n_reg;
    }
    return false;
}

// one walk of landmark l by its wave: DAMPER = false the springs (OPT:1033-1074), true the dampers with the next keyframe
// (OPT:1086-1135).  Returns the number of edges it makes (wave-uniform); *ran_off: see above.  EMIT writes them from `off` on.
template <bool EMIT, bool DAMPER>
__device__ inline int win_walk(const WinDev& W, int l, int k, int p, int lane, int off, int* sp_ij, float* sp_d0, int* dm_idx, float* dm_w, bool* ran_off) {
    const int* cur = W.cur + (size_t)k * W.n_points;
    const int* nxt = DAMPER ? W.cur + (size_t)(k + 1) * W.n_points : nullptr;
    int64_t lo; int n; bool cut;
    W.L.range(p, lo, n, cut);
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    int n_reg = 0, n_out = 0;
    bool broke = false;
    for (int ch = 0; ch < n && !broke; ch += 64) {
        const int a = ch + lane;
        const bool valid = a < n;
        const int64_t e = lo + a;
        const int o = valid ? W.L.col[e] : 0;
        const bool bad = valid && W.L.status[e] == NRS_GRAPH_BAD;
        const bool pres = valid && cur[o] >= 0 && (!DAMPER || nxt[o] >= 0);      // the other end is observed (by both keyframes)
        const unsigned long long presm = __ballot(pres);
        const int before = n_reg + __popcll(presm & below);         // regularisers counted when the loop comes to this entry
        const unsigned long long brkm = __ballot(valid && (bad || before > 10));
        const int fb = brkm ? __ffsll((long long)brkm) - 1 : 64;    // the loop breaks at this lane's entry
        bool make = pres && lane < fb;
        if (make && cur[o] < l && win_walk_reaches(W, k, o, p, DAMPER)) make = false;   // inserted by o's walk already
        const unsigned long long makem = __ballot(make);
        if (EMIT && make) {
            const size_t q = (size_t)off + n_out + __popcll(makem & below);
            if (!DAMPER) { sp_ij[2 * q] = l; sp_ij[2 * q + 1] = cur[o]; sp_d0[q] = W.L.d0[e]; }
            else { dm_idx[4 * q] = l; dm_idx[4 * q + 1] = cur[o]; dm_idx[4 * q + 2] = nxt[p]; dm_idx[4 * q + 3] = nxt[o]; dm_w[q] = W.L.w[e]; }
        }
        n_out += __popcll(makem);
        n_reg += __popcll(fb < 64 ? presm & ((1ull << fb) - 1ull) : presm);
        broke = fb < 64;
    }
    *ran_off = cut && !broke && n_reg <= 10;
    return n_out;
}

// EMIT = false: counts per landmark, and in flag[0] the walks that ran off, in flag[1] the smallest map point one of them started
// from (integer atomics of the count pass only; initialised to 0 / INT_MAX); true: writes at the scanned offsets
template <bool EMIT>
__global__ __launch_bounds__(256) void k_win_edges(WinDev W, int n_lm, int* cnt_s, int* cnt_d, const int* __restrict__ off_s, const int* __restrict__ off_d,
                                                   int* sp_ij, float* sp_d0, int* dm_idx, float* dm_w, int* flag) {
    const int lane = threadIdx.x & 63, l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= n_lm) return;                                           // (wave-uniform)
    const int k = W.lm_k[l], p = W.kf_pt[l];
    bool off_end = false;
    int n_ran = 0;
    const int ns = win_walk<EMIT, false>(W, l, k, p, lane, EMIT ? off_s[l] : 0, sp_ij, sp_d0, dm_idx, dm_w, &off_end);
    n_ran += off_end;
    int nd = 0;
    if (k + 1 < W.n_kf && W.cur[(size_t)(k + 1) * W.n_points + p] >= 0) {
        nd = win_walk<EMIT, true>(W, l, k, p, lane, EMIT ? off_d[l] : 0, sp_ij, sp_d0, dm_idx, dm_w, &off_end);
        n_ran += off_end;
    }
    if (!EMIT && lane == 0) {
        cnt_s[l] = ns; cnt_d[l] = nd;
        if (n_ran) { atomicAdd(&flag[0], n_ran); atomicMin(&flag[1], p); }
    }
}
__global__ void k_win_cur(int n_lm, const int* __restrict__ lm_k, const int* __restrict__ kf_pt, int n_points, int* cur) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l < n_lm) atomicMax(&cur[(size_t)lm_k[l] * n_points + kf_pt[l]], l);   // (a map point listed twice in a keyframe: the last entry wins, as on the host)
}
// the window's distinct map points: mark[p] = 1 where a landmark observes p; after the scan, ids[] ascending and the point -> row table
__global__ void k_win_mark(int n_lm, const int* __restrict__ kf_pt, int* mark) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l < n_lm) mark[kf_pt[l]] = 1;
}
__global__ void k_win_rows(int n_points, const int* __restrict__ mark, const int* __restrict__ pos, int* ids, int* row) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_points) return;
    row[p] = mark[p] ? pos[p] : -1;
    if (mark[p]) ids[pos[p]] = p;
}

// temporary storage of an exclusive scan over n ints: rocPRIM's own figure and 256 bytes (the scratch plans take it as a number)
static size_t win_scan_tmp_bytes(nrs_ctx* c, size_t n) {
    size_t tb = 0;
    (void)rocprim::exclusive_scan(nullptr, tb, (int*)nullptr, (int*)nullptr, 0, n, rocprim::plus<int>(), c->stream);
    return tb + 256;
}

// A window as its caller holds it: the landmarks of n_kf keyframes and, for the CSR form, the neighbour lists of n_points map points
// (nbr_*: null when the resident graph serves the lists; n_points is then its capacity).
struct WinIn {
    int n_kf; const int *kf_rowptr, *kf_pt, *lm_kf;
    int n_points; const int *nbr_rowptr, *nbr_col; const float *nbr_w, *nbr_d0; const int* nbr_status;
};

// The count pass of a window's walks (`count` launches it over wd: k_win_edges<false> here, k_ew_walk_wave<false> in nrs_engine_embwin.hpp;
// both add the walks that ran off into d_flag).  The CSR form (g = null): once.  The resident graph's lists: first at `cap` entries per
// point, then at twice as many for as long as a walk runs off, cap_max at the most -- beyond it the run-off is an error in the name of `who`.
struct WinRounds { int cap, rounds, ran_first; };                  // the cap that served, the passes, the walks that ran off in the first
template <class Count>
static int win_count_rounds(nrs_ctx* c, nrs_rgraph* g, WinDev& wd, int n_ids, const int* d_ids, const int* d_row, int* d_flag, int cap, int cap_max, const char* who,
                            Count&& count, WinRounds* out) {
    hipStream_t st = c->stream;
    int rounds = 0, ran_first = 0;
    for (;;) {
        if (g) {
            RgDeviceLists rl;
            NRS_TRY(rg_get_edges_device(g, n_ids, d_ids, cap, &rl));
            wd.L = WinLists{nullptr, d_row, rl.count, rl.stride, rl.col, rl.status, rl.w, rl.d0};
        }
        ++rounds;
        const int flag0[2] = {0, 0x7FFFFFFF};
        NRS_HIP(c, hipMemcpyAsync(d_flag, flag0, sizeof(flag0), hipMemcpyHostToDevice, st));
        count();
        NRS_HIP(c, hipGetLastError());
        int flag[2] = {0, 0};
        NRS_HIP(c, hipMemcpyAsync(flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, st));     // the round's one flag read
        NRS_HIP(c, hipStreamSynchronize(st));
        if (flag[0] == 0) break;
        if (rounds == 1) ran_first = flag[0];
        if (cap >= cap_max)
            return c->fail(NRS_ERR_INVALID, "%s: the neighbour walk of map point %d ran off its list at the limit of %d entries per point", who, flag[1], cap_max);
        cap = std::min(cap_max, 2 * cap);
    }
    *out = WinRounds{cap, rounds, ran_first};
    return NRS_OK;
}

// Builds the edge lists of a window on the device; the arrays live in the context's third and fourth scratch buffers until the next call.
// g = null: the caller's CSR lists.  g: the resident graph serves them, from `cap` entries per point on (win_count_rounds).
static int win_edges_device(nrs_ctx* c, const WinIn& in, nrs_rgraph* g, int cap, int64_t* stats, DevEdges* out) {
    const int n_kf = in.n_kf, n_points = in.n_points, n_lm = in.kf_rowptr[n_kf], nnz = g ? 0 : in.nbr_rowptr[n_points];
    hipStream_t st = c->stream;
    const size_t tmp_bytes = win_scan_tmp_bytes(c, (size_t)std::max(n_lm, g ? n_points : 0) + 1);
    // ---- scratch and uploads
    const auto P = dp_winedge_plan(DpWinEdgeIn{(size_t)n_kf, (size_t)n_lm, (size_t)n_points, (size_t)nnz, tmp_bytes, g != nullptr});
    NRS_TRY(c->ensure(c->pack_ws3, P.need));
    char* const w3 = c->pack_ws3.as<char>();
    int *d_rowptr = P.at<int>(w3, WE_rowptr), *d_pt = P.at<int>(w3, WE_pt), *d_k = P.at<int>(w3, WE_k), *d_nrp = P.at<int>(w3, WE_nrp), *d_col = P.at<int>(w3, WE_col),
        *d_st = P.at<int>(w3, WE_st), *d_cur = P.at<int>(w3, WE_cur), *d_cs = P.at<int>(w3, WE_cs), *d_cd = P.at<int>(w3, WE_cd), *d_os = P.at<int>(w3, WE_os),
        *d_od = P.at<int>(w3, WE_od), *d_mark = P.at<int>(w3, WE_mark), *d_pos = P.at<int>(w3, WE_pos), *d_ids = P.at<int>(w3, WE_ids), *d_row = P.at<int>(w3, WE_row),
        *d_flag = P.at<int>(w3, WE_flag);
    float *d_w = P.at<float>(w3, WE_w), *d_d0 = P.at<float>(w3, WE_d0);
    void* tmp = P.at<char>(w3, WE_tmp);
    NRS_HIP(c, hipMemcpyAsync(d_rowptr, in.kf_rowptr, sizeof(int) * (n_kf + 1), hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(d_pt, in.kf_pt, sizeof(int) * (size_t)n_lm, hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(d_k, in.lm_kf, sizeof(int) * (size_t)n_lm, hipMemcpyHostToDevice, st));
    if (!g) {
        NRS_HIP(c, hipMemcpyAsync(d_nrp, in.nbr_rowptr, sizeof(int) * ((size_t)n_points + 1), hipMemcpyHostToDevice, st));
        NRS_HIP(c, hipMemcpyAsync(d_col, in.nbr_col, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice, st));
        NRS_HIP(c, hipMemcpyAsync(d_st, in.nbr_status, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice, st));
        NRS_HIP(c, hipMemcpyAsync(d_w, in.nbr_w, sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice, st));
        NRS_HIP(c, hipMemcpyAsync(d_d0, in.nbr_d0, sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice, st));
    }
    NRS_HIP(c, hipMemsetAsync(d_cur, 0xFF, sizeof(int) * (size_t)n_kf * n_points, st));
    NRS_HIP(c, hipMemsetAsync(d_cs + n_lm, 0, sizeof(int), st));
    NRS_HIP(c, hipMemsetAsync(d_cd + n_lm, 0, sizeof(int), st));
    const dim3 g1((unsigned)((n_lm + 255) / 256)), gw((unsigned)((n_lm + 3) / 4)), b(256);   // a thread / a wave per landmark
    hipLaunchKernelGGL(k_win_cur, g1, b, 0, st, n_lm, d_k, d_pt, n_points, d_cur);
    int n_ids = 0;
    if (g) {                                                        // the distinct map points, ascending, and the point -> list-row table
        NRS_HIP(c, hipMemsetAsync(d_mark, 0, sizeof(int) * ((size_t)n_points + 1), st));
        hipLaunchKernelGGL(k_win_mark, g1, b, 0, st, n_lm, d_pt, d_mark);
        size_t t1 = tmp_bytes;
        NRS_HIP(c, rocprim::exclusive_scan(tmp, t1, d_mark, d_pos, 0, (size_t)n_points + 1, rocprim::plus<int>(), st));
        hipLaunchKernelGGL(k_win_rows, dim3((unsigned)((n_points + 255) / 256)), b, 0, st, n_points, d_mark, d_pos, d_ids, d_row);
        NRS_HIP(c, hipGetLastError());
        NRS_HIP(c, hipMemcpyAsync(&n_ids, d_pos + n_points, sizeof(int), hipMemcpyDeviceToHost, st));
        NRS_HIP(c, hipStreamSynchronize(st));
        if (n_ids <= 0 || n_ids > n_points) return c->fail(NRS_ERR_STATE, "nrs_dba_solve_window_rg: %d distinct map points", n_ids);
    }
    // ---- count pass, scans
    const int cap_max = g ? rg_max_cap_per_point(g) : 0;
    WinDev wd{n_kf, n_points, d_rowptr, d_pt, d_k, WinLists{d_nrp, nullptr, nullptr, 0, d_col, d_st, d_w, d_d0}, d_cur};
    WinRounds wr;
    NRS_TRY(win_count_rounds(c, g, wd, n_ids, d_ids, d_row, d_flag, std::min(cap, cap_max), cap_max, "nrs_dba_solve_window_rg", [&] {
        hipLaunchKernelGGL((k_win_edges<false>), gw, b, 0, st, wd, n_lm, d_cs, d_cd, (const int*)nullptr, (const int*)nullptr, (int*)nullptr, (float*)nullptr, (int*)nullptr, (float*)nullptr, d_flag);
    }, &wr));
    if (stats) { stats[0] = n_ids; stats[1] = wr.cap; stats[2] = wr.rounds; stats[3] = wr.ran_first; }
    int tot[2] = {0, 0};
    size_t t2 = tmp_bytes;
    NRS_HIP(c, rocprim::exclusive_scan(tmp, t2, d_cs, d_os, 0, (size_t)n_lm + 1, rocprim::plus<int>(), st));
    t2 = tmp_bytes;
    NRS_HIP(c, rocprim::exclusive_scan(tmp, t2, d_cd, d_od, 0, (size_t)n_lm + 1, rocprim::plus<int>(), st));
    NRS_HIP(c, hipMemcpyAsync(&tot[0], d_os + n_lm, sizeof(int), hipMemcpyDeviceToHost, st));
    NRS_HIP(c, hipMemcpyAsync(&tot[1], d_od + n_lm, sizeof(int), hipMemcpyDeviceToHost, st));
    NRS_HIP(c, hipStreamSynchronize(st));
    // ---- emit pass into the output buffer
    const auto O = dp_winout_plan((size_t)tot[0], (size_t)tot[1]);
    NRS_TRY(c->ensure(c->pack_ws4, O.need));
    char* const w4 = c->pack_ws4.as<char>();
    int *sp_ij = O.at<int>(w4, WO_sp_ij), *dm_idx = O.at<int>(w4, WO_dm_idx);
    float *sp_d0 = O.at<float>(w4, WO_sp_d0), *dm_w = O.at<float>(w4, WO_dm_w);
    hipLaunchKernelGGL((k_win_edges<true>), gw, b, 0, st, wd, n_lm, (int*)nullptr, (int*)nullptr, d_os, d_od, sp_ij, sp_d0, dm_idx, dm_w, (int*)nullptr);
    NRS_HIP(c, hipGetLastError());
    out->n_sp = tot[0]; out->n_dm = tot[1];
    out->sp_ij = sp_ij; out->sp_d0 = sp_d0; out->dm_idx = dm_idx; out->dm_w = dm_w;
    return NRS_OK;
}
int engine_build_edges_device(nrs_ctx* c, int n_kf, const int* kf_rowptr, const int* kf_pt, const int* lm_kf, int n_points, const int* nbr_rowptr,
                              const int* nbr_col, const float* nbr_w, const float* nbr_d0, const int* nbr_status, DevEdges* out) {
    return win_edges_device(c, WinIn{n_kf, kf_rowptr, kf_pt, lm_kf, n_points, nbr_rowptr, nbr_col, nbr_w, nbr_d0, nbr_status}, nullptr, 0, nullptr, out);
}
int engine_build_edges_device_rg(nrs_ctx* c, int n_kf, const int* kf_rowptr, const int* kf_pt, const int* lm_kf, nrs_rgraph* g, int cap_per_point,
                                 DevEdges* out, int64_t stats[4]) {
    return win_edges_device(c, WinIn{n_kf, kf_rowptr, kf_pt, lm_kf, rg_capacity(g), nullptr, nullptr, nullptr, nullptr, nullptr}, g, cap_per_point, stats, out);
}

int engine_edges_to_host(nrs_ctx* c, Engine* e, int* sp_ij, float* sp_d0, int* dm_idx, float* dm_w) {
    if (!e->dev_edges) return c->fail(NRS_ERR_STATE, "the resident problem keeps its edges on the host");
    const Dev& d = e->d;
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    if (sp_ij) NRS_HIP(c, hipMemcpy(sp_ij, e->raw_sp, sizeof(int) * 2 * (size_t)d.n_sp, hipMemcpyDeviceToHost));
    if (sp_d0) NRS_HIP(c, hipMemcpy(sp_d0, e->raw_d0, sizeof(float) * (size_t)d.n_sp, hipMemcpyDeviceToHost));
    if (dm_idx) NRS_HIP(c, hipMemcpy(dm_idx, e->raw_dm, sizeof(int) * 4 * (size_t)d.n_dm, hipMemcpyDeviceToHost));
    if (dm_w) NRS_HIP(c, hipMemcpy(dm_w, e->raw_w, sizeof(float) * (size_t)d.n_dm, hipMemcpyDeviceToHost));
    return NRS_OK;
}

}  // namespace nrs
