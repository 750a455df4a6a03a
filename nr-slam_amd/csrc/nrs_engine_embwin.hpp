// Device-side list construction of the EMBEDDED BA window (part of nrs_engine.hip; include/nrs.h nrs_dba_solve_window_embedded).
//
// The host form is nrs_dba_build_edges_embedded (csrc/nrs_host_build.cpp), whose output this reproduces index for index and bit
// for bit, the fp64 skinning weights included.  It is the per-observation walk of k_win_edges (nrs_engine_winedges.hpp) with two
// additions: the walks run between NODE copies only, and every observed point that is not a node is bound to the <= 11 node
// copies its own walk accepts.
//   numbering   a node copy is an observation whose map point has is_node set; node copies are numbered keyframe by keyframe in
//               observation order: an exclusive scan of the flag over the concatenation kf_pt.  The n_kf x n_points table `cur`
//               holds the node-copy index of (keyframe, map point) or -1; map points that are not nodes stay -1, so every walk
//               passes over them exactly as over a point the keyframe does not observe
//   walks       one thread per observation, count pass / exclusive scans / emit pass (as engine_build_edges_device).  A node copy
//               emits its springs and its dampers with the next keyframe (stop rule and duplicate rule of k_win_edges: the pair is
//               a duplicate iff the other node copy comes earlier in the keyframe and its own walk reaches this point; a duplicate
//               still counts as a regulariser).  Any other observation accepts at most 11 node copies of its keyframe, widens their
//               float weights to double, sums them in walk order and divides each by the sum; one that reaches no node copy emits
//               nothing.  Skinned observations keep observation order (their slot: a scan of the per-observation count)
//   gathers     lm_xyz / lm_uv / lm_kf of the node copies and sk_xyz / sk_uv / sk_kf of the skinned observations from the
//               caller's per-observation arrays
// DUPLICATE MAP POINTS.  The host walk and a parallel walk differ when a map point is listed twice in one keyframe: the host's table
// changes while it walks the keyframe, this one is complete before any walk starts.  The reference cannot produce the case
// (frame.h:108-123 maps id to index one to one), so it is detected here and reported (*duplicate = true; the entry point returns
// NRS_ERR_INVALID before any solver launch): a node copy whose own index is not the one left in `cur` is such a duplicate.
// SHARDED WINDOWS.  Every rank of a communicator runs this on its own device over identical inputs.  Numbering, `cur`, the duplicate
// check, the count pass and the scans cover the whole window (cheap; every rank gets the same counts and the same slots); with the
// totals come the node-copy and skinned-observation offsets at the keyframe boundaries (k_ew_kf_bounds), from which the rank takes its
// keyframes [k0, k1) -- the set-up's own shard_plan call on the per-keyframe node-copy counts (embwin_own_range) -- and the slice
// [sk_base, sk_base + sk_held) of the skinned list that belongs to them (observations are in keyframe order, so is the list).  Node
// copies, springs, dampers and sk_obs (4 bytes an observation: the caller's scatter goes through it) are emitted whole; sk_node,
// sk_omega, sk_xyz, sk_uv and sk_kf -- 156 of the 160 bytes of a skinned observation -- for the slice only, at slot - sk_base.  The blob,
// its device scratch and the pinned staging are sized from sk_held.
// RESIDENT GRAPH.  nrs_dba_solve_window_rg_embedded takes the lists from the device-resident all-pairs graph instead of the caller: the same
// walks by k_ew_walk_wave, a wave per observation over fixed-stride prefixes, in the doubling rounds of nrs_engine_winedges.hpp; every
// stage around the two walk kernels is shared (ew_begin / ew_number / ew_finish).
// The lists end up in pinned host memory of the context (one copy back), laid out by embwin_layout, and are handed to the set-up
// nrs_dba_upload_embedded runs (nrs_engine_setup.hpp reads host arrays).  Plain C++ and vector stores only; the atomics are the
// atomicMax on `cur`, as in k_win_cur, and the two integer atomics of the ran-off flag in k_ew_walk_wave's count pass.
#pragma once

namespace nrs {

// byte offsets of the 14 arrays of an EmbWindow in one blob (device scratch, pinned mirror and host storage share the layout)
enum { EW_SK_OMEGA, EW_LM_OBS, EW_SP_IJ, EW_SP_D0, EW_DM_IDX, EW_DM_W, EW_SK_OBS, EW_SK_NODE, EW_LM_XYZ, EW_LM_UV, EW_LM_KF, EW_SK_XYZ, EW_SK_UV, EW_SK_KF, EW_N };
// (sk_obs has the window's n_skin entries, the other skinned arrays the sk_held entries of this blob: all of them, or a rank's slice)
static size_t embwin_layout(int n_lm, int n_sp, int n_dm, int n_skin, int sk_held, size_t off[EW_N], size_t* sk_bytes = nullptr) {
    const size_t bytes[EW_N] = {88 * (size_t)sk_held, 4 * (size_t)n_lm, 8 * (size_t)n_sp, 4 * (size_t)n_sp, 16 * (size_t)n_dm, 4 * (size_t)n_dm, 4 * (size_t)n_skin,
                                44 * (size_t)sk_held, 12 * (size_t)n_lm, 8 * (size_t)n_lm, 4 * (size_t)n_lm, 12 * (size_t)sk_held, 8 * (size_t)sk_held, 4 * (size_t)sk_held};
    size_t o = 0, sk = 0;
    for (int i = 0; i < EW_N; ++i) {
        const size_t b = ((bytes[i] + 255) / 256) * 256 + 256;
        off[i] = o; o += b;
        if (i == EW_SK_OMEGA || i == EW_SK_NODE || i == EW_SK_XYZ || i == EW_SK_UV || i == EW_SK_KF) sk += b;
    }
    if (sk_bytes) *sk_bytes = sk;
    return o;
}
size_t embwin_bytes(int n_lm, int n_sp, int n_dm, int n_skin, int sk_held) {
    size_t off[EW_N];
    return embwin_layout(n_lm, n_sp, n_dm, n_skin, sk_held, off);
}
void embwin_own_range(int n_kf, const int* kf_nodes, int world, int rank, int* k0, int* k1) {
    std::vector<int> grp(n_kf + 1, 0), kb(world + 1, 0);
    for (int k = 0; k < n_kf; ++k) grp[k + 1] = grp[k] + std::max(1, (kf_nodes[k] + ROW_ALIGN - 1) / ROW_ALIGN);   // (pose_grp_ptr of the set-up)
    shard_plan(n_kf, grp.data(), world, kb.data());
    *k0 = kb[rank]; *k1 = kb[rank + 1];
}
void embwin_bind(EmbWindow* w, char* base) {
    size_t off[EW_N];
    w->bytes = embwin_layout(w->n_lm, w->n_sp, w->n_dm, w->n_skin, w->sk_held, off, &w->sk_bytes);
    w->sk_omega = reinterpret_cast<double*>(base + off[EW_SK_OMEGA]);
    w->lm_obs = reinterpret_cast<int*>(base + off[EW_LM_OBS]); w->sp_ij = reinterpret_cast<int*>(base + off[EW_SP_IJ]);
    w->sp_d0 = reinterpret_cast<float*>(base + off[EW_SP_D0]); w->dm_idx = reinterpret_cast<int*>(base + off[EW_DM_IDX]);
    w->dm_w = reinterpret_cast<float*>(base + off[EW_DM_W]); w->sk_obs = reinterpret_cast<int*>(base + off[EW_SK_OBS]);
    w->sk_node = reinterpret_cast<int*>(base + off[EW_SK_NODE]); w->lm_xyz = reinterpret_cast<float*>(base + off[EW_LM_XYZ]);
    w->lm_uv = reinterpret_cast<float*>(base + off[EW_LM_UV]); w->lm_kf = reinterpret_cast<int*>(base + off[EW_LM_KF]);
    w->sk_xyz = reinterpret_cast<float*>(base + off[EW_SK_XYZ]); w->sk_uv = reinterpret_cast<float*>(base + off[EW_SK_UV]);
    w->sk_kf = reinterpret_cast<int*>(base + off[EW_SK_KF]);
}

__global__ void k_ew_flag(int n_obs, const int* __restrict__ kf_pt, const uint8_t* __restrict__ is_node, int* flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_obs) flag[i] = is_node[kf_pt[i]] ? 1 : 0;
}
// cur[(k, p)] <- node-copy index (flag scanned: lm_of), as k_win_cur
__global__ void k_ew_cur(int n_obs, const int* __restrict__ obs_k, const int* __restrict__ kf_pt, const int* __restrict__ flag, const int* __restrict__ lm_of,
                         int n_points, int* cur) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_obs && flag[i]) atomicMax(&cur[(size_t)obs_k[i] * n_points + kf_pt[i]], lm_of[i]);
}
// a node copy that is not the one `cur` kept: its map point is listed twice in the keyframe.  tot[0..4) <- the four counts.
__global__ void k_ew_check(int n_obs, const int* __restrict__ obs_k, const int* __restrict__ kf_pt, const int* __restrict__ flag, const int* __restrict__ lm_of,
                           int n_points, const int* __restrict__ cur, int* tot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_obs && flag[i] && cur[(size_t)obs_k[i] * n_points + kf_pt[i]] != lm_of[i]) tot[4] = 1;
}
__global__ void k_ew_totals(int n_obs, const int* __restrict__ lm_of, const int* __restrict__ off_s, const int* __restrict__ off_d, const int* __restrict__ off_k, int* tot) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { tot[0] = lm_of[n_obs]; tot[1] = off_s[n_obs]; tot[2] = off_d[n_obs]; tot[3] = off_k[n_obs]; }
}

// lm_of / off_k at the keyframe boundaries: out[k] = node copies before keyframe k, out[n_kf + 1 + k] = skinned observations before it
__global__ void k_ew_kf_bounds(int n_kf, const int* __restrict__ kf_rowptr, const int* __restrict__ lm_of, const int* __restrict__ off_k, int* out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= n_kf) { out[k] = lm_of[kf_rowptr[k]]; out[n_kf + 1 + k] = off_k[kf_rowptr[k]]; }
}

// One thread per observation i = (keyframe k, map point p); W.lm_k / W.kf_pt are per OBSERVATION here, W.cur the node-copy table.
// EMIT = false: counts per observation; true: writes at the scanned offsets.  Emitting, sk_node / sk_omega hold the skinned observations
// of [i_lo, i_hi) only, from slot sk_lo on (a rank's keyframes; the whole window: 0, n_obs, 0); sk_obs is written for every one.
template <bool EMIT>
__global__ void k_ew_walk(WinDev W, int n_obs, const int* __restrict__ flag, const int* __restrict__ lm_of, int* cnt_s, int* cnt_d, int* cnt_k,
                          const int* __restrict__ off_s, const int* __restrict__ off_d, const int* __restrict__ off_k, int* lm_obs, int* sp_ij, float* sp_d0,
                          int* dm_idx, float* dm_w, int* sk_obs, int* sk_node, double* sk_omega, int i_lo, int i_hi, int sk_lo) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_obs) return;
    const int k = W.lm_k[i], p = W.kf_pt[i];
    const int* cur = W.cur + (size_t)k * W.n_points;
    const int lo = W.L.rowptr[p], hi = W.L.rowptr[p + 1];
    if (!flag[i]) {                                                  // a skinned observation: its walk accepts node copies
        if (EMIT && (i < i_lo || i >= i_hi)) {                       // (another rank's: its place in sk_obs, which the count pass decided)
            if (off_k[i + 1] != off_k[i]) sk_obs[off_k[i]] = i;
            return;
        }
        int n_reg = 0;
        double tot = 0.0;
        for (int e = lo; e < hi; ++e) {
            if (n_reg > 10 || W.L.status[e] == NRS_GRAPH_BAD) break;
            if (cur[W.L.col[e]] < 0) continue;
            tot += (double)W.L.w[e];                               // (walk order, from 0.0: the host's sum)
            ++n_reg;
        }
        if (!EMIT) { cnt_s[i] = 0; cnt_d[i] = 0; cnt_k[i] = n_reg > 0 ? 1 : 0; return; }
        if (n_reg == 0) return;                                      // (no node copy within reach: the observation constrains nothing)
        sk_obs[off_k[i]] = i;
        const size_t q = (size_t)(off_k[i] - sk_lo);
        int j = 0;
        for (int e = lo; e < hi && j < n_reg; ++e) {                 // the same walk again: its first n_reg accepted entries
            const int o = W.L.col[e];
            if (cur[o] < 0) continue;
            sk_node[11 * q + j] = cur[o];
            sk_omega[11 * q + j] = (double)W.L.w[e] / tot;
            ++j;
        }
        for (; j < 11; ++j) { sk_node[11 * q + j] = -1; sk_omega[11 * q + j] = 0.0; }
        return;
    }
    const int l = lm_of[i];
    int ns = 0, nd = 0, n_reg = 0;
    if (EMIT) lm_obs[l] = i;
    for (int e = lo; e < hi; ++e) {                                  // springs between node copies (OPT:1033-1074)
        if (n_reg > 10 || W.L.status[e] == NRS_GRAPH_BAD) break;
        const int o = W.L.col[e];
        if (cur[o] < 0) continue;
        ++n_reg;
        if (cur[o] < l && win_walk_reaches(W, k, o, p, false)) continue;        // inserted by o's walk already
        if (EMIT) { const size_t q = (size_t)(off_s[i] + ns); sp_ij[2 * q] = l; sp_ij[2 * q + 1] = cur[o]; sp_d0[q] = W.L.d0[e]; }
        ++ns;
    }
    if (k + 1 < W.n_kf) {                                            // dampers with the next keyframe (OPT:1076-1136)
        const int* nxt = W.cur + (size_t)(k + 1) * W.n_points;
        if (nxt[p] >= 0) {
            n_reg = 0;
            for (int e = lo; e < hi; ++e) {
                if (n_reg > 10 || W.L.status[e] == NRS_GRAPH_BAD) break;
                const int o = W.L.col[e];
                if (cur[o] < 0 || nxt[o] < 0) continue;
                ++n_reg;
                if (cur[o] < l && win_walk_reaches(W, k, o, p, true)) continue;
                if (EMIT) {
                    const size_t q = (size_t)(off_d[i] + nd);
                    dm_idx[4 * q] = l; dm_idx[4 * q + 1] = cur[o]; dm_idx[4 * q + 2] = nxt[p]; dm_idx[4 * q + 3] = nxt[o];
                    dm_w[q] = W.L.w[e];
                }
                ++nd;
            }
        }
    }
    if (!EMIT) { cnt_s[i] = ns; cnt_d[i] = nd; cnt_k[i] = 0; }
}

// per-observation data of the node copies (n_a, obs_a) and of the skinned observations (n_b, obs_b)
__global__ void k_ew_gather(int n_a, const int* __restrict__ obs_a, int n_b, const int* __restrict__ obs_b, const float* __restrict__ obs_xyz,
                            const float* __restrict__ obs_uv, const int* __restrict__ obs_k, float* a_xyz, float* a_uv, int* a_kf, float* b_xyz, float* b_uv, int* b_kf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_a) {
        const size_t o = (size_t)obs_a[i];
        for (int a = 0; a < 3; ++a) a_xyz[3 * (size_t)i + a] = obs_xyz[3 * o + a];
        for (int a = 0; a < 2; ++a) a_uv[2 * (size_t)i + a] = obs_uv[2 * o + a];
        a_kf[i] = obs_k[o];
    }
    if (i < n_b) {
        const size_t o = (size_t)obs_b[i];
        for (int a = 0; a < 3; ++a) b_xyz[3 * (size_t)i + a] = obs_xyz[3 * o + a];
        for (int a = 0; a < 2; ++a) b_uv[2 * (size_t)i + a] = obs_uv[2 * o + a];
        b_kf[i] = obs_k[o];
    }
}

// ---- the same walks, a WAVE per observation, over either list layout (WinLists::range: the caller's CSR, or the fixed-stride prefixes the
// resident graph leaves on the device -- nrs_dba_solve_window_rg_embedded).  A node copy's springs and dampers are win_walk itself on the
// node-copy table.  The walk of a skinned observation steps through its list 64 contiguous entries at a time with win_walk's ballots and
// its stop rule (the first BAD entry, or an entry that arrives with more than 10 accepted); it RAN OFF under the rule of
// nrs_engine_winedges.hpp.  The fp64 weight sum is the host's: carried wave-uniformly from 0.0, the accepted lanes' weights widened and
// added one by one in ascending lane order, chunk after chunk -- walk order, no tree.
// WRITE = false: returns the number of accepted node copies (<= 11), their weight sum in *tot.  WRITE = true: the same walk again, the
// accepted node copies and weight / *tot into row q of sk_node / sk_omega (an accepted entry's place is the number accepted before it).
template <bool WRITE>
__device__ inline int ew_skin_walk(const WinDev& W, int k, int p, int lane, double* tot, size_t q, int* sk_node, double* sk_omega, bool* ran_off) {
#pragma clang fp contract(off)
    const int* cur = W.cur + (size_t)k * W.n_points;
    int64_t lo; int n; bool cut;
    W.L.range(p, lo, n, cut);
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    int n_reg = 0;
    bool broke = false;
    double sum = 0.0;
    for (int ch = 0; ch < n && !broke; ch += 64) {
        const int a = ch + lane;
        const bool valid = a < n;
        const int64_t e = lo + a;
        const int o = valid ? W.L.col[e] : 0;
        const bool bad = valid && W.L.status[e] == NRS_GRAPH_BAD;
        const bool pres = valid && cur[o] >= 0;                      // a node copy of this keyframe
        const unsigned long long presm = __ballot(pres);
        const int before = n_reg + __popcll(presm & below);         // accepted when the loop comes to this entry
        const unsigned long long brkm = __ballot(valid && (bad || before > 10));
        const int fb = brkm ? __ffsll((long long)brkm) - 1 : 64;    // the loop breaks at this lane's entry
        const unsigned long long accm = fb < 64 ? presm & ((1ull << fb) - 1ull) : presm;
        const bool acc = pres && lane < fb;
        const float w = acc ? W.L.w[e] : 0.f;
        if (!WRITE) {
            for (unsigned long long m = accm; m; m &= m - 1ull) sum += (double)__shfl(w, __ffsll((long long)m) - 1);
        } else if (acc) {
            sk_node[11 * q + before] = cur[o];
            sk_omega[11 * q + before] = (double)w / *tot;
        }
        n_reg += __popcll(accm);
        broke = fb < 64;
    }
    if (!WRITE) *tot = sum;
    *ran_off = cut && !broke && n_reg <= 10;
    return n_reg;
}

// A wave per observation i; the arguments of k_ew_walk without the rank's slice.  EMIT = false: counts per observation, and in ran[0] the
// walks that ran off, in ran[1] the smallest map point one of them started from (the flag of k_win_edges<false>: integer atomics of the
// count pass only); of a skinned observation also the number of accepted node copies and their weight sum (sk_n / sk_tot: the last count
// round's stand).  true: writes at the scanned offsets; a skinned observation's one walk divides by the saved sum.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_ew_walk_wave(WinDev W, int n_obs, const int* __restrict__ flag, const int* __restrict__ lm_of, int* cnt_s, int* cnt_d, int* cnt_k,
                                                      const int* __restrict__ off_s, const int* __restrict__ off_d, const int* __restrict__ off_k, int* lm_obs, int* sp_ij,
                                                      float* sp_d0, int* dm_idx, float* dm_w, int* sk_obs, int* sk_node, double* sk_omega, int* ran, int* sk_n, double* sk_tot) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_obs) return;                                          // (wave-uniform)
    const int k = W.lm_k[i], p = W.kf_pt[i];
    bool off_end = false;
    int n_ran = 0;
    if (!flag[i]) {                                                  // a skinned observation
        if (!EMIT) {
            double tot = 0.0;
            const int n_acc = ew_skin_walk<false>(W, k, p, lane, &tot, 0, nullptr, nullptr, &off_end);
            if (lane == 0) {
                cnt_s[i] = 0; cnt_d[i] = 0; cnt_k[i] = n_acc > 0 ? 1 : 0;
                sk_n[i] = n_acc; sk_tot[i] = tot;
                if (off_end) { atomicAdd(&ran[0], 1); atomicMin(&ran[1], p); }
            }
            return;
        }
        const int n_acc = sk_n[i];
        if (n_acc == 0) return;                                      // (no node copy within reach: it constrains nothing)
        double tot = sk_tot[i];
        const size_t q = (size_t)off_k[i];
        if (lane == 0) sk_obs[q] = i;
        (void)ew_skin_walk<true>(W, k, p, lane, &tot, q, sk_node, sk_omega, &off_end);
        if (lane >= n_acc && lane < 11) { sk_node[11 * q + lane] = -1; sk_omega[11 * q + lane] = 0.0; }
        return;
    }
    const int l = lm_of[i];
    if (EMIT && lane == 0) lm_obs[l] = i;
    const int ns = win_walk<EMIT, false>(W, l, k, p, lane, EMIT ? off_s[i] : 0, sp_ij, sp_d0, dm_idx, dm_w, &off_end);
    n_ran += off_end;
    int nd = 0;
    if (k + 1 < W.n_kf && W.cur[(size_t)(k + 1) * W.n_points + p] >= 0) {
        nd = win_walk<EMIT, true>(W, l, k, p, lane, EMIT ? off_d[i] : 0, sp_ij, sp_d0, dm_idx, dm_w, &off_end);
        n_ran += off_end;
    }
    if (!EMIT && lane == 0) {
        cnt_s[i] = ns; cnt_d[i] = nd; cnt_k[i] = 0;
        if (n_ran) { atomicAdd(&ran[0], n_ran); atomicMin(&ran[1], p); }
    }
}

// ---- the construction in stages, shared by the CSR form (engine_build_embedded_window_device) and the resident-graph form
// (engine_build_embedded_window_device_rg); the two differ in where the lists come from and in the kernel of the count and emit passes.
struct EwBuild {                                                     // one build: its sizes and its scratch (pack_ws3, dp_embwin_plan)
    int n_kf, n_obs, n_points;
    size_t tmp_bytes;
    DpPlan<EL_COUNT> P;
    char* w3;
    int *d_pt, *d_k, *d_cur, *d_flag, *d_lm, *d_cs, *d_cd, *d_ck, *d_os, *d_od, *d_ok, *d_tot, *d_krp, *d_kfb;
    float *d_xyz, *d_uv;
    uint8_t* d_node;
    void* tmp;
};
// scratch, the uploads every form makes (the observations, their data, the node flags) and the cleared words
static int ew_begin(nrs_ctx* c, EwBuild& B, int n_kf, const int* kf_rowptr, const int* kf_pt, const int* obs_kf, const float* obs_xyz, const float* obs_uv, int n_points,
                    const uint8_t* is_node, size_t nnz, bool rg, bool own_only) {
    hipStream_t st = c->stream;
    const int n_obs = kf_rowptr[n_kf];
    B.n_kf = n_kf; B.n_obs = n_obs; B.n_points = n_points;
    B.tmp_bytes = win_scan_tmp_bytes(c, (size_t)std::max(n_obs, rg ? n_points : 0) + 1);
    B.P = dp_embwin_plan(DpEmbWinIn{(size_t)n_kf, (size_t)n_obs, (size_t)n_points, nnz, B.tmp_bytes, rg});
    NRS_TRY(c->ensure(c->pack_ws3, B.P.need));
    char* const w3 = B.w3 = c->pack_ws3.as<char>();
    const auto& P = B.P;
    B.d_pt = P.at<int>(w3, EL_pt); B.d_k = P.at<int>(w3, EL_k); B.d_cur = P.at<int>(w3, EL_cur); B.d_flag = P.at<int>(w3, EL_flag); B.d_lm = P.at<int>(w3, EL_lm);
    B.d_cs = P.at<int>(w3, EL_cs); B.d_cd = P.at<int>(w3, EL_cd); B.d_ck = P.at<int>(w3, EL_ck); B.d_os = P.at<int>(w3, EL_os); B.d_od = P.at<int>(w3, EL_od);
    B.d_ok = P.at<int>(w3, EL_ok); B.d_tot = P.at<int>(w3, EL_tot); B.d_krp = P.at<int>(w3, EL_krp); B.d_kfb = P.at<int>(w3, EL_kfb);
    B.d_xyz = P.at<float>(w3, EL_xyz); B.d_uv = P.at<float>(w3, EL_uv);
    B.d_node = P.at<uint8_t>(w3, EL_node);
    B.tmp = P.at<char>(w3, EL_tmp);
    NRS_HIP(c, hipMemcpyAsync(B.d_pt, kf_pt, sizeof(int) * (size_t)n_obs, hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(B.d_k, obs_kf, sizeof(int) * (size_t)n_obs, hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(B.d_node, is_node, (size_t)n_points, hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(B.d_xyz, obs_xyz, sizeof(float) * 3 * (size_t)n_obs, hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(B.d_uv, obs_uv, sizeof(float) * 2 * (size_t)n_obs, hipMemcpyHostToDevice, st));
    if (own_only) NRS_HIP(c, hipMemcpyAsync(B.d_krp, kf_rowptr, sizeof(int) * ((size_t)n_kf + 1), hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemsetAsync(B.d_cur, 0xFF, sizeof(int) * (size_t)n_kf * n_points, st));
    NRS_HIP(c, hipMemsetAsync(B.d_flag + n_obs, 0, sizeof(int), st));
    NRS_HIP(c, hipMemsetAsync(B.d_cs + n_obs, 0, sizeof(int), st));
    NRS_HIP(c, hipMemsetAsync(B.d_cd + n_obs, 0, sizeof(int), st));
    NRS_HIP(c, hipMemsetAsync(B.d_ck + n_obs, 0, sizeof(int), st));
    NRS_HIP(c, hipMemsetAsync(B.d_tot, 0, sizeof(int) * 8, st));
    return NRS_OK;
}
// node-copy numbering, the table and the duplicate-node check (its word: d_tot[4])
static int ew_number(nrs_ctx* c, const EwBuild& B) {
    hipStream_t st = c->stream;
    const dim3 g((unsigned)((B.n_obs + 255) / 256)), b(256);
    hipLaunchKernelGGL(k_ew_flag, g, b, 0, st, B.n_obs, B.d_pt, B.d_node, B.d_flag);
    size_t t2 = B.tmp_bytes;
    NRS_HIP(c, rocprim::exclusive_scan(B.tmp, t2, B.d_flag, B.d_lm, 0, (size_t)B.n_obs + 1, rocprim::plus<int>(), st));
    hipLaunchKernelGGL(k_ew_cur, g, b, 0, st, B.n_obs, B.d_k, B.d_pt, B.d_flag, B.d_lm, B.n_points, B.d_cur);
    hipLaunchKernelGGL(k_ew_check, g, b, 0, st, B.n_obs, B.d_k, B.d_pt, B.d_flag, B.d_lm, B.n_points, B.d_cur, B.d_tot);
    return NRS_OK;
}
// Behind the count pass: the scans and the totals, the rank's share (own_only), the emit pass (`emit(dv)`: the form's kernel, writing into
// the device blob dv is bound to), the gathers, one copy back into the pinned blob and out's pointers into it.
template <class Emit>
static int ew_finish(nrs_ctx* c, const EwBuild& B, const int* kf_rowptr, bool own_only, StageTimer& mark, Emit&& emit, EmbWindow* out, bool* duplicate) {
    hipStream_t st = c->stream;
    const int n_kf = B.n_kf, n_obs = B.n_obs;
    const dim3 b(256);
    size_t t2;
    t2 = B.tmp_bytes; NRS_HIP(c, rocprim::exclusive_scan(B.tmp, t2, B.d_cs, B.d_os, 0, (size_t)n_obs + 1, rocprim::plus<int>(), st));
    t2 = B.tmp_bytes; NRS_HIP(c, rocprim::exclusive_scan(B.tmp, t2, B.d_cd, B.d_od, 0, (size_t)n_obs + 1, rocprim::plus<int>(), st));
    t2 = B.tmp_bytes; NRS_HIP(c, rocprim::exclusive_scan(B.tmp, t2, B.d_ck, B.d_ok, 0, (size_t)n_obs + 1, rocprim::plus<int>(), st));
    hipLaunchKernelGGL(k_ew_totals, dim3(1), dim3(64), 0, st, n_obs, B.d_lm, B.d_os, B.d_od, B.d_ok, B.d_tot);
    if (own_only) hipLaunchKernelGGL(k_ew_kf_bounds, dim3((unsigned)((n_kf + 256) / 256)), b, 0, st, n_kf, B.d_krp, B.d_lm, B.d_ok, B.d_kfb);
    NRS_HIP(c, hipGetLastError());
    int tot[5] = {0, 0, 0, 0, 0};
    std::vector<int> kfb(own_only ? 2 * ((size_t)n_kf + 1) : 0);
    NRS_HIP(c, hipMemcpyAsync(tot, B.d_tot, sizeof(tot), hipMemcpyDeviceToHost, st));
    if (own_only) NRS_HIP(c, hipMemcpyAsync(kfb.data(), B.d_kfb, sizeof(int) * kfb.size(), hipMemcpyDeviceToHost, st));
    NRS_HIP(c, hipStreamSynchronize(st));
    mark("count + scans");
    if (tot[4]) { *duplicate = true; return NRS_OK; }
    out->n_obs = n_obs; out->n_lm = tot[0]; out->n_sp = tot[1]; out->n_dm = tot[2]; out->n_skin = tot[3];
    out->sk_base = 0; out->sk_held = tot[3]; out->k0 = 0; out->k1 = n_kf;
    if (own_only) {                                                  // this rank's keyframes and its slice of the skinned list
        std::vector<int> kf_nodes(n_kf);
        for (int k = 0; k < n_kf; ++k) kf_nodes[k] = kfb[k + 1] - kfb[k];
        embwin_own_range(n_kf, kf_nodes.data(), c->comm->world, c->comm->rank, &out->k0, &out->k1);
        out->sk_base = kfb[n_kf + 1 + out->k0]; out->sk_held = kfb[n_kf + 1 + out->k1] - out->sk_base;
        if (out->k0 < 0 || out->k1 > n_kf || out->k0 >= out->k1 || out->sk_base < 0 || out->sk_held < 0 || out->sk_base + out->sk_held > tot[3])
            return c->fail(NRS_ERR_STATE, "embedded lists: keyframe range [%d, %d) / slice [%d, +%d) of %d", out->k0, out->k1, out->sk_base, out->sk_held, tot[3]);
    }
    // ---- emit pass and gathers into one blob, one copy back
    size_t off[EW_N];
    const size_t bytes = embwin_layout(tot[0], tot[1], tot[2], tot[3], out->sk_held, off);
    NRS_TRY(c->ensure(c->pack_ws4, bytes + 4096));
    if (bytes > c->embwin_pin.cap) {
        const size_t want = bytes + bytes / 4;
        hipError_t he = c->ensure_pinned(c->embwin_pin, want, hipHostMallocDefault);
        if (he != hipSuccess) return c->fail(NRS_ERR_ALLOC, "hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(he));
    }
    EmbWindow dv = *out;
    embwin_bind(&dv, c->pack_ws4.as<char>());
    emit(dv);
    const int n_g = std::max(dv.n_lm, dv.sk_held);                   // (the gather of the skinned observations: the slice of sk_obs)
    if (n_g > 0)
        hipLaunchKernelGGL(k_ew_gather, dim3((unsigned)((n_g + 255) / 256)), b, 0, st, dv.n_lm, dv.lm_obs, dv.sk_held, dv.sk_obs + dv.sk_base, B.d_xyz, B.d_uv, B.d_k,
                           dv.lm_xyz, dv.lm_uv, dv.lm_kf, dv.sk_xyz, dv.sk_uv, dv.sk_kf);
    NRS_HIP(c, hipGetLastError());
    mark("emit + gathers");
    NRS_HIP(c, hipMemcpyAsync(c->embwin_pin.p, c->pack_ws4.as<char>(), bytes, hipMemcpyDeviceToHost, st));
    NRS_HIP(c, hipStreamSynchronize(st));
    mark("copy back");
    embwin_bind(out, c->embwin_pin.as<char>());
    out->on_device = 1;
    return NRS_OK;
}

// Builds the lists of an embedded window on the device and copies them to the context's pinned staging (out's pointers: valid until
// the next call).  The arguments are validated by the caller (indices in range, nnz > 0; own_only: a communicator of at most n_kf ranks).
int engine_build_embedded_window_device(nrs_ctx* c, int n_kf, const int* kf_rowptr, const int* kf_pt, const int* obs_kf, const float* obs_xyz, const float* obs_uv,
                                        int n_points, const uint8_t* is_node, const int* nbr_rowptr, const int* nbr_col, const float* nbr_w, const float* nbr_d0,
                                        const int* nbr_status, bool own_only, EmbWindow* out, bool* duplicate) {
    *duplicate = false;
    const int n_obs = kf_rowptr[n_kf], nnz = nbr_rowptr[n_points];
    hipStream_t st = c->stream;
    NRS_HIP(c, hipSetDevice(c->device));
    StageTimer mark{c, "embedded lists", true, 18, false};
    EwBuild B;
    NRS_TRY(ew_begin(c, B, n_kf, kf_rowptr, kf_pt, obs_kf, obs_xyz, obs_uv, n_points, is_node, (size_t)nnz, false, own_only));
    int *d_nrp = B.P.at<int>(B.w3, EL_nrp), *d_col = B.P.at<int>(B.w3, EL_col), *d_st = B.P.at<int>(B.w3, EL_st);
    float *d_w = B.P.at<float>(B.w3, EL_w), *d_d0 = B.P.at<float>(B.w3, EL_d0);
    NRS_HIP(c, hipMemcpyAsync(d_nrp, nbr_rowptr, sizeof(int) * ((size_t)n_points + 1), hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(d_col, nbr_col, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(d_st, nbr_status, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(d_w, nbr_w, sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice, st));
    NRS_HIP(c, hipMemcpyAsync(d_d0, nbr_d0, sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice, st));
    mark("uploads");
    NRS_TRY(ew_number(c, B));
    // ---- count pass (a thread per observation), then the shared stages with k_ew_walk's emit pass
    const dim3 g((unsigned)((n_obs + 255) / 256)), b(256);
    WinDev wd{n_kf, n_points, nullptr, B.d_pt, B.d_k, WinLists{d_nrp, nullptr, nullptr, 0, d_col, d_st, d_w, d_d0}, B.d_cur};
    hipLaunchKernelGGL((k_ew_walk<false>), g, b, 0, st, wd, n_obs, B.d_flag, B.d_lm, B.d_cs, B.d_cd, B.d_ck, (const int*)nullptr, (const int*)nullptr, (const int*)nullptr,
                       (int*)nullptr, (int*)nullptr, (float*)nullptr, (int*)nullptr, (float*)nullptr, (int*)nullptr, (int*)nullptr, (double*)nullptr, 0, n_obs, 0);
    return ew_finish(c, B, kf_rowptr, own_only, mark, [&](const EmbWindow& dv) {
        hipLaunchKernelGGL((k_ew_walk<true>), g, b, 0, st, wd, n_obs, B.d_flag, B.d_lm, (int*)nullptr, (int*)nullptr, (int*)nullptr, B.d_os, B.d_od, B.d_ok, dv.lm_obs, dv.sp_ij,
                           dv.sp_d0, dv.dm_idx, dv.dm_w, dv.sk_obs, dv.sk_node, dv.sk_omega, kf_rowptr[dv.k0], kf_rowptr[dv.k1], dv.sk_base);
    }, out, duplicate);
}

// The same lists served by the device-resident all-pairs graph (include/nrs.h nrs_dba_solve_window_rg_embedded): no neighbour array is
// uploaded.  The window's distinct map points -- over ALL observations, node or not: every walk starts from an observed point and follows
// only points its keyframe observes -- are listed as for the plain window (k_win_mark, the scan, k_win_rows); GetEdges and the count pass
// (k_ew_walk_wave<false>) run in win_count_rounds' doubling rounds; then the shared stages.  stats: as engine_build_edges_device_rg.
int engine_build_embedded_window_device_rg(nrs_ctx* c, int n_kf, const int* kf_rowptr, const int* kf_pt, const int* obs_kf, const float* obs_xyz, const float* obs_uv,
                                           nrs_rgraph* g, const uint8_t* is_node, int cap_per_point, EmbWindow* out, bool* duplicate, int64_t stats[4]) {
    *duplicate = false;
    const int n_obs = kf_rowptr[n_kf], n_points = rg_capacity(g);
    hipStream_t st = c->stream;
    NRS_HIP(c, hipSetDevice(c->device));
    StageTimer mark{c, "embedded lists (rg)", true, 18, false};
    EwBuild B;
    NRS_TRY(ew_begin(c, B, n_kf, kf_rowptr, kf_pt, obs_kf, obs_xyz, obs_uv, n_points, is_node, 0, true, false));
    int *d_mark = B.P.at<int>(B.w3, EL_mark), *d_pos = B.P.at<int>(B.w3, EL_pos), *d_ids = B.P.at<int>(B.w3, EL_ids), *d_row = B.P.at<int>(B.w3, EL_row),
        *d_ran = B.P.at<int>(B.w3, EL_ran), *d_skn = B.P.at<int>(B.w3, EL_skn);
    double* d_sktot = B.P.at<double>(B.w3, EL_sktot);
    mark("uploads");
    NRS_TRY(ew_number(c, B));
    // ---- the distinct map points, ascending, and the point -> list-row table
    const dim3 g1((unsigned)((n_obs + 255) / 256)), gw((unsigned)((n_obs + 3) / 4)), b(256);       // a thread / a wave per observation
    NRS_HIP(c, hipMemsetAsync(d_mark, 0, sizeof(int) * ((size_t)n_points + 1), st));
    hipLaunchKernelGGL(k_win_mark, g1, b, 0, st, n_obs, B.d_pt, d_mark);
    size_t t1 = B.tmp_bytes;
    NRS_HIP(c, rocprim::exclusive_scan(B.tmp, t1, d_mark, d_pos, 0, (size_t)n_points + 1, rocprim::plus<int>(), st));
    hipLaunchKernelGGL(k_win_rows, dim3((unsigned)((n_points + 255) / 256)), b, 0, st, n_points, d_mark, d_pos, d_ids, d_row);
    NRS_HIP(c, hipGetLastError());
    int n_ids = 0, dup = 0;
    NRS_HIP(c, hipMemcpyAsync(&n_ids, d_pos + n_points, sizeof(int), hipMemcpyDeviceToHost, st));
    NRS_HIP(c, hipMemcpyAsync(&dup, B.d_tot + 4, sizeof(int), hipMemcpyDeviceToHost, st));       // (ew_number's duplicate-node word: refused before any round)
    NRS_HIP(c, hipStreamSynchronize(st));
    if (dup) { *duplicate = true; return NRS_OK; }
    if (n_ids <= 0 || n_ids > n_points) return c->fail(NRS_ERR_STATE, "nrs_dba_solve_window_rg_embedded: %d distinct map points", n_ids);
    // ---- GetEdges and the count pass, in rounds
    const int cap_max = rg_max_cap_per_point(g);
    WinDev wd{n_kf, n_points, nullptr, B.d_pt, B.d_k, WinLists{nullptr, d_row, nullptr, 0, nullptr, nullptr, nullptr, nullptr}, B.d_cur};
    WinRounds wr;
    NRS_TRY(win_count_rounds(c, g, wd, n_ids, d_ids, d_row, d_ran, std::min(cap_per_point, cap_max), cap_max, "nrs_dba_solve_window_rg_embedded", [&] {
        hipLaunchKernelGGL((k_ew_walk_wave<false>), gw, b, 0, st, wd, n_obs, B.d_flag, B.d_lm, B.d_cs, B.d_cd, B.d_ck, (const int*)nullptr, (const int*)nullptr,
                           (const int*)nullptr, (int*)nullptr, (int*)nullptr, (float*)nullptr, (int*)nullptr, (float*)nullptr, (int*)nullptr, (int*)nullptr, (double*)nullptr, d_ran, d_skn, d_sktot);
    }, &wr));
    if (stats) { stats[0] = n_ids; stats[1] = wr.cap; stats[2] = wr.rounds; stats[3] = wr.ran_first; }
    return ew_finish(c, B, kf_rowptr, false, mark, [&](const EmbWindow& dv) {
        hipLaunchKernelGGL((k_ew_walk_wave<true>), gw, b, 0, st, wd, n_obs, B.d_flag, B.d_lm, (int*)nullptr, (int*)nullptr, (int*)nullptr, B.d_os, B.d_od, B.d_ok, dv.lm_obs,
                           dv.sp_ij, dv.sp_d0, dv.dm_idx, dv.dm_w, dv.sk_obs, dv.sk_node, dv.sk_omega, (int*)nullptr, d_skn, d_sktot);
    }, out, duplicate);
}

}  // namespace nrs
