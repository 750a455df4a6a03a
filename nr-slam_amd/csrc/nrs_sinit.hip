// f8: stereo map initialisation (include/nrs.h "f8"; DESIGN.md 4 "Stereo map initialisation").
//   nrs_dbscan3d      Dbscan3D (modules/utilities/dbscan.cc:61-104): this project's definition of the clustering, the reference's ranking
//   nrs_init_stereo   Tracking::StereoMapInitialization (modules/tracking/tracking.cc:216-289) up to the selected landmarks
//
// The clustering runs on m points whose count is a word on the device (nrs_init_stereo's gate leaves it there), in rows of W = ceil(cap / 64)
// 64-bit words where cap is the host's bound on m.  Launches:
//   k_db_neigh     a wave per point over all m: d2 in fp64 in the stated order, one ballot per 64 points = one word of the point's adjacency
//                  row; the neighbour count, the core flag and the starting label (its own index for a core point)
//   k_db_comp      ONE workgroup: the core bit mask, then minimum-label propagation over the core points with pointer jumping until a
//                  whole sweep changes nothing.  Labels only ever decrease and are always the index of a core point of the same component,
//                  so the fixed point -- every core point holds its component's lowest core index -- is unique and the result does not
//                  depend on the order in which the waves run.  Then the roots (label == index) in ascending order get the raw labels:
//                  a stable compaction in chunks of 1024 with a carried count (the form of nrs_point_reuse)
//   k_db_border    a wave per point: a core point takes its root's raw label, a non-core point the lowest raw label among its core
//                  neighbours, else -1; class sizes by integer atomics
//   k_db_rank      a thread per class: rank = classes that are larger, or as large with a lower key (noise: key -1, class 0 here)
//   k_db_label     label = rank of the raw label's class
// nrs_init_stereo puts k_si_gate (status / depth gate, stable compaction in keypoint order) between the matcher's launches
// (stereo_match_enqueue, nrs_eval.hip) and these, and k_si_select (codes, labels by keypoint, the rank-0 points in keypoint order) behind.
// One workgroup never waits for another; the only persistent loop is inside k_db_comp's single workgroup.
//
// f6: flow-track clustering (include/nrs.h "f6"; DESIGN.md 4 "Flow-track clustering"), on the same rows.
//   nrs_dbscan_nd             DbscanND (modules/utilities/dbscan.cc:106-131): the same rule over dim <= 64 coordinates, no ranking
//   nrs_flow_tracks_cluster   MonocularMapInitializer::FeatureTracksClustering (modules/tracking/monocular_map_initializer.cc:185-219)
// Launches: k_flow_build (tracks only), k_db_neigh_nd (LDS tiles of 64 candidates shared by a workgroup's queries; NRS_DBND_NO_TILE:
// k_db_neigh_nd_plain, a wave per point), then k_db_comp and k_db_border as above and k_dbnd_counts; the raw label is the label.
#include <climits>
#include "nrs_ctx.hpp"
#include "nrs_device.hpp"
#include "nrs_sinit_host.hpp"
#include "nrs_flowc_host.hpp"

namespace nrs {
namespace {

typedef unsigned long long u64;
constexpr int DB_BLOCK = 1024;                            // the single-workgroup kernels: a compaction chunk
constexpr int DB_WORDS = SINIT_MAX / 64;                  // words of the longest adjacency row (256)

inline size_t padded(size_t bytes) { return (bytes + 255) / 256 * 256; }
struct Carver {                                            // 256-byte aligned pieces of one allocation
    char* p;
    size_t used = 0;
    explicit Carver(char* base) : p(base) {}
    template <class T> T* take(size_t count) {
        T* r = reinterpret_cast<T*>(p + used);
        used += padded(count * sizeof(T));
        return r;
    }
};

// the clustering's device arrays for up to cap points
struct DbWs {
    int cap, W;
    u64* adj;            // cap x W
    u64* coremask;       // DB_WORDS
    int* core;           // cap
    int* lab;            // cap: lowest core index of the component so far (INT_MAX: not a core point)
    int* rawid;          // cap: raw label of a root
    int* size;           // cap + 1: class sizes, noise first
    int* rank;           // cap + 1
};
size_t db_ws_bytes(int cap) { return DbRowsLayout((size_t)cap).bytes; }     // (nrs_flowc_host.hpp: the piece's layout, checked on the host)
DbWs db_carve(char* base, int cap) {
    const DbRowsLayout L((size_t)cap);
    DbWs w;
    w.cap = cap; w.W = (int)L.W;
    w.adj = reinterpret_cast<u64*>(base + L.adj);
    w.coremask = reinterpret_cast<u64*>(base + L.coremask);
    w.core = reinterpret_cast<int*>(base + L.core);
    w.lab = reinterpret_cast<int*>(base + L.lab);
    w.rawid = reinterpret_cast<int*>(base + L.rawid);
    w.size = reinterpret_cast<int*>(base + L.size);
    w.rank = reinterpret_cast<int*>(base + L.rank);
    return w;
}

__device__ inline int ld_relaxed(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline int wave_min(int v) {
    for (int m = 1; m < 64; m <<= 1) v = min(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ inline int lowest_bit(u64 b) { return __ffsll((long long)b) - 1; }

// rank of this thread's flag among the workgroup's set flags (thread order) and their total: wave ballots + one LDS row of wave counts
__device__ inline int db_block_rank(bool flag, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const u64 m = __ballot(flag);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                                               // (the row's previous use is over)
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int off = 0;
    total = 0;
    for (int k = 0; k < DB_BLOCK / 64; ++k) { const int cnt = s_wave[k]; if (k < wv) off += cnt; total += cnt; }
    return off + before;
}

__global__ __launch_bounds__(256) void k_db_neigh(const int* __restrict__ d_m, int cap, int W, const float* __restrict__ xyz, double eps2,
                                                  int min_points, u64* __restrict__ adj, int* __restrict__ core, int* __restrict__ lab) {
#pragma clang fp contract(off)
    const int m = min(*d_m, cap);
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m) return;                                            // (uniform over the wave)
    const double xi = (double)xyz[3 * i], yi = (double)xyz[3 * i + 1], zi = (double)xyz[3 * i + 2];
    const int Wm = (m + 63) / 64;
    int cnt = 0;
    for (int wd = 0; wd < Wm; ++wd) {
        const int j = wd * 64 + lane;
        bool nb = false;
        if (j < m && j != i) {
            const double dx = (double)xyz[3 * j] - xi, dy = (double)xyz[3 * j + 1] - yi, dz = (double)xyz[3 * j + 2] - zi;
            const double xx = dx * dx;
            const double yy = dy * dy;
            const double zz = dz * dz;
            const double s = xx + yy;
            const double d2 = s + zz;
            nb = d2 <= eps2;                                       // inclusive; NaN and +inf compare false
        }
        const u64 word = __ballot(nb);
        if (lane == 0) adj[(size_t)i * W + wd] = word;
        cnt += __popcll(word);
    }
    if (lane == 0) {
        const bool c = cnt >= min_points;
        core[i] = c ? 1 : 0;
        lab[i] = c ? i : INT_MAX;
    }
}

__global__ __launch_bounds__(DB_BLOCK) void k_db_comp(const int* __restrict__ d_m, int cap, int W, const u64* __restrict__ adj,
                                                      const int* __restrict__ core, int* lab, u64* __restrict__ coremask,
                                                      int* __restrict__ rawid, int* __restrict__ size, int* __restrict__ counts) {
    __shared__ u64 s_core[DB_WORDS];
    __shared__ int s_wave[DB_BLOCK / 64];
    __shared__ int s_changed;
    const int m = min(*d_m, cap);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int Wm = (m + 63) / 64;
    for (int k = tid; k < DB_WORDS; k += DB_BLOCK) s_core[k] = 0ull;
    __syncthreads();
    for (int c0 = 0; c0 < m; c0 += DB_BLOCK) {
        const int i = c0 + tid;
        const u64 mask = __ballot(i < m && core[i] != 0);
        if (lane == 0) s_core[(c0 >> 6) + wv] = mask;              // (c0 <= 15360: word (c0 >> 6) + wv <= 255)
    }
    __syncthreads();
    for (int k = tid; k < DB_WORDS; k += DB_BLOCK) coremask[k] = s_core[k];
    // minimum-label propagation, a wave per core point and sweep; every value read is a label some wave wrote or the starting one
    for (;;) {
        __syncthreads();
        if (tid == 0) s_changed = 0;
        __syncthreads();
        for (int i = wv; i < m; i += DB_BLOCK / 64) {
            if (!((s_core[i >> 6] >> (i & 63)) & 1ull)) continue;  // (uniform over the wave)
            const int cur = ld_relaxed(lab + i);
            int mn = cur;
            for (int wd = lane; wd < Wm; wd += 64) {
                u64 bits = adj[(size_t)i * W + wd] & s_core[wd];
                while (bits) {
                    const int j = wd * 64 + lowest_bit(bits);
                    bits &= bits - 1ull;
                    mn = min(mn, ld_relaxed(lab + j));
                }
            }
            mn = wave_min(mn);
            for (int r = ld_relaxed(lab + mn); r < mn; r = ld_relaxed(lab + mn)) mn = r;      // pointer jumping: strictly decreasing
            if (mn < cur && lane == 0) { atomicMin(lab + i, mn); s_changed = 1; }
        }
        __syncthreads();
        if (!s_changed) break;
    }
    // raw labels of the roots in ascending index; the class sizes start at 0
    for (int k = tid; k <= m; k += DB_BLOCK) size[k] = 0;
    int base = 0;
    for (int c0 = 0; c0 < m; c0 += DB_BLOCK) {
        const int i = c0 + tid;
        const bool root = i < m && core[i] != 0 && ld_relaxed(lab + i) == i;
        int total;
        const int r = db_block_rank(root, s_wave, total);
        if (root) rawid[i] = base + r;
        base += total;
    }
    if (tid == 0) { counts[0] = base; counts[1] = 0; counts[2] = 0; }
}

__global__ __launch_bounds__(256) void k_db_border(const int* __restrict__ d_m, int cap, int W, const u64* __restrict__ adj,
                                                   const u64* __restrict__ coremask, const int* __restrict__ core, const int* __restrict__ lab,
                                                   const int* __restrict__ rawid, int* __restrict__ raw, int* size) {
    const int m = min(*d_m, cap);
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m) return;
    int r;
    if (core[i]) r = rawid[lab[i]];
    else {
        const int Wm = (m + 63) / 64;
        int mn = INT_MAX;
        for (int wd = lane; wd < Wm; wd += 64) {
            u64 bits = adj[(size_t)i * W + wd] & coremask[wd];
            while (bits) {
                const int j = wd * 64 + lowest_bit(bits);
                bits &= bits - 1ull;
                mn = min(mn, rawid[lab[j]]);
            }
        }
        mn = wave_min(mn);
        r = mn == INT_MAX ? -1 : mn;
    }
    if (lane == 0) { raw[i] = r; atomicAdd(size + (r + 1), 1); }
}

__global__ void k_db_rank(int cap, int noise_competes, const int* __restrict__ size, int* __restrict__ rank, int* counts) {
    const int ncl = min(counts[0], cap);
    const int k = blockIdx.x * blockDim.x + threadIdx.x;           // class k has the key k - 1
    if (k > ncl) return;
    const int sz = size[k];
    if (k == 0) {
        counts[1] = sz;
        if (!noise_competes) { rank[0] = -1; return; }
    }
    int r = 0;
    for (int k2 = noise_competes ? 0 : 1; k2 <= ncl; ++k2) {
        const int s2 = size[k2];
        if (s2 > sz || (s2 == sz && k2 < k)) ++r;
    }
    rank[k] = r;
    if (r == 0) counts[2] = sz;
}

__global__ void k_db_label(const int* __restrict__ d_m, int cap, const int* __restrict__ raw, const int* __restrict__ rank, int* __restrict__ label) {
    const int m = min(*d_m, cap);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) label[i] = rank[raw[i] + 1];
}

// the five launches on cap >= 1; d_m, xyz, raw, label and counts are device pointers (raw / label: cap entries, counts: 3)
void dbscan_enqueue(nrs_ctx* c, const DbWs& w, const int* d_m, const float* d_xyz, double eps, int min_points, int noise_competes, int* d_raw,
                    int* d_label, int* d_counts) {
    const double eps2 = eps * eps;
    const int cap = w.cap;
    hipLaunchKernelGGL(k_db_neigh, dim3((cap + 3) / 4), dim3(256), 0, c->stream, d_m, cap, w.W, d_xyz, eps2, min_points, w.adj, w.core, w.lab);
    hipLaunchKernelGGL(k_db_comp, dim3(1), dim3(DB_BLOCK), 0, c->stream, d_m, cap, w.W, w.adj, w.core, w.lab, w.coremask, w.rawid, w.size, d_counts);
    hipLaunchKernelGGL(k_db_border, dim3((cap + 3) / 4), dim3(256), 0, c->stream, d_m, cap, w.W, w.adj, w.coremask, w.core, w.lab, w.rawid, d_raw, w.size);
    hipLaunchKernelGGL(k_db_rank, dim3((cap + 1 + 255) / 256), dim3(256), 0, c->stream, cap, noise_competes ? 1 : 0, w.size, w.rank, d_counts);
    hipLaunchKernelGGL(k_db_label, dim3((cap + 255) / 256), dim3(256), 0, c->stream, d_m, cap, d_raw, w.rank, d_label);
}

// ---- flow-track clustering (include/nrs.h "f6"; DESIGN.md 4 "Flow-track clustering"): the neighbour stage over dim coordinates, the one
// stage that knows the dimension.  k_db_comp and k_db_border follow unchanged; no ranking, the raw label is the label.

// monocular_map_initializer.cc:191-211: a thread per (track, step), two fp32 subtractions
__global__ __launch_bounds__(256) void k_flow_build(int n, int length, const float* __restrict__ xy, float* __restrict__ flow) {
#pragma clang fp contract(off)
    const int steps = length - 1;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * steps) return;
    const size_t trk = e / steps, t = e - trk * steps + 1;
    const float* p = xy + (trk * length + t) * 2;
    flow[trk * 2 * steps + 2 * (t - 1)] = p[0] - p[-2];
    flow[trk * 2 * steps + 2 * (t - 1) + 1] = p[1] - p[-1];
}

// The tiled form.  A workgroup of four waves owns 4 R consecutive query points (a wave R of them) and streams ALL m candidates through LDS in
// tiles of 64 points: the tile is a contiguous span of the point-major array, read once per workgroup with consecutive threads on
// consecutive floats, and held dimension-major with an odd stride (65 floats), so that the transposing writes of consecutive threads (same
// point, next coordinate) fall on consecutive banks and a lane's walk over k reads lane-consecutive words.  The query coordinates lie in LDS
// as doubles, [k][query]: every lane of a wave reads the same address (a broadcast).  A lane owns candidate 64 wd + lane and accumulates d2
// for its wave's R queries in fp64, ascending k, the first product starting the sum; one ballot per tile and query is one adjacency word.
// Lanes past the tail tile's points and the candidate i itself give zero bits.
template <int R>
__global__ __launch_bounds__(256) void k_db_neigh_nd(const int* __restrict__ d_m, int cap, int W, int dim, const float* __restrict__ data,
                                                     double eps2, int min_points, u64* __restrict__ adj, int* __restrict__ core,
                                                     int* __restrict__ lab) {
#pragma clang fp contract(off)
    constexpr int Q = 4 * R;
    __shared__ float s_tile[FLOWC_MAX_DIM * FLOWC_TILE_STRIDE];
    __shared__ double s_q[FLOWC_MAX_DIM * Q];
    const int m = min(*d_m, cap);
    const int q0 = blockIdx.x * Q;
    if (q0 >= m) return;                                           // (uniform over the workgroup: before any barrier)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int step_p = 256 / dim, step_k = 256 % dim;              // what 256 floats further is in (point, coordinate)
    for (int e = tid; e < Q * dim; e += 256) {
        const int q = e / dim, k = e - q * dim, i = q0 + q;
        s_q[k * Q + q] = i < m ? (double)data[(size_t)i * dim + k] : 0.0;
    }
    int cnt[R];
#pragma unroll
    for (int r = 0; r < R; ++r) cnt[r] = 0;
    const int Wm = (m + 63) / 64;
    for (int wd = 0; wd < Wm; ++wd) {
        const int j0 = wd * FLOWC_TILE, np = min(FLOWC_TILE, m - j0);
        __syncthreads();                                           // the previous tile is read (first trip: the queries are written)
        const float* src = data + (size_t)j0 * dim;
        int p = tid / dim, k = tid - p * dim;
        for (int e = tid; e < np * dim; e += 256) {
            s_tile[k * FLOWC_TILE_STRIDE + p] = src[e];
            p += step_p; k += step_k;
            if (k >= dim) { k -= dim; ++p; }
        }
        __syncthreads();
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0;
        if (lane < np) {
            const double c0 = (double)s_tile[lane];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double d = c0 - s_q[wv * R + r];
                acc[r] = d * d;
            }
            for (int kk = 1; kk < dim; ++kk) {
                const double cj = (double)s_tile[kk * FLOWC_TILE_STRIDE + lane];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const double d = cj - s_q[kk * Q + wv * R + r];
                    const double pr = d * d;
                    acc[r] = acc[r] + pr;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = q0 + wv * R + r;
            const bool nb = lane < np && j0 + lane != i && acc[r] <= eps2;       // inclusive; NaN and +inf compare false
            const u64 word = __ballot(nb);
            if (i < m) {
                if (lane == 0) adj[(size_t)i * W + wd] = word;
                cnt[r] += __popcll(word);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = q0 + wv * R + r;
        if (i < m && lane == 0) {
            const bool c = cnt[r] >= min_points;
            core[i] = c ? 1 : 0;
            lab[i] = c ? i : INT_MAX;
        }
    }
}

// NRS_DBND_NO_TILE: k_db_neigh with a loop over the coordinates -- a wave per point, every lane fetches its candidate from global memory;
// the same sum in the same order, the same bits
__global__ __launch_bounds__(256) void k_db_neigh_nd_plain(const int* __restrict__ d_m, int cap, int W, int dim, const float* __restrict__ data,
                                                           double eps2, int min_points, u64* __restrict__ adj, int* __restrict__ core,
                                                           int* __restrict__ lab) {
#pragma clang fp contract(off)
    const int m = min(*d_m, cap);
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m) return;                                            // (uniform over the wave)
    const float* pi = data + (size_t)i * dim;
    const int Wm = (m + 63) / 64;
    int cnt = 0;
    for (int wd = 0; wd < Wm; ++wd) {
        const int j = wd * 64 + lane;
        bool nb = false;
        if (j < m && j != i) {
            const float* pj = data + (size_t)j * dim;
            const double d0 = (double)pj[0] - (double)pi[0];
            double d2 = d0 * d0;
            for (int k = 1; k < dim; ++k) {
                const double d = (double)pj[k] - (double)pi[k];
                const double pr = d * d;
                d2 = d2 + pr;
            }
            nb = d2 <= eps2;
        }
        const u64 word = __ballot(nb);
        if (lane == 0) adj[(size_t)i * W + wd] = word;
        cnt += __popcll(word);
    }
    if (lane == 0) {
        const bool c = cnt >= min_points;
        core[i] = c ? 1 : 0;
        lab[i] = c ? i : INT_MAX;
    }
}

// counts[1] = the noise class's size (what k_db_rank does on its way; no ranking here)
__global__ void k_dbnd_counts(const int* __restrict__ size, int* counts) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[1] = size[0];
}

// the four launches on cap >= 1 points of dim coordinates; d_m, data, label and counts are device pointers (label: cap entries, counts: 3)
void dbscan_nd_enqueue(nrs_ctx* c, const DbWs& w, const int* d_m, int dim, const float* d_data, double eps, int min_points, int* d_label,
                       int* d_counts) {
    const double eps2 = eps * eps;
    const int cap = w.cap;
    if (c->dbg.is_set(SW_DBND_NO_TILE)) {
        hipLaunchKernelGGL(k_db_neigh_nd_plain, dim3((cap + 3) / 4), dim3(256), 0, c->stream, d_m, cap, w.W, dim, d_data, eps2, min_points, w.adj,
                           w.core, w.lab);
    } else {
        const int R = flowc_queries_per_wave(cap), Q = 4 * R;
        const dim3 grid((cap + Q - 1) / Q);
        if (R == 1) hipLaunchKernelGGL(k_db_neigh_nd<1>, grid, dim3(256), 0, c->stream, d_m, cap, w.W, dim, d_data, eps2, min_points, w.adj, w.core, w.lab);
        else if (R == 2) hipLaunchKernelGGL(k_db_neigh_nd<2>, grid, dim3(256), 0, c->stream, d_m, cap, w.W, dim, d_data, eps2, min_points, w.adj, w.core, w.lab);
        else hipLaunchKernelGGL(k_db_neigh_nd<4>, grid, dim3(256), 0, c->stream, d_m, cap, w.W, dim, d_data, eps2, min_points, w.adj, w.core, w.lab);
    }
    hipLaunchKernelGGL(k_db_comp, dim3(1), dim3(DB_BLOCK), 0, c->stream, d_m, cap, w.W, w.adj, w.core, w.lab, w.coremask, w.rawid, w.size, d_counts);
    hipLaunchKernelGGL(k_db_border, dim3((cap + 3) / 4), dim3(256), 0, c->stream, d_m, cap, w.W, w.adj, w.coremask, w.core, w.lab, w.rawid, d_label, w.size);
    hipLaunchKernelGGL(k_dbnd_counts, dim3(1), dim3(64), 0, c->stream, w.size, d_counts);
}

struct SiPacked { unsigned xyz, status, code, raw, label, selected, sel_xyz; };          // word offsets of SinitLayout

// tracking.cc:229-233: status OK and z_min < z < z_max (a NaN fails), survivors in keypoint order.  hdr[0] n_matched, hdr[1] n_gated
// (the clustering's point count); codes 1 / 2 are final, a survivor's code is written by k_si_select
__global__ __launch_bounds__(DB_BLOCK) void k_si_gate(int n, float z_min, float z_max, int* out, SiPacked P, int* __restrict__ gidx,
                                                      float* __restrict__ gxyz) {
    __shared__ int s_wave[DB_BLOCK / 64];
    const float* of = reinterpret_cast<const float*>(out);
    int n_ok = 0, n_gate = 0;
    for (int c0 = 0; c0 < n; c0 += DB_BLOCK) {
        const int i = c0 + (int)threadIdx.x;
        bool ok = false, pass = false;
        float x = 0.f, y = 0.f, z = 0.f;
        if (i < n) {
            ok = out[P.status + i] == NRS_EVAL_OK;
            x = of[P.xyz + 3 * i]; y = of[P.xyz + 3 * i + 1]; z = of[P.xyz + 3 * i + 2];
            pass = ok && z > z_min && z < z_max;
            out[P.code + i] = !ok ? 1 : (pass ? 0 : 2);
            out[P.raw + i] = -2;
            out[P.label + i] = -2;
        }
        int tot_ok, tot;
        db_block_rank(ok, s_wave, tot_ok);
        const int r = db_block_rank(pass, s_wave, tot);
        if (pass) {
            const int o = n_gate + r;
            gidx[o] = i;
            gxyz[3 * o] = x; gxyz[3 * o + 1] = y; gxyz[3 * o + 2] = z;
        }
        n_ok += tot_ok; n_gate += tot;
    }
    if (threadIdx.x == 0) { out[0] = n_ok; out[1] = n_gate; out[2] = 0; out[3] = 0; out[4] = 0; out[5] = 0; out[6] = 0; out[7] = 0; }
}

// tracking.cc:254-263: the points of rank 0 in keypoint order; every clustered point's labels go back to its keypoint
__global__ __launch_bounds__(DB_BLOCK) void k_si_select(int n, const int* __restrict__ gidx, const float* __restrict__ gxyz,
                                                        const int* __restrict__ raw, const int* __restrict__ label, const int* __restrict__ counts,
                                                        int* out, SiPacked P) {
    __shared__ int s_wave[DB_BLOCK / 64];
    float* of = reinterpret_cast<float*>(out);
    const int m = min(out[1], n);
    int n_sel = 0;
    for (int c0 = 0; c0 < m; c0 += DB_BLOCK) {
        const int o = c0 + (int)threadIdx.x;
        bool sel = false;
        int i = 0;
        if (o < m) {
            i = gidx[o];
            const int l = label[o];
            sel = l == 0;
            out[P.raw + i] = raw[o];
            out[P.label + i] = l;
            out[P.code + i] = sel ? 0 : 3;
        }
        int tot;
        const int r = db_block_rank(sel, s_wave, tot);
        if (sel) {
            const int s = n_sel + r;
            out[P.selected + s] = i;
            of[P.sel_xyz + 3 * s] = gxyz[3 * o]; of[P.sel_xyz + 3 * s + 1] = gxyz[3 * o + 1]; of[P.sel_xyz + 3 * s + 2] = gxyz[3 * o + 2];
        }
        n_sel += tot;
    }
    if (threadIdx.x == 0) { out[2] = counts[0]; out[3] = counts[1]; out[4] = n_sel; out[5] = counts[2]; }
}

}  // namespace
}  // namespace nrs

using namespace nrs;

extern "C" int nrs_dbscan3d(nrs_ctx* c, int32_t n, const float* xyz, double eps, int32_t min_points, int32_t noise_competes, int32_t* raw_label,
                            int32_t* label, int32_t counts[3]) {
    if (!c) return NRS_ERR_INVALID;
    char msg[256];
    if (dbscan_check_args(n, xyz, eps, min_points, label, counts, msg, sizeof msg) != 0) return c->fail(NRS_ERR_INVALID, "%s", msg);
    counts[0] = counts[1] = counts[2] = 0;
    if (n == 0) return NRS_OK;
    NRS_HIP(c, hipSetDevice(c->device));
    // in: m | xyz[3n];  out: counts[4] | raw[n] | label[n], one download
    const size_t in_bytes = padded(sizeof(int)) + padded(sizeof(float) * 3 * (size_t)n), out_words = 4 + 2 * (size_t)n;
    const size_t bytes = in_bytes + padded(sizeof(int) * out_words) + db_ws_bytes(n);
    DevBuf big;                                                    // (freed when the call returns)
    NRS_TRY(c->ensure(big, bytes));
    Carver cv(big.as<char>());
    int* d_m = cv.take<int>(1);
    float* d_xyz = cv.take<float>(3 * (size_t)n);
    int* d_out = cv.take<int>(out_words);
    const DbWs w = db_carve(big.as<char>() + cv.used, n);
    NRS_HIP(c, hipMemcpyAsync(d_m, &n, sizeof(int), hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(d_xyz, xyz, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    dbscan_enqueue(c, w, d_m, d_xyz, eps, min_points, noise_competes, d_out + 4, d_out + 4 + n, d_out);
    NRS_HIP(c, hipGetLastError());
    std::vector<int32_t> host(out_words);
    NRS_HIP(c, hipMemcpyAsync(host.data(), d_out, sizeof(int) * out_words, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    if (host[0] < 0 || host[0] > n || host[1] < 0 || host[1] > n || host[2] < 0 || host[2] > n)
        return c->fail(NRS_ERR_HIP, "nrs_dbscan3d: the counts came back as (%d, %d, %d) for %d points", host[0], host[1], host[2], n);
    counts[0] = host[0]; counts[1] = host[1]; counts[2] = host[2];
    if (raw_label) memcpy(raw_label, host.data() + 4, sizeof(int32_t) * (size_t)n);
    memcpy(label, host.data() + 4 + n, sizeof(int32_t) * (size_t)n);
    return NRS_OK;
}

extern "C" void nrs_init_stereo_options_init(nrs_init_stereo_options* opt) {
    if (opt) sinit_options_init(opt);
}

// Both entry points: nrs_init_stereo (host images: ONE upload of the two images and the keypoints) and nrs_init_stereo_front (on_device: left /
// right are the packed resident images of nrs_front_process_stereo, only the keypoints go up).  Everything behind the upload is shared.
static int sinit_run(nrs_ctx* c, const char* who, const nrs_camera* cam, const nrs_init_stereo_options* opt, const uint8_t* left, const uint8_t* right,
                     bool on_device, int32_t w, int32_t h, int32_t stride_l, int32_t stride_r, int32_t n, const float* xy, nrs_init_stereo_result* out) {
    char msg[256];
    if (sinit_check_args(opt, out, n, msg, sizeof msg) != 0) return c->fail(NRS_ERR_INVALID, "%s", msg);
    NRS_TRY(stereo_match_check(c, who, cam, left, right, w, h, stride_l, stride_r, n, xy != nullptr));
    sinit_clear(out);
    if (n == 0) return NRS_OK;
    NRS_HIP(c, hipSetDevice(c->device));
    const SinitUpload U(on_device ? 0 : (size_t)w, on_device ? 0 : (size_t)h, (size_t)n);     // (resident images: the upload is the keypoints alone)
    const SinitLayout L((size_t)n);
    const size_t ws_bytes = stereo_match_ws_bytes(c, w, h, n);
    const size_t bytes = padded(U.bytes) + ws_bytes + padded(sizeof(double) * n) + padded(sizeof(int) * 2 * n) + padded(sizeof(int) * L.words) +
                         padded(sizeof(int) * n) + padded(sizeof(float) * 3 * n) + 2 * padded(sizeof(int) * n) + padded(sizeof(int) * 4) + db_ws_bytes(n);
    DevBuf big;                                                    // (freed when the call returns)
    NRS_TRY(c->ensure(big, bytes));
    Carver cv(big.as<char>());
    char* d_in = cv.take<char>(U.bytes);
    char* d_ws = cv.take<char>(ws_bytes);
    double* d_score = cv.take<double>(n);
    int* d_match = cv.take<int>(2 * (size_t)n);
    int* d_out = cv.take<int>(L.words);
    int* d_gidx = cv.take<int>(n);
    float* d_gxyz = cv.take<float>(3 * (size_t)n);
    int* d_raw = cv.take<int>(n);
    int* d_label = cv.take<int>(n);
    int* d_counts = cv.take<int>(4);
    const DbWs dw = db_carve(big.as<char>() + cv.used, n);
    if (cv.used + db_ws_bytes(n) > bytes) return c->fail(NRS_ERR_STATE, "%s: workspace accounting", who);
    std::vector<char> up(U.bytes);
    sinit_pack_upload(U, left, stride_l, right, stride_r, xy, up.data());                                // (on_device: zero image rows, the keypoints only)
    NRS_HIP(c, hipMemcpyAsync(d_in, up.data(), U.bytes, hipMemcpyHostToDevice, c->stream));              // the one upload
    const uint8_t* d_left = on_device ? left : reinterpret_cast<const uint8_t*>(d_in + U.left);
    const uint8_t* d_right = on_device ? right : reinterpret_cast<const uint8_t*>(d_in + U.right);
    const float* d_xy = reinterpret_cast<const float*>(d_in + U.xy);
    const SiPacked P{(unsigned)L.xyz, (unsigned)L.status, (unsigned)L.code, (unsigned)L.raw, (unsigned)L.label, (unsigned)L.selected, (unsigned)L.sel_xyz};
    NRS_TRY(stereo_match_enqueue(c, cam, opt->bf, w, h, n, d_left, d_right, d_xy, d_ws, reinterpret_cast<float*>(d_out + L.xyz), d_out + L.status,
                                 d_score, d_match));
    hipLaunchKernelGGL(k_si_gate, dim3(1), dim3(DB_BLOCK), 0, c->stream, n, opt->z_min, opt->z_max, d_out, P, d_gidx, d_gxyz);
    dbscan_enqueue(c, dw, d_out + 1, d_gxyz, opt->eps, opt->min_points, opt->noise_competes, d_raw, d_label, d_counts);
    hipLaunchKernelGGL(k_si_select, dim3(1), dim3(DB_BLOCK), 0, c->stream, n, d_gidx, d_gxyz, d_raw, d_label, d_counts, d_out, P);
    NRS_HIP(c, hipGetLastError());
    std::vector<int32_t> packed(L.words);
    NRS_HIP(c, hipMemcpyAsync(packed.data(), d_out, sizeof(int) * L.words, hipMemcpyDeviceToHost, c->stream));   // the one download
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    if (sinit_unpack(packed.data(), n, out) != 0) {
        sinit_clear(out);
        return c->fail(NRS_ERR_HIP, "%s: the packed result's header (%d, %d, %d, %d, %d, %d) contradicts itself for %d keypoints", who, packed[0],
                       packed[1], packed[2], packed[3], packed[4], packed[5], n);
    }
    return NRS_OK;
}

extern "C" int nrs_init_stereo(nrs_ctx* c, const nrs_camera* cam, const nrs_init_stereo_options* opt, const uint8_t* left, const uint8_t* right,
                               int32_t w, int32_t h, int32_t stride_l, int32_t stride_r, int32_t n, const float* xy, nrs_init_stereo_result* out) {
    if (!c) return NRS_ERR_INVALID;
    return sinit_run(c, "nrs_init_stereo", cam, opt, left, right, false, w, h, stride_l, stride_r, n, xy, out);
}

extern "C" int nrs_init_stereo_front(nrs_ctx* c, const nrs_camera* cam, const nrs_init_stereo_options* opt, int32_t w, int32_t h, int32_t image,
                                     int32_t n, const float* xy, nrs_init_stereo_result* out) {
    if (!c) return NRS_ERR_INVALID;
    const uint8_t *left = nullptr, *right = nullptr;
    NRS_TRY(front_resident_pair(c, "nrs_init_stereo_front", w, h, image, &left, &right));
    return sinit_run(c, "nrs_init_stereo_front", cam, opt, left, right, true, w, h, w, w, n, xy, out);
}

// Both flow-clustering entry points: ONE upload (the count and the caller's floats), the launches, ONE packed download.  length = 0: the
// floats are n x dim points; otherwise n x length x 2 keypoints, and k_flow_build writes the points into the download's flows
static int dbnd_run(nrs_ctx* c, const char* who, int n, int dim, int length, const float* in, double eps, int min_points, float* flows_out,
                    int32_t* label, int32_t counts[2]) {
    NRS_HIP(c, hipSetDevice(c->device));
    const FlowcScratch S((size_t)n, (size_t)dim, (size_t)length);
    DevBuf big;                                                    // (freed when the call returns)
    NRS_TRY(c->ensure(big, S.bytes));
    char* base = big.as<char>();
    int* d_m = reinterpret_cast<int*>(base + S.m);
    float* d_in = reinterpret_cast<float*>(base + S.in);
    int* d_out = reinterpret_cast<int*>(base + S.out);
    float* d_flows = reinterpret_cast<float*>(d_out + S.flows_word);
    const DbWs w = db_carve(base + S.rows, n);
    std::vector<char> up(S.up_bytes, 0);
    memcpy(up.data() + S.m, &n, sizeof(int));
    memcpy(up.data() + S.in, in, sizeof(float) * S.in_floats);
    NRS_HIP(c, hipMemcpyAsync(base, up.data(), S.up_bytes, hipMemcpyHostToDevice, c->stream));            // the one upload
    if (length) {
        const size_t steps = (size_t)n * (length - 1);
        hipLaunchKernelGGL(k_flow_build, dim3((unsigned)((steps + 255) / 256)), dim3(256), 0, c->stream, n, length, d_in, d_flows);
    }
    dbscan_nd_enqueue(c, w, d_m, dim, length ? d_flows : d_in, eps, min_points, d_out + 4, d_out);
    NRS_HIP(c, hipGetLastError());
    std::vector<int32_t> host(S.out_words);
    NRS_HIP(c, hipMemcpyAsync(host.data(), d_out, sizeof(int) * S.out_words, hipMemcpyDeviceToHost, c->stream));   // the one download
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    if (host[0] < 0 || host[0] > n || host[1] < 0 || host[1] > n)
        return c->fail(NRS_ERR_HIP, "%s: the counts came back as (%d, %d) for %d points", who, host[0], host[1], n);
    counts[0] = host[0]; counts[1] = host[1];
    memcpy(label, host.data() + 4, sizeof(int32_t) * (size_t)n);
    if (length && flows_out) memcpy(flows_out, host.data() + S.flows_word, sizeof(float) * (size_t)n * dim);
    return NRS_OK;
}

extern "C" int nrs_dbscan_nd(nrs_ctx* c, int32_t n, int32_t dim, const float* data, double eps, int32_t min_points, int32_t* label,
                             int32_t counts[2]) {
    if (!c) return NRS_ERR_INVALID;
    char msg[256];
    if (dbscan_nd_check_args(n, dim, data, eps, min_points, label, counts, msg, sizeof msg) != 0) return c->fail(NRS_ERR_INVALID, "%s", msg);
    counts[0] = counts[1] = 0;
    if (n == 0) return NRS_OK;
    return dbnd_run(c, "nrs_dbscan_nd", n, dim, 0, data, eps, min_points, nullptr, label, counts);
}

extern "C" int nrs_flow_tracks_cluster(nrs_ctx* c, int32_t n_tracks, int32_t length, const float* tracks_xy, float* flows_out, int32_t* label,
                                       int32_t counts[2]) {
    if (!c) return NRS_ERR_INVALID;
    char msg[256];
    if (flow_tracks_check_args(n_tracks, length, tracks_xy, label, counts, msg, sizeof msg) != 0) return c->fail(NRS_ERR_INVALID, "%s", msg);
    counts[0] = counts[1] = 0;
    if (n_tracks == 0) return NRS_OK;
    const int dim = flowc_dim(length);
    return dbnd_run(c, "nrs_flow_tracks_cluster", n_tracks, dim, length, tracks_xy, flowc_eps(dim), FLOWC_MIN_POINTS, flows_out, label, counts);
}
