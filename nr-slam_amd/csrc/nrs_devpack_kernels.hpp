// Kernels of the device-side problem construction for plain deformable-BA windows (part of nrs_engine.hip; the staged build that
// launches them and the description of what they reproduce: nrs_engine_devpack.hpp).
#pragma once

namespace nrs {

constexpr int DP_HCAP = 2048, DP_HASH = 4096;

__device__ inline uint64_t dp_spread(uint64_t v) {                  // 21 bits -> every third bit (the host packer's `spread`)
    v &= 0x1fffff;
    v = (v | v << 32) & 0x1f00000000ffffULL;
    v = (v | v << 16) & 0x1f0000ff0000ffULL;
    v = (v | v << 8) & 0x100f00f00f00f00fULL;
    v = (v | v << 4) & 0x10c30c30c30c30c3ULL;
    v = (v | v << 2) & 0x1249249249249249ULL;
    return v;
}

// min / max of the vertex positions (fp64 of the caller's floats): one workgroup, fixed order (min / max are order-free)
__global__ __launch_bounds__(1024) void k_dp_minmax(int M, const double* __restrict__ xyz, double* out /*6*/) {
    __shared__ double lo[3][1024], hi[3][1024];
    const int tid = threadIdx.x;
    double l[3] = {1e300, 1e300, 1e300}, h[3] = {-1e300, -1e300, -1e300};
    for (int v = tid; v < M; v += 1024)
        for (int a = 0; a < 3; ++a) { const double p = xyz[3 * (size_t)v + a]; l[a] = fmin(l[a], p); h[a] = fmax(h[a], p); }
    for (int a = 0; a < 3; ++a) { lo[a][tid] = l[a]; hi[a][tid] = h[a]; }
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s)
            for (int a = 0; a < 3; ++a) { lo[a][tid] = fmin(lo[a][tid], lo[a][tid + s]); hi[a][tid] = fmax(hi[a][tid], hi[a][tid + s]); }
        __syncthreads();
    }
    if (tid < 3) { out[tid] = lo[tid][0]; out[3 + tid] = hi[tid][0]; }
}

__global__ void k_dp_morton(int M, const double* __restrict__ xyz, const double* __restrict__ mm, int morton, uint64_t* code, int* val) {
#pragma clang fp contract(off)
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= M) return;
    uint64_t c = 0;
    if (morton)
        for (int a = 0; a < 3; ++a) {
            const double ext = mm[3 + a] - mm[a];
            const double f = ext > 0 ? (xyz[3 * (size_t)v + a] - mm[a]) / ext : 0.0;
            c |= dp_spread((uint64_t)(f * 2097151.0)) << a;
        }
    code[v] = c;
    val[v] = v;
}

// vertex -> row after the per-keyframe sort: sorted position i of keyframe k -> row pose_grp_ptr[k] * 256 + (i - pose_ptr[k])
__global__ void k_dp_rows0(int M, const int* __restrict__ sorted_v, const int* __restrict__ lm_kf, const int* __restrict__ pose_ptr,
                           const int* __restrict__ pose_grp_ptr, int* vrow, int* row_v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const int v = sorted_v[i], k = lm_kf[v];
    const int r = pose_grp_ptr[k] * ROW_ALIGN + (i - pose_ptr[k]);
    vrow[v] = r;
    row_v[r] = v;
}

// incidence counts per VERTEX (tile sort keys)
__global__ void k_dp_vcounts(int n_sp, const int* __restrict__ sp_ij, int n_dm, const int* __restrict__ dm_idx, int* cs, int* cd) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * (int64_t)n_sp) atomicAdd(&cs[sp_ij[i]], 1);
    if (i < 4 * (int64_t)n_dm) atomicAdd(&cd[dm_idx[i]], 1);
}

// tile sort key of a row: (damper count desc, spring count desc), padding rows last; the segmented sort is stable
__global__ void k_dp_tilekeys(int n_rows, const int* __restrict__ row_v, const int* __restrict__ cs, const int* __restrict__ cd, uint32_t* key, int* val) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const int v = row_v[r];
    key[r] = v < 0 ? 0xFFFFFFFFu : (((uint32_t)(0x7FFF - min(cd[v], 0x7FFF)) << 16) | (uint32_t)(0xFFFF - min(cs[v], 0xFFFF)));
    val[r] = v;
}
__global__ void k_dp_rows1(int n_rows, const int* __restrict__ sorted_v, int* vrow) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const int v = sorted_v[r];
    if (v >= 0) vrow[v] = r;
}

// rows of every incidence + counts per row + sort keys (row << 32 | sequence number in the host's fill order)
__global__ void k_dp_inc(int n_sp, const int* __restrict__ sp_ij, int n_dm, const int* __restrict__ dm_idx, const int* __restrict__ vrow,
                         int* cnt_s, int* cnt_d, uint64_t* key_s, uint64_t* key_d) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * (int64_t)n_sp) {
        const int r = vrow[sp_ij[i]];
        atomicAdd(&cnt_s[r], 1);
        key_s[i] = ((uint64_t)(uint32_t)r << 32) | (uint64_t)(uint32_t)i;
    }
    if (i < 4 * (int64_t)n_dm) {
        const int r = vrow[dm_idx[i]];
        atomicAdd(&cnt_d[r], 1);
        key_d[i] = ((uint64_t)(uint32_t)r << 32) | (uint64_t)(uint32_t)i;
    }
}

// ---- a rank of a sharded window: the incidences of rows in [lo, hi) only.  Counts first (the record-side scratch is sized from
// them), then the keys, compacted: a workgroup reserves its share of the output with one atomic per list -- the order this leaves
// is arbitrary and does not matter, the keys are distinct and the radix sorts that follow put them in (row, sequence) order.
// tot / cur [0..4): spring incidences, damper incidences, springs counted here (first endpoint owned), dampers counted here
__global__ __launch_bounds__(256) void k_dp_count_own(int n_sp, const int* __restrict__ sp_ij, int n_dm, const int* __restrict__ dm_idx, const int* __restrict__ vrow,
                                                      int lo, int hi, int* cnt_s, int* cnt_d, int* tot) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int es = 0, ed = 0;
    if (i < 2 * (int64_t)n_sp) {
        const int r = vrow[sp_ij[i]];
        if (r >= lo && r < hi) { atomicAdd(&cnt_s[r], 1); es = !(i & 1); }
    }
    if (i < 4 * (int64_t)n_dm) {
        const int r = vrow[dm_idx[i]];
        if (r >= lo && r < hi) { atomicAdd(&cnt_d[r], 1); ed = !(i & 3); }
    }
    const int ns = __syncthreads_count(es), nd = __syncthreads_count(ed);
    if (threadIdx.x == 0) { if (ns) atomicAdd(&tot[2], ns); if (nd) atomicAdd(&tot[3], nd); }
}
__global__ __launch_bounds__(256) void k_dp_keys_own(int n_sp, const int* __restrict__ sp_ij, int n_dm, const int* __restrict__ dm_idx, const int* __restrict__ vrow,
                                                     int lo, int hi, uint64_t* key_s, uint64_t* key_d, uint64_t* ek_s, uint64_t* ek_d, int* cur) {
    __shared__ int n_loc[4], base[4];
    const int tid = threadIdx.x;
    if (tid < 4) n_loc[tid] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + tid;
    int rs = -1, rd = -1, ps = 0, pd = 0, pes = -1, ped = -1;
    if (i < 2 * (int64_t)n_sp) {
        const int r = vrow[sp_ij[i]];
        if (r >= lo && r < hi) { rs = r; ps = atomicAdd(&n_loc[0], 1); if (!(i & 1)) pes = atomicAdd(&n_loc[2], 1); }
    }
    if (i < 4 * (int64_t)n_dm) {
        const int r = vrow[dm_idx[i]];
        if (r >= lo && r < hi) { rd = r; pd = atomicAdd(&n_loc[1], 1); if (!(i & 3)) ped = atomicAdd(&n_loc[3], 1); }
    }
    __syncthreads();
    if (tid < 4) base[tid] = n_loc[tid] ? atomicAdd(&cur[tid], n_loc[tid]) : 0;
    __syncthreads();
    if (rs >= 0) {
        key_s[base[0] + ps] = ((uint64_t)(uint32_t)rs << 32) | (uint64_t)(uint32_t)i;
        if (pes >= 0) ek_s[base[2] + pes] = ((uint64_t)(uint32_t)rs << 32) | (uint64_t)(uint32_t)(i >> 1);
    }
    if (rd >= 0) {
        key_d[base[1] + pd] = ((uint64_t)(uint32_t)rd << 32) | (uint64_t)(uint32_t)i;
        if (ped >= 0) ek_d[base[3] + ped] = ((uint64_t)(uint32_t)rd << 32) | (uint64_t)(uint32_t)(i >> 2);
    }
}

// slice widths (x 64): a slice = 64 / T rows, T lanes per row
__global__ void k_dp_widths(int n_slices, int T, const int* __restrict__ cnt_s, const int* __restrict__ cnt_d, int* ws, int* wd) {
    const int sl = blockIdx.x * blockDim.x + threadIdx.x;
    if (sl >= n_slices) return;
    const int Rw = 64 / T;
    int a = 0, b = 0;
    for (int r = 0; r < Rw; ++r) { a = max(a, (cnt_s[sl * Rw + r] + T - 1) / T); b = max(b, (cnt_d[sl * Rw + r] + T - 1) / T); }
    ws[sl] = a * 64;
    wd[sl] = b * 64;
}

__device__ inline size_t dp_pos_of(const int* ptr, int T, int row, int k) {  // packed position of the k-th incidence of a row
    const int Rw = 64 / T, sl = row / Rw, r = row - sl * Rw;
    return (size_t)ptr[sl] + (size_t)(k / T) * 64 + (size_t)r * T + (size_t)(k % T);
}

// fill: sorted incidence i of a row -> its sliced-ELL slot (global neighbour rows; the halo pass turns them into tile-local ids)
__global__ void k_dp_fill_s(int64_t n, int T, const uint64_t* __restrict__ key, const int* __restrict__ row_start, const int* __restrict__ ss_ptr,
                            const int* __restrict__ sp_ij, const float* __restrict__ sp_d0, const int* __restrict__ vrow,
                            int* S_other, float* S_d0, uint8_t* S_side) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int row = (int)(key[i] >> 32);
    const uint32_t seq = (uint32_t)key[i];
    const size_t p = dp_pos_of(ss_ptr, T, row, (int)(i - row_start[row]));
    S_other[p] = vrow[sp_ij[seq ^ 1u]];
    S_d0[p] = sp_d0[seq >> 1];
    S_side[p] = (uint8_t)(1 + (seq & 1u));                           // 1: first endpoint (counts the edge's chi2), 2: second
}
__global__ void k_dp_fill_d(int64_t n, int T, const uint64_t* __restrict__ key, const int* __restrict__ row_start, const int* __restrict__ sd_ptr,
                            const int* __restrict__ dm_idx, const float* __restrict__ dm_w, const int* __restrict__ vrow,
                            int* D_o, float* D_w, int8_t* D_role) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int row = (int)(key[i] >> 32);
    const uint32_t seq = (uint32_t)key[i];
    const int role = (int)(seq & 3u);
    const size_t q = seq >> 2, p = dp_pos_of(sd_ptr, T, row, (int)(i - row_start[row]));
    int z = 0;
    for (int k = 0; k < 4; ++k)
        if (k != role) D_o[3 * p + z++] = vrow[dm_idx[4 * q + k]];
    D_w[p] = dm_w[q];
    D_role[p] = (int8_t)role;
}

// ---- halo of a tile: the rows its incidences reference outside its own 128 rows.  PASS 0 counts (hs, ns), PASS 1 writes
// the lists and the final incidence headers.  LDS: open-addressing hash set (row, seen-by-a-spring flag), then a bitonic sort
// of (damper-only << 31 | row).  The grid covers tiles [b0, b0 + gridDim.x): a rank of a sharded window runs its own tiles only
// (the others have empty lists) and takes from pass 0 the smallest / largest halo row of every tile as well (hmin / hmax: the
// shard fields are derived from them, nrs_engine_setup.hpp "shard window").
template <int PASS>
__global__ __launch_bounds__(256) void k_dp_halo(int b0, int* hmin, int* hmax, int tile_rows, int T, uint16_t* row_tp16, const int* __restrict__ ss_ptr, const int* __restrict__ sd_ptr, const int* __restrict__ S_other,
                                                 const uint8_t* __restrict__ S_side, const int* __restrict__ D_o, const int8_t* __restrict__ D_role,
                                                 int* hs, int* hns, const int* __restrict__ halo_ptr, int* halo_rows, uint32_t* s_om, uint2* d_hdr,
                                                 int* overflow) {
    __shared__ uint32_t hk[DP_HASH];                                 // row + 1 (0 = empty)
    __shared__ uint32_t hf[DP_HASH];                                 // 1 = referenced by a spring
    __shared__ uint32_t keys[DP_HCAP];
    __shared__ int cnt, cnt_s, row_mn, row_mx;
    const int b = b0 + blockIdx.x, tid = threadIdx.x;
    const int row0 = b * tile_rows, row1 = row0 + tile_rows;
    for (int i = tid; i < DP_HASH; i += 256) { hk[i] = 0; hf[i] = 0; }
    if (tid == 0) { cnt = 0; cnt_s = 0; row_mn = 0x7FFFFFFF; row_mx = -1; }
    __syncthreads();
    const int s0 = ss_ptr[b * 4], s1 = ss_ptr[b * 4 + 4], d0 = sd_ptr[b * 4], d1 = sd_ptr[b * 4 + 4];
    auto insert = [&](int o, uint32_t spring) {
        if (o < 0 || (o >= row0 && o < row1)) return;
        uint32_t h = ((uint32_t)o * 2654435761u) >> 20;              // 12 bits
        for (int probe = 0; probe < DP_HASH; ++probe, h = (h + 1) & (DP_HASH - 1)) {
            const uint32_t old = atomicCAS(&hk[h], 0u, (uint32_t)o + 1u);
            if (old == 0u || old == (uint32_t)o + 1u) { if (spring) atomicOr(&hf[h], 1u); return; }
        }
        atomicExch(overflow, 1);
    };
    for (int p = s0 + tid; p < s1; p += 256) insert(S_other[p], 1u);
    __syncthreads();
    for (int64_t p = 3 * (int64_t)d0 + tid; p < 3 * (int64_t)d1; p += 256) insert(D_o[p], 0u);
    __syncthreads();
    for (int i = tid; i < DP_HCAP; i += 256) keys[i] = 0xFFFFFFFFu;
    __syncthreads();
    for (int i = tid; i < DP_HASH; i += 256) {
        if (hk[i]) {
            const int j = atomicAdd(&cnt, 1);
            if (hf[i]) atomicAdd(&cnt_s, 1);
            if (j < DP_HCAP) keys[j] = (hf[i] ? 0u : 0x80000000u) | (hk[i] - 1u);
            if (PASS == 0 && hmin) { atomicMin(&row_mn, (int)(hk[i] - 1u)); atomicMax(&row_mx, (int)(hk[i] - 1u)); }
        }
    }
    __syncthreads();
    const int n = cnt, ns = cnt_s;
    if (PASS == 0 && hmin && tid == 0) { hmin[b] = row_mn; hmax[b] = row_mx; }
    if (n > DP_HCAP) { if (tid == 0) atomicExch(overflow, 1); if (PASS == 0 && tid == 0) { hs[b] = n; hns[b] = ns; } return; }
    if (PASS == 0) { if (tid == 0) { hs[b] = n; hns[b] = ns; } return; }
    // bitonic sort of keys[0 .. 2048): spring part first (bit 31 clear), each part ascending by row; padding (0xFFFFFFFF) last
    for (int k = 2; k <= DP_HCAP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < DP_HCAP; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const uint32_t a = keys[i], c = keys[l];
                    const bool up = (i & k) == 0;
                    if ((a > c) == up) { keys[i] = c; keys[l] = a; }
                }
            }
            __syncthreads();
        }
    const int hb = halo_ptr[b];
    for (int i = tid; i < n; i += 256) halo_rows[hb + i] = (int)(keys[i] & 0x7FFFFFFFu);
    auto loc = [&](int o) -> uint32_t {                              // tile-local id as u16 (REC_NONE: no neighbour)
        if (o < 0) return (uint32_t)REC_NONE;
        if (o >= row0 && o < row1) return (uint32_t)(o - row0);
        // spring part [0, ns), damper-only part [ns, n): binary search in both
        int lo = 0, hi = ns;
        while (lo < hi) { const int m = (lo + hi) >> 1; if ((keys[m] & 0x7FFFFFFFu) < (uint32_t)o) lo = m + 1; else hi = m; }
        if (lo < ns && (keys[lo] & 0x7FFFFFFFu) == (uint32_t)o) return (uint32_t)(tile_rows + lo);
        lo = ns; hi = n;
        while (lo < hi) { const int m = (lo + hi) >> 1; if ((keys[m] & 0x7FFFFFFFu) < (uint32_t)o) lo = m + 1; else hi = m; }
        return (uint32_t)(tile_rows + lo);
    };
    // springs: {other u16 | meta u16 << 16}, meta = SR_ACTIVE | SR_COUNT on the edge's first endpoint; padding: other = REC_NONE, meta 0
    for (int p = s0 + tid; p < s1; p += 256) {
        const int o = S_other[p];
        const uint32_t side = S_side[p];
        const uint32_t m16 = o < 0 ? 0u : (uint32_t)(SR_ACTIVE | (side == 1 ? SR_COUNT : 0));
        s_om[p] = loc(o) | (m16 << 16);
    }
    // dampers: the three others in canonical order (engine_create: perm), meta = role | DM_ACTIVE | DM_COUNT on role 0
    for (int p = d0 + tid; p < d1; p += 256) {
        const int role = D_role[p];
        if (role < 0) { d_hdr[p] = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu); continue; }
        const int pm0 = role < 2 ? 0 : 2, pm1 = (role == 0) ? 1 : (role == 1 ? 2 : (role == 2 ? 0 : 1)), pm2 = (role == 0) ? 2 : (role == 1 ? 1 : (role == 2 ? 1 : 0));
        const uint32_t l0 = loc(D_o[3 * (size_t)p + pm0]), l1 = loc(D_o[3 * (size_t)p + pm1]), l2 = loc(D_o[3 * (size_t)p + pm2]);
        const uint32_t m16 = (uint32_t)(role | DM_ACTIVE | (role == 0 ? DM_COUNT : 0));
        d_hdr[p] = make_uint2(l0 | (l1 << 16), l2 | (m16 << 16));
        // the row's own temporal partner (l1): next for roles 1c / 2c, previous for 1n / 2n -- the same for all of its dampers
        const int sl = b * 4 + (p >= sd_ptr[b * 4 + 1]) + (p >= sd_ptr[b * 4 + 2]) + (p >= sd_ptr[b * 4 + 3]);
        const int row = sl * (64 / T) + ((p - sd_ptr[sl]) & 63) / T;
        row_tp16[2 * (size_t)row + (role < 2 ? 0 : 1)] = (uint16_t)l1;
    }
    __syncthreads();
    for (int p = d0 + tid; p < d1; p += 256) {                       // ... which is verified, not assumed
        const int role = D_role[p];
        if (role < 0) continue;
        const int sl = b * 4 + (p >= sd_ptr[b * 4 + 1]) + (p >= sd_ptr[b * 4 + 2]) + (p >= sd_ptr[b * 4 + 3]);
        const int row = sl * (64 / T) + ((p - sd_ptr[sl]) & 63) / T;
        if (row_tp16[2 * (size_t)row + (role < 2 ? 0 : 1)] != (uint16_t)(d_hdr[p].x >> 16)) atomicExch(overflow + 1, 1);
    }
}

// chi2 edge lists: keys (counting row << 32 | edge), then the records in sorted order
__global__ void k_dp_eckeys(int n_sp, const int* __restrict__ sp_ij, int n_dm, const int* __restrict__ dm_idx, const int* __restrict__ vrow,
                            uint64_t* ks, uint64_t* kd) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_sp) ks[i] = ((uint64_t)(uint32_t)vrow[sp_ij[2 * (size_t)i]] << 32) | (uint32_t)i;
    if (i < n_dm) kd[i] = ((uint64_t)(uint32_t)vrow[dm_idx[4 * (size_t)i]] << 32) | (uint32_t)i;
}
__global__ void k_dp_ecfill(int n_sp, const uint64_t* __restrict__ ks, const int* __restrict__ sp_ij, const float* __restrict__ sp_d0, int n_dm,
                            const uint64_t* __restrict__ kd, const int* __restrict__ dm_idx, const float* __restrict__ dm_w, const int* __restrict__ vrow,
                            EcSpring* ec_sp, EcDamper* ec_dm, float* ec_w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_sp) {
        const uint32_t q = (uint32_t)ks[i];
        ec_sp[i] = EcSpring{vrow[sp_ij[2 * (size_t)q]], vrow[sp_ij[2 * (size_t)q + 1]], sp_d0[q], 0};
    }
    if (i < n_dm) {
        const uint32_t q = (uint32_t)kd[i];
        EcDamper e;
        for (int k = 0; k < 4; ++k) e.r[k] = vrow[dm_idx[4 * (size_t)q + k]];
        ec_dm[i] = e;
        ec_w[i] = dm_w[q];
    }
}

// per-row data from per-vertex data (padding rows: fixed, no observation, zeros)
// (rows [r0, r1): every row, or the rows a rank of a sharded window holds -- the arrays are addressed by the global row)
__global__ void k_dp_rowdata(int r0, int r1, const int* __restrict__ row_v, const double* __restrict__ xyz, const float* __restrict__ uv_in,
                             uint8_t* rflag, float* uv, double* xl) {
    const int r = r0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= r1) return;
    const int v = row_v[r];
    rflag[r] = v < 0 ? (uint8_t)RF_FIXED : (uint8_t)(RF_OBS | RF_REPROJ_ACTIVE);
    uv[2 * (size_t)r] = v < 0 ? 0.f : uv_in[2 * (size_t)v];
    uv[2 * (size_t)r + 1] = v < 0 ? 0.f : uv_in[2 * (size_t)v + 1];
    for (int a = 0; a < 3; ++a) xl[3 * (size_t)r + a] = v < 0 ? 0.0 : xyz[3 * (size_t)v + a];
}
__global__ void k_dp_rowcnt(int r0, int r1, const int* __restrict__ cnt_s, const int* __restrict__ cnt_d, uint32_t* out) {
    const int r = r0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (r < r1) out[r] = (uint32_t)cnt_s[r] | ((uint32_t)cnt_d[r] << 16);
}
__global__ void k_dp_rowv(int M, const int* __restrict__ vrow, int* row_v) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < M) row_v[vrow[v]] = v;
}

// fused single-launch path: the first BLK halo rows of every tile at a fixed stride (no pointer chase in k_pcg_fused)
// (plain two-kernel path: the first HALO_FIX rows, -1 behind the list's end -- stage_rows<true>)
__global__ void k_dp_halofix(int n_tiles, const int* __restrict__ halo_ptr, const int* __restrict__ halo_rows, int* halo_fix, int stride, int pad) {
    const int b = blockIdx.x;
    if (b >= n_tiles) return;
    const int hb = halo_ptr[b], hn = halo_ptr[b + 1] - hb;
    for (int i = threadIdx.x; i < stride; i += blockDim.x) halo_fix[(size_t)b * stride + i] = i < hn ? halo_rows[hb + i] : pad;
}

}  // namespace nrs
