// f6: monocular map initialisation -- EssentialMatrixInitialization::Initialize (reference
// modules/tracking/essential_matrix_initialization.cc:47-410) in one call: one upload, three launches, one download.
//   k_init_prepare      one workgroup: compaction of the TRACKED keypoints + their rays (:83-103), and the sampler -- farthest-point seeds,
//                       <= 10 Lloyd iterations, member lists, the hashed picks (this project's definition, DESIGN.md "f6")
//   k_init_hypotheses   one wave per hypothesis: A (8 x 9, fp32 as written, :183-188), its right null vector and the 3 x 3 SVD by a one-sided
//                       Jacobi in fp64 on LDS (no register array is indexed at run time), Ef rounded to fp32, then the score over the first
//                       n_matches compact rays (:236-256) with the lanes striding the points
//   k_init_reconstruct  one workgroup: arg-max (highest score, lowest h), the inlier flags of the winner, DecomposeEssentialMatrix /
//                       ReconstructCameras (:284-318) and ReconstructPoints (:320-410) with the counters and the verdict
// The fp32 steps run with contraction off in the operation order of tests/init_oracle.py; no atomics (every count is a reduction).
#include <type_traits>
#include <cstdint>
#include <cstring>
#include <vector>
#include "nrs_ctx.hpp"
#include "nrs_device.hpp"
#include "nrs_geom_f32.hpp"

namespace nrs {

constexpr int IN_T = 1024;                  // threads of the two single-workgroup kernels
constexpr int IN_W = IN_T / 64;
constexpr int IN_MAXH = 4096;
constexpr int IN_HDR = 64;                  // words of the packed result header

struct InitArgs {
    Cam cam;
    int n, n_matches, n_hyp, nc, compact_indexing, have_samples, min_tri;
    float thr, rpp, max_low;
    unsigned long long seed;
    const float* ref_xy; const float* cur_xy; const int* status;      // n
    int* cmap; float* cxy; float* rref; float* rcur;                  // nc: keypoint index, reference keypoint, the two rays
    float* mind; int* members; int* cl_off;                           // sampler scratch: nc, nc, 9
    // packed result (one download): header words, then the arrays
    int* hdr; float* xyz; int* code; float* hyp_E; int* hyp_score; int* samples; int* labels; float* centres; uint8_t* inlier;
};
static_assert(std::is_trivially_copyable_v<InitArgs>, "passed to kernels by value: plain pointers, never an owner");

// ---- workgroup helpers (IN_T threads)
__device__ inline int block_excl_scan(int v, int* sm, int& total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int y = __shfl_up(x, off, 64); if (lane >= off) x += y; }
    if (lane == 63) sm[w] = x;
    __syncthreads();
    if (tid == 0) { int acc = 0; for (int i = 0; i < IN_W; ++i) { const int t = sm[i]; sm[i] = acc; acc += t; } sm[IN_W] = acc; }
    __syncthreads();
    const int excl = sm[w] + x - v;
    total = sm[IN_W];
    __syncthreads();
    return excl;
}
__device__ inline int block_sum_int(int v, int* sm) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int i = 0; i < IN_W; ++i) s += sm[i];
    __syncthreads();
    return s;
}
__device__ inline double block_sum_double(double v, double* sm) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0;
    for (int i = 0; i < IN_W; ++i) s += sm[i];
    __syncthreads();
    return s;
}
__device__ inline float dist2_f32(float ax, float ay, float bx, float by) {
#pragma clang fp contract(off)
    const float dx = ax - bx, dy = ay - by;
    return dx * dx + dy * dy;
}
// splitmix64 of seed + (k + 1) * golden
__device__ inline unsigned long long init_hash(unsigned long long seed, unsigned long long k) {
    unsigned long long z = seed + (k + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ inline void unit_ray_f32(const Cam& cam, const float* xy, float* r) {
#pragma clang fp contract(off)
    unproject_f32(cam, xy[0], xy[1], r);
    const float nn = normf3(r);
    r[0] /= nn; r[1] /= nn; r[2] /= nn;
}

__global__ __launch_bounds__(IN_T) void k_init_prepare(InitArgs A) {
    __shared__ int smi[IN_W + 1];
    __shared__ double smd[IN_W];
    __shared__ float cen[16], cen_new[16];
    __shared__ float bval[IN_W];
    __shared__ int bidx[IN_W];
    __shared__ int s_moved;
    const int tid = threadIdx.x, n = A.n;
    // ================= UnprojectTrackedFeatures: compact indices in ascending keypoint order
    const int chunk = (n + IN_T - 1) / IN_T;
    const int lo = min(n, tid * chunk), hi = min(n, lo + chunk);
    int cnt = 0;
    for (int i = lo; i < hi; ++i) cnt += A.status[i] == NRS_TRACKED;
    int total;
    int pos = block_excl_scan(cnt, smi, total);
    for (int i = lo; i < hi; ++i)
        if (A.status[i] == NRS_TRACKED) {
            A.cmap[pos] = i;
            A.cxy[2 * pos] = A.ref_xy[2 * i]; A.cxy[2 * pos + 1] = A.ref_xy[2 * i + 1];
            float r[3];
            unit_ray_f32(A.cam, A.ref_xy + 2 * i, r);
            A.rref[3 * pos] = r[0]; A.rref[3 * pos + 1] = r[1]; A.rref[3 * pos + 2] = r[2];
            unit_ray_f32(A.cam, A.cur_xy + 2 * i, r);
            A.rcur[3 * pos] = r[0]; A.rcur[3 * pos + 1] = r[1]; A.rcur[3 * pos + 2] = r[2];
            ++pos;
        }
    __syncthreads();
    const int nc = total;                      // == A.nc (the host counted the same flags)
    if (A.have_samples || nc < 8) return;
    // ================= seeds: farthest-point sampling, first = compact index 0, ties to the lowest index
    if (tid == 0) { cen[0] = A.cxy[0]; cen[1] = A.cxy[1]; }
    __syncthreads();
    for (int i = tid; i < nc; i += IN_T) A.mind[i] = dist2_f32(A.cxy[2 * i], A.cxy[2 * i + 1], cen[0], cen[1]);
    for (int k = 1; k < 8; ++k) {
        float bv = -1.f;
        int bi = 0x7fffffff;
        for (int i = tid; i < nc; i += IN_T) { const float d = A.mind[i]; if (d > bv) { bv = d; bi = i; } }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if ((tid & 63) == 0) { bval[tid >> 6] = bv; bidx[tid >> 6] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < IN_W; ++w)
                if (bval[w] > bv || (bval[w] == bv && bidx[w] < bi)) { bv = bval[w]; bi = bidx[w]; }
            if (bi == 0x7fffffff) bi = 0;          // (only NaN distances: keep the index in range)
            cen[2 * k] = A.cxy[2 * bi]; cen[2 * k + 1] = A.cxy[2 * bi + 1];
        }
        __syncthreads();
        const float px = cen[2 * k], py = cen[2 * k + 1];
        for (int i = tid; i < nc; i += IN_T) { const float d = dist2_f32(A.cxy[2 * i], A.cxy[2 * i + 1], px, py); if (d < A.mind[i]) A.mind[i] = d; }
        __syncthreads();
    }
    // ================= Lloyd: <= 10 iterations, stop when no centre moved more than 1 px
    for (int it = 0; it < 10; ++it) {
        for (int i = tid; i < nc; i += IN_T) {
            const float x = A.cxy[2 * i], y = A.cxy[2 * i + 1];
            float bd = dist2_f32(x, y, cen[0], cen[1]);
            int bc = 0;
#pragma unroll
            for (int c = 1; c < 8; ++c) { const float d = dist2_f32(x, y, cen[2 * c], cen[2 * c + 1]); if (d < bd) { bd = d; bc = c; } }
            A.labels[i] = bc;
        }
        __syncthreads();
        for (int c = 0; c < 8; ++c) {
            double sx = 0, sy = 0;
            int m = 0;
            for (int i = tid; i < nc; i += IN_T)
                if (A.labels[i] == c) { sx += (double)A.cxy[2 * i]; sy += (double)A.cxy[2 * i + 1]; ++m; }
            sx = block_sum_double(sx, smd);
            sy = block_sum_double(sy, smd);
            m = block_sum_int(m, smi);
            if (tid == 0) {
                cen_new[2 * c] = m ? (float)(sx / (double)m) : cen[2 * c];
                cen_new[2 * c + 1] = m ? (float)(sy / (double)m) : cen[2 * c + 1];
            }
        }
        __syncthreads();
        if (tid == 0) {
            int moved = 0;
            for (int c = 0; c < 8; ++c) {
                if (dist2_f32(cen_new[2 * c], cen_new[2 * c + 1], cen[2 * c], cen[2 * c + 1]) > 1.0f) moved = 1;
                cen[2 * c] = cen_new[2 * c]; cen[2 * c + 1] = cen_new[2 * c + 1];
            }
            s_moved = moved;
        }
        __syncthreads();
        if (!s_moved) break;
    }
    if (tid < 16) A.centres[tid] = cen[tid];
    // ================= members of every cluster in ascending compact index
    const int cchunk = (nc + IN_T - 1) / IN_T;
    const int clo = min(nc, tid * cchunk), chi = min(nc, clo + cchunk);
    int off = 0;
    for (int c = 0; c < 8; ++c) {
        int m = 0;
        for (int i = clo; i < chi; ++i) m += A.labels[i] == c;
        int tot;
        int p = off + block_excl_scan(m, smi, tot);
        for (int i = clo; i < chi; ++i)
            if (A.labels[i] == c) A.members[p++] = i;
        if (tid == 0) { A.cl_off[c] = off; if (c == 7) A.cl_off[8] = off + tot; }
        off += tot;
    }
    __syncthreads();
    // ================= picks: hypothesis h takes from cluster c the member of rank hash(seed, 8 h + c) mod |c|
    for (int j = tid; j < 8 * A.n_hyp; j += IN_T) {
        const int c = j & 7;
        const int o = A.cl_off[c], size = A.cl_off[c + 1] - o;
        const unsigned long long hsh = init_hash(A.seed, (unsigned long long)j);
        A.samples[j] = size > 0 ? A.members[o + (int)(hsh % (unsigned long long)size)] : (int)(hsh % (unsigned long long)nc);
    }
}

// One-sided (Hestenes) Jacobi in fp64 on LDS: rotates the columns of G (m x n, row-major) until they are orthogonal; V (n x n) collects the
// rotations, so G_in V = G_out and the singular values are the column norms of G_out.  Every thread of the workgroup calls it: all of
// them read the same LDS words (uniform control flow), threads [0, m) and [m, m + n) apply a rotation to one row of G / V each.
__device__ inline void jacobi_columns(double* G, int m, int n, double* V) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n * n; i += blockDim.x) V[i] = (i / n == i % n) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < 30; ++sweep) {
        int rotated = 0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                double al = 0, be = 0, ga = 0;
                for (int i = 0; i < m; ++i) { const double gp = G[i * n + p], gq = G[i * n + q]; al += gp * gp; be += gq * gq; ga += gp * gq; }
                __syncthreads();
                // (a column 1e-14 times shorter than the other would turn by less than that angle: left alone, or rounding noise never settles)
                if (ga != 0.0 && fabs(ga) > 1e-15 * sqrt(al * be) && be > 1e-28 * al && al > 1e-28 * be) {
                    rotated = 1;
                    const double zeta = (be - al) / (2.0 * ga);
                    const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                    double* row = tid < m ? G + tid * n : (tid < m + n ? V + (tid - m) * n : nullptr);
                    if (row) { const double a = row[p], b = row[q]; row[p] = cs * a - sn * b; row[q] = sn * a + cs * b; }
                }
                __syncthreads();
            }
        if (!rotated) break;
    }
}

// U diag(1, 1, 0) V^T of a 3 x 3 matrix after jacobi_columns (G V = [sigma_j u_j]): the two columns of the largest norm; k3 = the dropped one.
// Plain scalars (one thread calls it).
__device__ inline void top2_of_columns(const double* G, double* nrm, int& a, int& b, int& k3) {
    for (int j = 0; j < 3; ++j) nrm[j] = sqrt(G[j] * G[j] + G[3 + j] * G[3 + j] + G[6 + j] * G[6 + j]);
    k3 = 0;
    if (nrm[1] < nrm[k3]) k3 = 1;
    if (nrm[2] < nrm[k3]) k3 = 2;
    a = k3 == 0 ? 1 : 0;
    b = k3 == 2 ? 1 : 2;
}

// ComputeScoreAndInliers for one point (:239-244), fp32 in a fixed order; acos through double (the convention of nrs_device.hpp)
__device__ inline bool epipolar_inlier(const float* E, const float* r, const float* c, float thr) {
#pragma clang fp contract(off)
    float v[3];
    for (int i = 0; i < 3; ++i) v[i] = (E[3 * i] * r[0] + E[3 * i + 1] * r[1]) + E[3 * i + 2] * r[2];
    float nn = normf3(v);
    v[0] /= nn; v[1] /= nn; v[2] /= nn;
    nn = normf3(c);
    const float c0 = c[0] / nn, c1 = c[1] / nn, c2 = c[2] / nn;
    const float dot = (v[0] * c0 + v[1] * c1) + v[2] * c2;
    const float ac = (float)acos((double)dot);
    return fabsf(1.57079632679489661923f - ac) < thr;
}

__global__ __launch_bounds__(64) void k_init_hypotheses(InitArgs A) {
    __shared__ double G[72], V[81], G3[9], V3[9];
    __shared__ float Ef[9];
    const int lane = threadIdx.x, h = blockIdx.x;
    if (lane < 8) {
#pragma clang fp contract(off)
        const int s = A.samples[8 * h + lane];
        const float* r = A.rref + 3 * s;
        const float* c = A.rcur + 3 * s;
        for (int k = 0; k < 3; ++k)
            for (int j = 0; j < 3; ++j) G[9 * lane + 3 * k + j] = (double)(r[j] * c[k]);
    }
    __syncthreads();
    jacobi_columns(G, 8, 9, V);
    if (lane == 0) {
        int kmin = 0;
        double best = 0;
        for (int j = 0; j < 9; ++j) {
            double s = 0;
            for (int i = 0; i < 8; ++i) s += G[9 * i + j] * G[9 * i + j];
            if (j == 0 || s < best) { best = s; kmin = j; }
        }
        for (int i = 0; i < 9; ++i) G3[i] = (double)(float)V[9 * i + kmin];        // E, rows = the null vector's thirds, as fp32
    }
    __syncthreads();
    jacobi_columns(G3, 3, 3, V3);
    if (lane == 0) {
        double nrm[3];
        int a, b, k3;
        top2_of_columns(G3, nrm, a, b, k3);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const float e = (float)(-(G3[3 * i + a] / nrm[a] * V3[3 * j + a] + G3[3 * i + b] / nrm[b] * V3[3 * j + b]));
                Ef[3 * i + j] = e;
                A.hyp_E[9 * h + 3 * i + j] = e;
            }
    }
    __syncthreads();
    float E[9];
    for (int i = 0; i < 9; ++i) E[i] = Ef[i];
    int score = 0;
    for (int base = 0; base < A.n_matches; base += 64) {
        const int i = base + lane;
        const bool in = i < A.n_matches && epipolar_inlier(E, A.rref + 3 * i, A.rcur + 3 * i, A.thr);
        score += __popcll(__ballot(in));
    }
    if (lane == 0) A.hyp_score[h] = score;
}

__global__ __launch_bounds__(IN_T) void k_init_reconstruct(InitArgs A) {
    __shared__ int smi[IN_W + 1];
    __shared__ int bs[IN_W], bh[IN_W];
    __shared__ double G3[9], V3[9];
    __shared__ float sE[9], sR[9], st[3];
    __shared__ Se3f sT;
    __shared__ float s_wtc[3];
    const int tid = threadIdx.x;
    // ================= the best hypothesis: highest score, lowest h (`score > best_score`, :154)
    int sc = -1, bi = 0x7fffffff;
    for (int h = tid; h < A.n_hyp; h += IN_T) { const int s = A.hyp_score[h]; if (s > sc) { sc = s; bi = h; } }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int os = __shfl_xor(sc, off, 64), oh = __shfl_xor(bi, off, 64);
        if (os > sc || (os == sc && oh < bi)) { sc = os; bi = oh; }
    }
    if ((tid & 63) == 0) { bs[tid >> 6] = sc; bh[tid >> 6] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < IN_W; ++w)
            if (bs[w] > sc || (bs[w] == sc && bh[w] < bi)) { sc = bs[w]; bi = bh[w]; }
        A.hdr[1] = bi;
        A.hdr[2] = sc;
        for (int i = 0; i < 9; ++i) { sE[i] = A.hyp_E[9 * bi + i]; reinterpret_cast<float*>(A.hdr)[16 + i] = sE[i]; G3[i] = (double)sE[i]; }
    }
    __syncthreads();
    float E[9];
    for (int i = 0; i < 9; ++i) E[i] = sE[i];
    for (int i = tid; i < A.n_matches; i += IN_T) A.inlier[i] = epipolar_inlier(E, A.rref + 3 * i, A.rcur + 3 * i, A.thr) ? 1 : 0;
    // ================= DecomposeEssentialMatrix (:303-318) in fp64, rounded; the smaller rotation by trace
    jacobi_columns(G3, 3, 3, V3);
    if (tid == 0) {
        double nrm[3];
        int a, b, k3;
        top2_of_columns(G3, nrm, a, b, k3);
        double ua[3], ub[3], u3[3], va[3], vb[3], v3[3];
        for (int i = 0; i < 3; ++i) { ua[i] = G3[3 * i + a] / nrm[a]; ub[i] = G3[3 * i + b] / nrm[b]; va[i] = V3[3 * i + a]; vb[i] = V3[3 * i + b]; v3[i] = V3[3 * i + k3]; }
        u3[0] = ua[1] * ub[2] - ua[2] * ub[1]; u3[1] = ua[2] * ub[0] - ua[0] * ub[2]; u3[2] = ua[0] * ub[1] - ua[1] * ub[0];
        const double un = sqrt(u3[0] * u3[0] + u3[1] * u3[1] + u3[2] * u3[2]);
        for (int i = 0; i < 3; ++i) u3[i] /= un;
        double R1[9], R2[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double w = ub[i] * va[j] - ua[i] * vb[j], z = u3[i] * v3[j];
                R1[3 * i + j] = -w + z;               // U W^T V^T with U = [ua ub u3], V = [va vb v3]
                R2[3 * i + j] = w + z;                // U W V^T
            }
        auto det3 = [](const double* M) { return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]); };
        if (det3(R1) < 0) for (int i = 0; i < 9; ++i) R1[i] = -R1[i];
        if (det3(R2) < 0) for (int i = 0; i < 9; ++i) R2[i] = -R2[i];
        float R1f[9], R2f[9];
        for (int i = 0; i < 9; ++i) { R1f[i] = (float)R1[i]; R2f[i] = (float)R2[i]; }
        {
#pragma clang fp contract(off)
            const float tr1 = (R1f[0] + R1f[4]) + R1f[8], tr2 = (R2f[0] + R2f[4]) + R2f[8];
            for (int i = 0; i < 9; ++i) sR[i] = tr2 > tr1 ? R2f[i] : R1f[i];
        }
        // t = U.col(2): its sign is the SVD's in the reference; here the component of the largest magnitude (lowest index on ties) is positive
        int km = 0;
        if (fabs(u3[1]) > fabs(u3[km])) km = 1;
        if (fabs(u3[2]) > fabs(u3[km])) km = 2;
        const double sg = u3[km] < 0 ? -1.0 : 1.0;
        for (int i = 0; i < 3; ++i) st[i] = (float)(sg * u3[i]);
    }
    __syncthreads();
    // ================= the sign of t: `away` over the inlier rays (:295-298); indexed as the reference indexes them
    int away = 0;
    for (int idx = tid; idx < A.n_matches; idx += IN_T) {
        if (A.inlier[idx]) {
#pragma clang fp contract(off)
        const int kp = A.compact_indexing ? A.cmap[idx] : idx;
        float r1[3], r2[3];
        unit_ray_f32(A.cam, A.ref_xy + 2 * kp, r1);
        unit_ray_f32(A.cam, A.cur_xy + 2 * kp, r2);
        float s = 0.f;
        float d[3];
        for (int i = 0; i < 3; ++i) d[i] = (((sR[3 * i] * r1[0] + sR[3 * i + 1] * r1[1]) + sR[3 * i + 2] * r1[2]) - r2[i]) * (r2[i] - st[i]);
        s = (d[0] + d[1]) + d[2];
        away += (s > 0.f) - (s < 0.f);
        }
    }
    away = block_sum_int(away, smi);
    if (tid == 0) {
        const float sg = away < 0 ? -1.f : 1.f;
        double R[9], q[4];
        for (int i = 0; i < 9; ++i) R[i] = (double)sR[i];
        R_to_quat(R, q);
        quat_normalize(q);                                   // qw >= 0
        for (int i = 0; i < 4; ++i) sT.q[i] = (float)q[i];
        for (int i = 0; i < 3; ++i) sT.t[i] = sg * st[i];
        float* o = reinterpret_cast<float*>(A.hdr) + 25;
        for (int i = 0; i < 4; ++i) o[i] = sT.q[i];
        for (int i = 0; i < 3; ++i) o[4 + i] = sT.t[i];
        const Se3f Ti = se3_inv(sT);
        for (int i = 0; i < 3; ++i) s_wtc[i] = Ti.t[i];
    }
    __syncthreads();
    // ================= ReconstructPoints (:320-410)
    for (int i = tid; i < A.n; i += IN_T) { A.code[i] = 1; A.xyz[3 * i] = 0.f; A.xyz[3 * i + 1] = 0.f; A.xyz[3 * i + 2] = 0.f; }
    __syncthreads();
    const Se3f T = sT;
    Se3f I;
    I.q[0] = 0.f; I.q[1] = 0.f; I.q[2] = 0.f; I.q[3] = 1.f; I.t[0] = 0.f; I.t[1] = 0.f; I.t[2] = 0.f;
    int nN = 0, n_tri = 0, n_par = 0, n_d1 = 0, n_r1 = 0, n_d2 = 0, n_r2 = 0;
    for (int idx = tid; idx < A.n_matches; idx += IN_T) {
        if (A.inlier[idx]) {
#pragma clang fp contract(off)
        const int kp = A.compact_indexing ? A.cmap[idx] : idx;
        ++nN;
        float r1[3], r2[3], X[3];
        unit_ray_f32(A.cam, A.ref_xy + 2 * kp, r1);
        unit_ray_f32(A.cam, A.cur_xy + 2 * kp, r2);
        triangulate_mid_point_f32(r1, r2, I, T, X);
        const float n2[3] = {X[0] - s_wtc[0], X[1] - s_wtc[1], X[2] - s_wtc[2]};
        const float par = rays_parallax_f32(X, n2);
        int code = 0;
        float u, v, ex, ey, pc[3];
        if (par < A.rpp * 5.f) { code = 2; ++n_par; }
        else if (X[2] < 0.0f) { code = 3; ++n_d1; }
        else {
            project_f32(A.cam, X[0], X[1], X[2], u, v);
            ex = A.ref_xy[2 * kp] - u; ey = A.ref_xy[2 * kp + 1] - v;
            if ((double)(ex * ex + ey * ey) > 5.991) { code = 4; ++n_r1; }
            else {
                se3_point(T, X, pc);
                if (pc[2] < 0.0f) { code = 5; ++n_d2; }
                else {
                    project_f32(A.cam, pc[0], pc[1], pc[2], u, v);
                    ex = A.cur_xy[2 * kp] - u; ey = A.cur_xy[2 * kp + 1] - v;
                    if ((double)(ex * ex + ey * ey) > 5.991) { code = 6; ++n_r2; }
                }
            }
        }
        A.code[kp] = code;
        if (code == 0) { ++n_tri; A.xyz[3 * kp] = X[0]; A.xyz[3 * kp + 1] = X[1]; A.xyz[3 * kp + 2] = X[2]; }
        }
    }
    nN = block_sum_int(nN, smi); n_tri = block_sum_int(n_tri, smi); n_par = block_sum_int(n_par, smi); n_d1 = block_sum_int(n_d1, smi);
    n_r1 = block_sum_int(n_r1, smi); n_d2 = block_sum_int(n_d2, smi); n_r2 = block_sum_int(n_r2, smi);
    if (tid == 0) {
        int* c = A.hdr + 4;
        c[0] = nN; c[1] = n_tri; c[2] = n_par; c[3] = n_d1; c[4] = n_r1; c[5] = n_d2; c[6] = n_r2; c[7] = 0;
        int verdict = 0;
        if (n_tri < A.min_tri) verdict = 2;
        else if ((double)n_par > (double)nN * (double)A.max_low) verdict = 3;
        A.hdr[0] = verdict;
    }
}

}  // namespace nrs

using namespace nrs;

extern "C" void nrs_init_options_init(nrs_init_options* o) {
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->struct_size = (uint32_t)sizeof(*o);
    o->n_hypotheses = 0;
    o->epipolar_threshold = 0.005f;
    o->radians_per_pixel = 0.0025f;
    o->min_triangulated = 100;
    o->max_low_parallax = 0.25f;
    o->compact_indexing = 0;
    o->seed = 4;
}

extern "C" int nrs_init_essential(nrs_ctx* c, const nrs_camera* cam, const nrs_init_options* opt, int32_t n, const float* ref_xy,
                                  const float* cur_xy, const int32_t* status, int32_t n_matches, const int32_t* samples,
                                  nrs_init_result* out) {
    if (!c) return NRS_ERR_INVALID;
    if (!cam || !opt || !out || n <= 0 || n_matches < 0 || !ref_xy || !cur_xy || !status)
        return c->fail(NRS_ERR_INVALID, "nrs_init_essential: bad argument");
    if (opt->struct_size != sizeof(nrs_init_options)) return c->fail(NRS_ERR_INVALID, "nrs_init_essential: nrs_init_options.struct_size %u, expected %zu", opt->struct_size, sizeof(nrs_init_options));
    if (out->struct_size != sizeof(nrs_init_result)) return c->fail(NRS_ERR_INVALID, "nrs_init_essential: nrs_init_result.struct_size %u, expected %zu", out->struct_size, sizeof(nrs_init_result));
    if (cam->model != NRS_CAM_PINHOLE && cam->model != NRS_CAM_KB8) return c->fail(NRS_ERR_INVALID, "unknown camera model %d", cam->model);
    if (opt->n_hypotheses < 0 || opt->n_hypotheses > IN_MAXH) return c->fail(NRS_ERR_INVALID, "nrs_init_essential: n_hypotheses %d (0 or 1..%d)", opt->n_hypotheses, IN_MAXH);
    // ComputeMaxTries(0.8, 0.95) (:78-81, 130-132)
    const int n_hyp = opt->n_hypotheses ? opt->n_hypotheses : (int)(std::log(1 - 0.95f) / std::log(1 - std::pow(0.8f, 8)));
    int nc = 0;
    for (int i = 0; i < n; ++i) nc += status[i] == NRS_TRACKED;
    if (n_matches > nc) return c->fail(NRS_ERR_INVALID, "nrs_init_essential: n_matches %d exceeds the %d TRACKED keypoints", n_matches, nc);
    if (samples && n_matches >= 8)
        for (int i = 0; i < 8 * n_hyp; ++i)
            if (samples[i] < 0 || samples[i] >= nc) return c->fail(NRS_ERR_INVALID, "nrs_init_essential: sample %d of hypothesis %d out of range (%d)", i % 8, i / 8, samples[i]);
    out->verdict = 0; out->best_hypothesis = 0; out->score = 0; out->n_compact = nc; out->n_hypotheses = n_hyp;
    for (int i = 0; i < 8; ++i) out->counters[i] = 0;
    for (int i = 0; i < 9; ++i) out->E[i] = 0.f;
    for (int i = 0; i < 7; ++i) out->pose_qt[i] = i == 3 ? 1.f : 0.f;
    if (n_matches < 8) {                                  // "Not enough matches" (:51-53): nothing is computed
        out->verdict = 1;
        if (out->inlier) memset(out->inlier, 0, (size_t)n_matches);
        if (out->xyz) memset(out->xyz, 0, sizeof(float) * 3 * (size_t)n);
        if (out->code) for (int i = 0; i < n; ++i) out->code[i] = 1;
        return NRS_OK;
    }
    NRS_HIP(c, hipSetDevice(c->device));
    auto al = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t N = (size_t)n, NC = (size_t)nc, NH = (size_t)n_hyp;
    const size_t in_bytes = al(8 * N) * 2 + al(4 * N) + al(32 * NH);
    const size_t ws_bytes = al(4 * NC) + al(8 * NC) + al(12 * NC) * 2 + al(4 * NC) * 2 + al(64);
    const size_t o_hdr = 0, o_xyz = o_hdr + al(4 * IN_HDR), o_code = o_xyz + al(12 * N), o_hE = o_code + al(4 * N), o_hs = o_hE + al(36 * NH),
                 o_smp = o_hs + al(4 * NH), o_lab = o_smp + al(32 * NH), o_cen = o_lab + al(4 * NC), o_inl = o_cen + al(64), out_bytes = o_inl + al((size_t)n_matches);
    DevBuf big;                                                    // (freed when the call returns)
    NRS_TRY(c->ensure(big, in_bytes + ws_bytes + out_bytes + 256));
    char* p = big.as<char>();
    InitArgs A;
    A.cam.model = cam->model;
    for (int i = 0; i < 8; ++i) A.cam.p[i] = cam->params[i];
    A.n = n; A.n_matches = n_matches; A.n_hyp = n_hyp; A.nc = nc; A.compact_indexing = opt->compact_indexing != 0; A.have_samples = samples != nullptr;
    A.min_tri = opt->min_triangulated; A.thr = opt->epipolar_threshold; A.rpp = opt->radians_per_pixel; A.max_low = opt->max_low_parallax;
    A.seed = opt->seed;
    auto carve = [&](size_t nbytes) { char* d = p; p += al(nbytes); return d; };
    char* d_ref = carve(8 * N); char* d_cur = carve(8 * N); char* d_st = carve(4 * N);
    A.ref_xy = reinterpret_cast<float*>(d_ref); A.cur_xy = reinterpret_cast<float*>(d_cur); A.status = reinterpret_cast<int*>(d_st);
    A.cmap = reinterpret_cast<int*>(carve(4 * NC)); A.cxy = reinterpret_cast<float*>(carve(8 * NC));
    A.rref = reinterpret_cast<float*>(carve(12 * NC)); A.rcur = reinterpret_cast<float*>(carve(12 * NC));
    A.mind = reinterpret_cast<float*>(carve(4 * NC)); A.members = reinterpret_cast<int*>(carve(4 * NC)); A.cl_off = reinterpret_cast<int*>(carve(64));
    char* d_out = p;
    A.hdr = reinterpret_cast<int*>(d_out + o_hdr); A.xyz = reinterpret_cast<float*>(d_out + o_xyz); A.code = reinterpret_cast<int*>(d_out + o_code);
    A.hyp_E = reinterpret_cast<float*>(d_out + o_hE); A.hyp_score = reinterpret_cast<int*>(d_out + o_hs); A.samples = reinterpret_cast<int*>(d_out + o_smp);
    A.labels = reinterpret_cast<int*>(d_out + o_lab); A.centres = reinterpret_cast<float*>(d_out + o_cen); A.inlier = reinterpret_cast<uint8_t*>(d_out + o_inl);
    NRS_HIP(c, hipMemcpyAsync(d_ref, ref_xy, 8 * N, hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(d_cur, cur_xy, 8 * N, hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(d_st, status, 4 * N, hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemsetAsync(d_out, 0, out_bytes, c->stream));
    if (samples) NRS_HIP(c, hipMemcpyAsync(A.samples, samples, 32 * NH, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_init_prepare, dim3(1), dim3(IN_T), 0, c->stream, A);
    NRS_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(k_init_hypotheses, dim3(n_hyp), dim3(64), 0, c->stream, A);
    NRS_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(k_init_reconstruct, dim3(1), dim3(IN_T), 0, c->stream, A);
    NRS_HIP(c, hipGetLastError());
    // (the caller's arrays and this staging vector are pageable: the copies are ordered on the stream but not asynchronous to the host)
    std::vector<char> host(out_bytes);
    NRS_HIP(c, hipMemcpyAsync(host.data(), d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    const int* hdr = reinterpret_cast<const int*>(host.data() + o_hdr);
    const float* hdrf = reinterpret_cast<const float*>(hdr);
    out->verdict = hdr[0]; out->best_hypothesis = hdr[1]; out->score = hdr[2];
    for (int i = 0; i < 8; ++i) out->counters[i] = hdr[4 + i];
    for (int i = 0; i < 9; ++i) out->E[i] = hdrf[16 + i];
    for (int i = 0; i < 7; ++i) out->pose_qt[i] = hdrf[25 + i];
    if (out->xyz) memcpy(out->xyz, host.data() + o_xyz, 12 * N);
    if (out->code) memcpy(out->code, host.data() + o_code, 4 * N);
    if (out->hyp_E) memcpy(out->hyp_E, host.data() + o_hE, 36 * NH);
    if (out->hyp_score) memcpy(out->hyp_score, host.data() + o_hs, 4 * NH);
    if (out->samples_out) memcpy(out->samples_out, host.data() + o_smp, 32 * NH);
    if (out->labels && !samples) memcpy(out->labels, host.data() + o_lab, 4 * NC);
    if (out->centres && !samples) memcpy(out->centres, host.data() + o_cen, 64);
    if (out->inlier) memcpy(out->inlier, host.data() + o_inl, (size_t)n_matches);
    return NRS_OK;
}
