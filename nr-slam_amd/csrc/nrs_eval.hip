// f7: evaluation (include/nrs.h "f7: evaluation"; DESIGN.md 4 "Evaluation (f7)").
//   nrs_stereo_match_pattern      StereoPatternMatching::computeStereo3D (modules/stereo/stereo_pattern_matching.cc:33-94)
//   nrs_eval_depth_ground_truth   FrameEvaluator::ComputeGroundTruth, precomputed_depth_ branch (modules/utilities/frame_evaluator.cc:265-278)
//   nrs_stereo_from_tracks        the loop of StereoLucasKanade::ComputeStereo3D (modules/stereo/stereo_lucas_kanade.cc:50-72)
//   nrs_eval_rmse                 ComputeReconstructionRMSE and its two forms (frame_evaluator.cc:54-226)
//   nrs_eval_frame                EvaluateFrameReconstruction + SaveGroundTruthToFrame (frame_evaluator.cc:35-52, 291-305)
//
// The pattern matcher is an implicit GEMM in exact integers: M = search positions of the right image, N = keypoints, K = the 225 pixels
// of a 15 x 15 window padded to 256.  Launches of one call:
//   k_stereo_prep     per keypoint: the two boundary tests, the template (u8 for the plain form, shifted by 128 to i8 for the matrix
//                     cores, the K pad 0 AFTER the shift), its maximum, sum T and sum T^2
//   k_stereo_box      per search position: sum I and sum I^2 of its window (int32)
//   k_corr_mfma       v_mfma_i32_16x16x64_i8: a workgroup owns 64 x 32 positions and 64 keypoints; the templates sit in registers as B
//                     fragments for the whole launch, the right-image tile is staged once in LDS (shifted) and every wave builds the A
//                     fragments of 16 positions of a row from it; sum TI = sum T'I' + 128 (sum T' + sum I') + 225 * 128^2
//   k_corr_plain      NRS_STEREO_NO_MFMA=1: one lane per position, integer multiply-adds on the unshifted bytes -- the anchor of the
//                     operand lane maps
//   k_stereo_final    reduces the per-workgroup (score, position) maxima of a keypoint and writes status / match / score / xyz
// Both correlation kernels leave one (fp64 score, position) per workgroup and keypoint; "better" is a larger score, then a lower row-major
// position, which is associative and commutative -- the result does not depend on any order, and there are no atomics.
#include <climits>
#include "nrs_ctx.hpp"
#include "nrs_device.hpp"
#include "nrs_eval_host.hpp"
#include "nrs_geom_f32.hpp"

namespace nrs {
namespace {

constexpr int ST_T = 15, ST_K = 225, ST_KP = 256;        // template side, pixels, padded K
constexpr int ST_NG = 64;                                 // keypoints of a workgroup (both forms)
constexpr int MF_W = 64, MF_H = 32, MF_LS = 80;           // matrix-core form: positions of a workgroup, LDS row stride (78 bytes used)
constexpr int PL_B = 16, PL_LS = 32;                      // plain form: 16 x 16 positions, a 30 x 30 tile

typedef int v4i __attribute__((ext_vector_type(4)));

struct StereoDims { int w, h, Wr, Hr; };                  // image; result of matchTemplate (search region minus 14)

__device__ inline double ccorr_normed(int TI, int T2, int I2) {
    if (T2 == 0 || I2 == 0) return 0.0;                   // a zero norm scores 0
    return (double)TI / sqrt((double)T2 * (double)I2);    // the product is below 2^53: exact; sqrt and divide correctly rounded
}
__device__ inline bool better(double s, int p, double bs, int bp) { return s > bs || (s == bs && p < bp); }

__global__ void k_stereo_prep(const uint8_t* __restrict__ left, StereoDims D, int n, int npad, const float* __restrict__ xy,
                              int8_t* __restrict__ Tp, uint8_t* __restrict__ Tu, int* __restrict__ sumT, int* __restrict__ T2,
                              int* __restrict__ st) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    int status = NRS_EVAL_OUT_OF_BOUNDS, ox = 0, oy = 0;
    if (i < n) {
        const float x = xy[2 * i], y = xy[2 * i + 1];
        bool oob = !(x == x) || !(y == y) || x < 0.f || y < 0.f || y > (float)(D.h - 20) || x > (float)(D.w - 20);
        oob = oob || (x - 7.f) < 20.f || (y - 7.f) < 0.f || (x + 7.f) > (float)D.w || (y + 7.f) > (float)D.h;
        if (!oob) { ox = (int)(x - 7.f); oy = (int)(y - 7.f); status = NRS_EVAL_OK; }
        if (status == NRS_EVAL_OK && (ox < 0 || oy < 0 || ox + ST_T > D.w || oy + ST_T > D.h)) status = NRS_EVAL_OUT_OF_BOUNDS;   // (cannot happen: belt and braces for the reads below)
    }
    int s = 0, s2 = 0, mx = 0;
    for (int k = 0; k < ST_KP; ++k) {
        int v = 0;
        const bool real = status == NRS_EVAL_OK && k < ST_K;
        if (real) v = left[(size_t)(oy + k / ST_T) * D.w + ox + k % ST_T];
        s += v; s2 += v * v; mx = max(mx, v);
        Tu[(size_t)i * ST_KP + k] = (uint8_t)v;
        Tp[(size_t)i * ST_KP + k] = real ? (int8_t)(v - 128) : (int8_t)0;
    }
    if (status == NRS_EVAL_OK && mx > 250) status = NRS_EVAL_SATURATED;
    sumT[i] = s; T2[i] = s2; st[i] = status;
}

__global__ void k_stereo_box(const uint8_t* __restrict__ right, StereoDims D, int* __restrict__ boxI, int* __restrict__ boxI2) {
    const int px = blockIdx.x * blockDim.x + threadIdx.x, py = blockIdx.y;
    if (px >= D.Wr || py >= D.Hr) return;
    int s = 0, s2 = 0;
    for (int ky = 0; ky < ST_T; ++ky)
        for (int kx = 0; kx < ST_T; ++kx) {
            const int v = right[(size_t)(py + ky) * D.w + px + kx];
            s += v; s2 += v * v;
        }
    boxI[(size_t)py * D.Wr + px] = s;
    boxI2[(size_t)py * D.Wr + px] = s2;
}

// ---- plain form: 256 lanes = 16 x 16 positions; the 64 templates of the keypoint group in LDS; per keypoint a wave reduction
__global__ __launch_bounds__(256) void k_corr_plain(const uint8_t* __restrict__ right, StereoDims D, int npad, const uint8_t* __restrict__ Tu,
                                                    const int* __restrict__ T2, const int* __restrict__ boxI2, double* __restrict__ part_s,
                                                    int* __restrict__ part_p) {
    __shared__ uint8_t tile[30 * PL_LS];
    __shared__ uint8_t tm[ST_NG * ST_KP];
    __shared__ double red_s[ST_NG * 4];
    __shared__ int red_p[ST_NG * 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, wv = tid >> 6;
    const int x0 = blockIdx.x * PL_B, y0 = blockIdx.y * PL_B, kp0 = blockIdx.z * ST_NG;
    for (int idx = tid; idx < 30 * PL_LS; idx += 256) {
        const int r = idx / PL_LS, c = idx % PL_LS, gx = x0 + c, gy = y0 + r;
        tile[idx] = (c < 30 && gx < D.w && gy < D.h) ? right[(size_t)gy * D.w + gx] : (uint8_t)0;
    }
    for (int idx = tid; idx < ST_NG * ST_KP; idx += 256) tm[idx] = Tu[(size_t)kp0 * ST_KP + idx];
    __syncthreads();
    const int px = x0 + tx, py = y0 + ty;
    const bool valid = px < D.Wr && py < D.Hr;
    const int pos = valid ? py * D.Wr + px : INT_MAX;
    const int I2 = valid ? boxI2[pos] : 0;
    for (int j = 0; j < ST_NG; ++j) {
        int acc = 0;
        const uint8_t* t = tm + j * ST_KP;
        for (int ky = 0; ky < ST_T; ++ky)
#pragma unroll
            for (int kx = 0; kx < ST_T; ++kx) acc += (int)tile[(ty + ky) * PL_LS + tx + kx] * (int)t[ky * ST_T + kx];
        double s = valid ? ccorr_normed(acc, T2[kp0 + j], I2) : -1.0;
        int p = pos;
        for (int m = 1; m < 64; m <<= 1) {
            const double os = __shfl_xor(s, m, 64);
            const int op = __shfl_xor(p, m, 64);
            if (better(os, op, s, p)) { s = os; p = op; }
        }
        if ((tid & 63) == 0) { red_s[j * 4 + wv] = s; red_p[j * 4 + wv] = p; }
    }
    __syncthreads();
    if (tid < ST_NG) {
        double s = red_s[tid * 4];
        int p = red_p[tid * 4];
        for (int k = 1; k < 4; ++k)
            if (better(red_s[tid * 4 + k], red_p[tid * 4 + k], s, p)) { s = red_s[tid * 4 + k]; p = red_p[tid * 4 + k]; }
        const size_t o = (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * npad + kp0 + tid;
        part_s[o] = s; part_p[o] = p;
    }
}

// ---- matrix-core form.  v_mfma_i32_16x16x64_i8: A = windows (row = position lane & 15), B = templates (column = keypoint lane & 15), both
// hold the 16 k of lane group g = lane >> 4 in their 16 bytes (the same k set on both sides, so the order inside it cannot matter);
// C: column = lane & 15 (keypoint), row = 4 g + reg (position).
__global__ __launch_bounds__(256) void k_corr_mfma(const uint8_t* __restrict__ right, StereoDims D, int npad, const int8_t* __restrict__ Tp,
                                                   const int* __restrict__ sumT, const int* __restrict__ T2, const int* __restrict__ boxI,
                                                   const int* __restrict__ boxI2, double* __restrict__ part_s, int* __restrict__ part_p) {
    __shared__ uint8_t tile[(MF_H + 14) * MF_LS];
    __shared__ double red_s[16 * ST_NG];
    __shared__ int red_p[16 * ST_NG];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 15, g = lane >> 4;
    const int x0 = blockIdx.x * MF_W, y0 = blockIdx.y * MF_H, kp0 = blockIdx.z * ST_NG;
    for (int idx = tid; idx < (MF_H + 14) * MF_LS; idx += 256) {
        const int rr = idx / MF_LS, c = idx % MF_LS, gx = x0 + c, gy = y0 + rr;
        const uint8_t v = (c < MF_W + 14 && gx < D.w && gy < D.h) ? right[(size_t)gy * D.w + gx] : (uint8_t)128;
        tile[idx] = v ^ 0x80;                                  // u8 - 128 as an i8 bit pattern; outside the image: 0
    }
    v4i b[4][4];
    int sTs[4], t2[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int kp = kp0 + nt * 16 + r;
        sTs[nt] = sumT[kp] - ST_K * 128;
        t2[nt] = T2[kp];
#pragma unroll
        for (int s = 0; s < 4; ++s) b[nt][s] = *reinterpret_cast<const v4i*>(Tp + (size_t)kp * ST_KP + 64 * s + 16 * g);
    }
    int base[4], kx0[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int k0 = 64 * s + 16 * g;
        kx0[s] = k0 % ST_T;
        base[s] = (k0 / ST_T) * MF_LS + kx0[s];
    }
    double best[4];
    int bpos[4];
    float fth[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) { best[nt] = -1.0; bpos[nt] = INT_MAX; fth[nt] = -1.f; }
    __syncthreads();
    for (int ty = 0; ty < MF_H; ++ty) {
        if (y0 + ty >= D.Hr) break;                            // (uniform over the workgroup)
        const int rowbase = ty * MF_LS + wv * 16 + r;
        v4i a[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int dw = 0; dw < 4; ++dw) {
                unsigned word = 0;
#pragma unroll
                for (int bb = 0; bb < 4; ++bb) {
                    const int j = 4 * dw + bb;
                    const bool real = s < 3 || (64 * s + 16 * g + j) < ST_K;      // the K pad is 0 after the shift
                    const int off = base[s] + j + ((kx0[s] + j >= ST_T) ? MF_LS - ST_T : 0);
                    const unsigned v = real ? (unsigned)tile[rowbase + off] : 0u;
                    word |= v << (8 * bb);
                }
                a[s][dw] = (int)word;
            }
        }
        v4i acc[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            acc[nt] = v4i{0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[s], b[nt][s], acc[nt], 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int px = x0 + wv * 16 + 4 * g + reg, py = y0 + ty;
            if (px >= D.Wr) continue;
            const int pos = py * D.Wr + px;
            const int I = boxI[pos], I2 = boxI2[pos];
            const int corr = 128 * (I - ST_K * 128) + ST_K * 128 * 128;
            const float rs = I2 ? rsqrtf((float)I2) : 0.f;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int TI = acc[nt][reg] + 128 * sTs[nt] + corr;
                // cheap screen: within a keypoint the score orders as TI / sqrt(I2); a candidate more than 1e-5 (relative) below the
                // running best's fp32 value is strictly below it in fp64 too (the fp32 value is good to < 1e-6)
                const float f = (float)TI * rs;
                if (f >= fth[nt]) {
                    const double sc = ccorr_normed(TI, t2[nt], I2);
                    if (better(sc, pos, best[nt], bpos[nt])) { best[nt] = sc; bpos[nt] = pos; fth[nt] = f * (1.f - 1e-5f); }
                }
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        red_s[(wv * 4 + g) * ST_NG + nt * 16 + r] = best[nt];
        red_p[(wv * 4 + g) * ST_NG + nt * 16 + r] = bpos[nt];
    }
    __syncthreads();
    if (tid < ST_NG) {
        double s = red_s[tid];
        int p = red_p[tid];
        for (int k = 1; k < 16; ++k)
            if (better(red_s[k * ST_NG + tid], red_p[k * ST_NG + tid], s, p)) { s = red_s[k * ST_NG + tid]; p = red_p[k * ST_NG + tid]; }
        const size_t o = (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * npad + kp0 + tid;
        part_s[o] = s; part_p[o] = p;
    }
}

__global__ void k_stereo_final(StereoDims D, int n, int npad, int n_chunks, const float* __restrict__ xy, const int* __restrict__ st,
                               const double* __restrict__ part_s, const int* __restrict__ part_p, Cam cam, float bf, float* __restrict__ xyz,
                               int* __restrict__ status, double* __restrict__ score, int* __restrict__ match) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float nanf_ = __int_as_float(0x7fc00000);
    int s = st[i];
    float o[3] = {nanf_, nanf_, nanf_};
    double bs = __longlong_as_double(0x7ff8000000000000LL);
    int mx = -1, my = -1;
    if (s == NRS_EVAL_OK) {
        bs = -1.0;
        int bp = INT_MAX;
        for (int c = 0; c < n_chunks; ++c) {
            const double cs = part_s[(size_t)c * npad + i];
            const int cp = part_p[(size_t)c * npad + i];
            if (better(cs, cp, bs, bp)) { bs = cs; bp = cp; }
        }
        mx = bp % D.Wr; my = bp / D.Wr;
        if (bs < 0.99) s = NRS_EVAL_LOW_CORRELATION;
        else {
            const float x = xy[2 * i], y = xy[2 * i + 1];
            const float disp = fabsf((float)(mx + 7) - x);
            if (disp == 0.f) s = NRS_EVAL_ZERO_DISPARITY;
            else {
                const float z = bf / disp;
                const float rx = (x - cam.p[2]) / cam.p[0];
                const float ry = (y - cam.p[3]) / cam.p[1];
                o[0] = z * rx; o[1] = z * ry; o[2] = z;
            }
        }
    }
    xyz[3 * i] = o[0]; xyz[3 * i + 1] = o[1]; xyz[3 * i + 2] = o[2];
    status[i] = s; score[i] = bs; match[2 * i] = mx; match[2 * i + 1] = my;
}

// FrameEvaluator::ComputeGroundTruth, precomputed_depth_ (frame_evaluator.cc:265-278) with Interpolate (geometry_toolbox.h:47-60)
__global__ void k_depth_gt(Cam cam, const float* __restrict__ m, int w, int h, int n, const float* __restrict__ xy, float* __restrict__ gt,
                           int* __restrict__ status) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float nanf_ = __int_as_float(0x7fc00000);
    const float x = xy[2 * i], y = xy[2 * i + 1];
    float o[3] = {nanf_, nanf_, nanf_};
    int s = NRS_EVAL_OK;
    if (!(x >= 0.f) || !(y >= 0.f) || x >= (float)(w - 1) || y >= (float)(h - 1)) s = NRS_EVAL_OUT_OF_BOUNDS;
    else {
        float xi, yi;
        const float fx = modff(x, &xi), fy = modff(y, &yi);
        const float w00 = (1.f - fx) * (1.f - fy);
        const float w01 = (1.f - fx) * fy;
        const float w10 = fx * (1.f - fy);
        const float w11 = 1.f - w00 - w01 - w10;
        const int ix = (int)xi, iy = (int)yi;
        const float p00 = m[(size_t)iy * w + ix] * w00;
        const float p10 = m[(size_t)iy * w + ix + 1] * w10;
        const float p01 = m[(size_t)(iy + 1) * w + ix] * w01;
        const float p11 = m[(size_t)(iy + 1) * w + ix + 1] * w11;
        float d = p00 + p10;
        d = d + p01;
        d = d + p11;
        if (!isfinite(d)) s = NRS_EVAL_BAD_DEPTH;
        else {
            float ray[3];
            unproject_f32(cam, x, y, ray);
            const float rz = ray[2];
            o[0] = (ray[0] / rz) * d; o[1] = (ray[1] / rz) * d; o[2] = (ray[2] / rz) * d;
        }
    }
    gt[3 * i] = o[0]; gt[3 * i + 1] = o[1]; gt[3 * i + 2] = o[2];
    status[i] = s;
}

struct Carver {                                            // 256-byte aligned pieces of one allocation
    char* p;
    size_t used = 0;
    explicit Carver(char* base) : p(base) {}
    template <class T> T* take(size_t count) {
        T* r = reinterpret_cast<T*>(p + used);
        used += (count * sizeof(T) + 255) / 256 * 256;
        return r;
    }
};
inline size_t padded(size_t bytes) { return (bytes + 255) / 256 * 256; }

Cam to_cam(const nrs_camera* cam) {
    Cam c;
    c.model = cam->model;
    for (int i = 0; i < 8; ++i) c.p[i] = cam->params[i];
    return c;
}

}  // namespace
}  // namespace nrs

using namespace nrs;

// ---- the pattern matcher behind its two entry points: nrs_stereo_match_pattern (upload / download shell below) and nrs_init_stereo
// (nrs_sinit.hip), which keeps the images and the result on the device.  Both run exactly these launches.
namespace nrs {
namespace {
struct StereoPlan {
    StereoDims D;
    bool plain;
    int npad;
    dim3 grid;
    size_t n_chunks, npos;
};
StereoPlan stereo_plan(nrs_ctx* c, int w, int h, int n) {
    StereoPlan P;
    P.D.w = w; P.D.h = h;
    P.D.Wr = (w - 3) - (ST_T - 1);
    P.D.Hr = 2 * (int)((float)(h - 1) / 2.f - 2.f) - (ST_T - 1);
    P.plain = c->dbg.is_set(SW_STEREO_NO_MFMA);
    P.npad = (n + ST_NG - 1) / ST_NG * ST_NG;
    P.grid = P.plain ? dim3((P.D.Wr + PL_B - 1) / PL_B, (P.D.Hr + PL_B - 1) / PL_B, P.npad / ST_NG)
                     : dim3((P.D.Wr + MF_W - 1) / MF_W, (P.D.Hr + MF_H - 1) / MF_H, P.npad / ST_NG);
    P.n_chunks = (size_t)P.grid.x * P.grid.y;
    P.npos = (size_t)(P.D.Wr > 0 ? P.D.Wr : 0) * (size_t)(P.D.Hr > 0 ? P.D.Hr : 0);
    return P;
}
}  // namespace

int stereo_match_check(nrs_ctx* c, const char* who, const nrs_camera* cam, const uint8_t* left, const uint8_t* right, int w, int h, int stride_l,
                       int stride_r, int n, bool arrays_ok) {
    if (!cam || !left || !right || n < 0 || (n > 0 && !arrays_ok) || stride_l < w || stride_r < w) return c->fail(NRS_ERR_INVALID, "%s: bad argument", who);
    if (w < 32 || h < 32 || w > 16384 || h > 16384) return c->fail(NRS_ERR_INVALID, "%s: image %d x %d (32 .. 16384 a side)", who, w, h);
    const StereoPlan P = stereo_plan(c, w, h, 1);
    if (P.D.Wr < 1 || P.D.Hr < 1) return c->fail(NRS_ERR_INVALID, "%s: no search position in a %d x %d image", who, w, h);
    return NRS_OK;
}

size_t stereo_match_ws_bytes(nrs_ctx* c, int w, int h, int n) {
    const StereoPlan P = stereo_plan(c, w, h, n);
    return 2 * padded((size_t)P.npad * ST_KP) + 3 * padded(sizeof(int) * P.npad) + 2 * padded(sizeof(int) * P.npos) +
           padded(sizeof(double) * P.n_chunks * P.npad) + padded(sizeof(int) * P.n_chunks * P.npad);
}

int stereo_match_enqueue(nrs_ctx* c, const nrs_camera* cam, float bf, int w, int h, int n, const uint8_t* d_left, const uint8_t* d_right,
                         const float* d_xy, char* ws, float* d_xyz, int* d_status, double* d_score, int* d_match) {
    const StereoPlan P = stereo_plan(c, w, h, n);
    const StereoDims D = P.D;
    const int npad = P.npad;
    Carver cv(ws);
    int8_t* d_Tp = cv.take<int8_t>((size_t)npad * ST_KP);
    uint8_t* d_Tu = cv.take<uint8_t>((size_t)npad * ST_KP);
    int* d_sumT = cv.take<int>(npad);
    int* d_T2 = cv.take<int>(npad);
    int* d_st = cv.take<int>(npad);
    int* d_boxI = cv.take<int>(P.npos);
    int* d_boxI2 = cv.take<int>(P.npos);
    double* d_ps = cv.take<double>(P.n_chunks * npad);
    int* d_pp = cv.take<int>(P.n_chunks * npad);
    if (cv.used > stereo_match_ws_bytes(c, w, h, n)) return c->fail(NRS_ERR_STATE, "the pattern matcher's workspace accounting");
    hipLaunchKernelGGL(k_stereo_prep, dim3((npad + 63) / 64), dim3(64), 0, c->stream, d_left, D, n, npad, d_xy, d_Tp, d_Tu, d_sumT, d_T2, d_st);
    hipLaunchKernelGGL(k_stereo_box, dim3((D.Wr + 255) / 256, D.Hr), dim3(256), 0, c->stream, d_right, D, d_boxI, d_boxI2);
    if (P.plain)
        hipLaunchKernelGGL(k_corr_plain, P.grid, dim3(256), 0, c->stream, d_right, D, npad, d_Tu, d_T2, d_boxI2, d_ps, d_pp);
    else
        hipLaunchKernelGGL(k_corr_mfma, P.grid, dim3(256), 0, c->stream, d_right, D, npad, d_Tp, d_sumT, d_T2, d_boxI, d_boxI2, d_ps, d_pp);
    hipLaunchKernelGGL(k_stereo_final, dim3((n + 63) / 64), dim3(64), 0, c->stream, D, n, npad, (int)P.n_chunks, d_xy, d_st, d_ps, d_pp, to_cam(cam), bf,
                       d_xyz, d_status, d_score, d_match);
    NRS_HIP(c, hipGetLastError());
    return NRS_OK;
}
}  // namespace nrs

// The upload / download shell of the pattern matcher.  on_device: left / right are packed w x h images the device already holds (the
// resident pair of nrs_front_process_stereo) and only the keypoints go up; otherwise host images, packed while they are uploaded
static int stereo_match_shell(nrs_ctx* c, const char* who, const nrs_camera* cam, float bf, const uint8_t* left, const uint8_t* right, bool on_device,
                              int32_t w, int32_t h, int32_t stride_l, int32_t stride_r, int32_t n, const float* xy, float* xyz, int32_t* status,
                              double* score, int32_t* match_xy) {
    NRS_TRY(stereo_match_check(c, who, cam, left, right, w, h, stride_l, stride_r, n, xy && xyz && status));
    if (n == 0) return NRS_OK;
    NRS_HIP(c, hipSetDevice(c->device));
    const size_t img = on_device ? 0 : (size_t)w * h, ws_bytes = stereo_match_ws_bytes(c, w, h, n);
    const size_t bytes = 2 * padded(img) + padded(sizeof(float) * 2 * n) + ws_bytes + padded(sizeof(float) * 3 * n) + padded(sizeof(int) * n) +
                         padded(sizeof(double) * n) + padded(sizeof(int) * 2 * n);
    DevBuf big;                                                    // (freed when the call returns)
    NRS_TRY(c->ensure(big, bytes));
    Carver cv(big.as<char>());
    const uint8_t *d_left = left, *d_right = right;
    if (!on_device) {
        uint8_t* up_l = cv.take<uint8_t>(img);
        uint8_t* up_r = cv.take<uint8_t>(img);
        NRS_HIP(c, hipMemcpy2DAsync(up_l, w, left, stride_l, w, h, hipMemcpyHostToDevice, c->stream));      // packed on the device
        NRS_HIP(c, hipMemcpy2DAsync(up_r, w, right, stride_r, w, h, hipMemcpyHostToDevice, c->stream));
        d_left = up_l; d_right = up_r;
    }
    float* d_xy = cv.take<float>(2 * (size_t)n);
    char* d_ws = cv.take<char>(ws_bytes);
    float* d_xyz = cv.take<float>(3 * (size_t)n);
    int* d_status = cv.take<int>(n);
    double* d_score = cv.take<double>(n);
    int* d_match = cv.take<int>(2 * (size_t)n);
    if (cv.used > bytes) return c->fail(NRS_ERR_STATE, "%s: workspace accounting", who);
    NRS_HIP(c, hipMemcpyAsync(d_xy, xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, c->stream));
    NRS_TRY(stereo_match_enqueue(c, cam, bf, w, h, n, d_left, d_right, d_xy, d_ws, d_xyz, d_status, d_score, d_match));
    NRS_HIP(c, hipMemcpyAsync(xyz, d_xyz, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(status, d_status, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    if (score) NRS_HIP(c, hipMemcpyAsync(score, d_score, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    if (match_xy) NRS_HIP(c, hipMemcpyAsync(match_xy, d_match, sizeof(int) * 2 * n, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    return NRS_OK;
}

extern "C" int nrs_stereo_match_pattern(nrs_ctx* c, const nrs_camera* cam, float bf, const uint8_t* left, const uint8_t* right, int32_t w, int32_t h,
                                        int32_t stride_l, int32_t stride_r, int32_t n, const float* xy, float* xyz, int32_t* status,
                                        double* score, int32_t* match_xy) {
    if (!c) return NRS_ERR_INVALID;
    return stereo_match_shell(c, "nrs_stereo_match_pattern", cam, bf, left, right, false, w, h, stride_l, stride_r, n, xy, xyz, status, score, match_xy);
}

extern "C" int nrs_stereo_match_pattern_front(nrs_ctx* c, const nrs_camera* cam, float bf, int32_t w, int32_t h, int32_t image, int32_t n,
                                              const float* xy, float* xyz, int32_t* status, double* score, int32_t* match_xy) {
    if (!c) return NRS_ERR_INVALID;
    const uint8_t *left = nullptr, *right = nullptr;
    NRS_TRY(front_resident_pair(c, "nrs_stereo_match_pattern_front", w, h, image, &left, &right));
    return stereo_match_shell(c, "nrs_stereo_match_pattern_front", cam, bf, left, right, true, w, h, w, w, n, xy, xyz, status, score, match_xy);
}

extern "C" int nrs_eval_depth_ground_truth(nrs_ctx* c, const nrs_camera* cam, const float* depth, int32_t w, int32_t h, int32_t stride, int32_t n,
                                           const float* xy, float* gt_xyz, int32_t* gt_status) {
    if (!c) return NRS_ERR_INVALID;
    if (!cam || !depth || w < 2 || h < 2 || stride < w || n < 0 || (n > 0 && (!xy || !gt_xyz || !gt_status)))
        return c->fail(NRS_ERR_INVALID, "nrs_eval_depth_ground_truth: bad argument");
    if (cam->model != NRS_CAM_PINHOLE && cam->model != NRS_CAM_KB8) return c->fail(NRS_ERR_INVALID, "unknown camera model %d", cam->model);
    if (n == 0) return NRS_OK;
    NRS_HIP(c, hipSetDevice(c->device));
    const size_t img = (size_t)w * h;
    DevBuf big;                                                    // (freed when the call returns)
    NRS_TRY(c->ensure(big, padded(sizeof(float) * img) + padded(sizeof(float) * 2 * n) + padded(sizeof(float) * 3 * n) + padded(sizeof(int) * n)));
    Carver cv(big.as<char>());
    float* d_m = cv.take<float>(img);
    float* d_xy = cv.take<float>(2 * (size_t)n);
    float* d_gt = cv.take<float>(3 * (size_t)n);
    int* d_st = cv.take<int>(n);
    NRS_HIP(c, hipMemcpy2DAsync(d_m, sizeof(float) * w, depth, sizeof(float) * stride, sizeof(float) * w, h, hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(d_xy, xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_depth_gt, dim3((n + 63) / 64), dim3(64), 0, c->stream, to_cam(cam), d_m, w, h, n, d_xy, d_gt, d_st);
    NRS_HIP(c, hipGetLastError());
    NRS_HIP(c, hipMemcpyAsync(gt_xyz, d_gt, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(gt_status, d_st, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    return NRS_OK;
}

extern "C" int nrs_stereo_from_tracks(const nrs_camera* cam, float bf, int32_t n, const float* left_xy, const float* right_xy,
                                      const int32_t* track_status, float* xyz, int32_t* status) {
    return nrs_eval::stereo_from_tracks(cam, bf, n, left_xy, right_xy, track_status, xyz, status);
}

extern "C" int nrs_eval_rmse(int32_t n, const float* est_z, const float* gt_z, const uint8_t* gt_ok, int32_t align_scales, int32_t precomputed_depth,
                             float* rmse, float* scale, int32_t counts[3], uint8_t* inlier) {
    return nrs_eval::eval_rmse(n, est_z, gt_z, gt_ok, align_scales, precomputed_depth, rmse, scale, counts, inlier);
}

extern "C" int nrs_eval_frame(nrs_ctx* c, const nrs_camera* cam, const float pose_qt[7], int32_t n, const float* world_xyz, const float* xy,
                              const float* depth, int32_t w, int32_t h, int32_t stride, const float* gt_xyz, const int32_t* gt_status,
                              float* rmse, float* scale, int32_t counts[3], float* gt_world, int32_t* gt_status_out) {
    if (!cam || !pose_qt || n < 0 || !rmse || !scale || !counts || (n > 0 && (!world_xyz || !xy)) || (depth && !c) ||
        (!depth && n > 0 && (!gt_xyz || !gt_status)))
        return c ? c->fail(NRS_ERR_INVALID, "nrs_eval_frame: bad argument") : NRS_ERR_INVALID;
    std::vector<float> gt(3 * (size_t)n), est(n), gz(n);
    std::vector<int32_t> st(n);
    std::vector<uint8_t> ok(n);
    if (depth) NRS_TRY(nrs_eval_depth_ground_truth(c, cam, depth, w, h, stride, n, xy, gt.data(), st.data()));
    else { std::copy(gt_xyz, gt_xyz + 3 * (size_t)n, gt.begin()); std::copy(gt_status, gt_status + n, st.begin()); }
    const nrs_eval::Rt T = nrs_eval::se3f(pose_qt);
    for (int i = 0; i < n; ++i) {
        est[i] = nrs_eval::se3f_act_z(T, world_xyz + 3 * (size_t)i);
        gz[i] = gt[3 * (size_t)i + 2];
        ok[i] = st[i] == NRS_EVAL_OK;
    }
    if (gt_status_out) std::copy(st.begin(), st.end(), gt_status_out);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    if (gt_world) std::fill(gt_world, gt_world + 3 * (size_t)n, nan);
    const int rc = nrs_eval::eval_rmse(n, est.data(), gz.data(), ok.data(), 1, depth ? 1 : 0, rmse, scale, counts, nullptr);
    if (rc != NRS_OK) return c ? c->fail(rc, "nrs_eval_frame: %d points with ground truth, %d inliers: no RMSE", counts[0], counts[2]) : rc;
    if (gt_world) {
        const nrs_eval::Rt Ti = nrs_eval::se3f_inv(pose_qt);
        for (int i = 0; i < n; ++i) {
            if (!ok[i]) continue;
            const float p[3] = {gt[3 * (size_t)i] / *scale, gt[3 * (size_t)i + 1] / *scale, gt[3 * (size_t)i + 2] / *scale};
            nrs_eval::se3f_act(Ti, p, gt_world + 3 * (size_t)i);
        }
    }
    return NRS_OK;
}
