// a21-a23: pyramidal Lucas-Kanade tracker on MI355X
// (reference modules/matching/lucas_kanade_tracker.cc: SetReferenceImage :47-168, Track :170-596,
//  PhotometricInformation round trip :598-631; cv::buildOpticalFlowPyramid call sites :50,:184).
//
// Layout / mapping:
//   * pyramid levels live padded by winSize (21) on every side: image border = reflect-101,
//     derivative border = 0, exactly the ROI-in-a-larger-buffer OpenCV hands to the tracker, so the
//     tracker's reads at negative coordinates are plain loads.  One kernel per level computes
//     pyrDown (5-tap [1 4 6 4 1], (sum+128)>>8) straight into the padded layout, one the Scharr pair.
//   * templates are point-major: [(point*levels + level)] x {441 x i16 intensity*32, 441 x (i16,i16)
//     derivative, meanI, meanI2, valid}: one contiguous 2.6 KB run per (point, level).
//   * one wave64 per point runs the whole coarse-to-fine iteration: lanes own 7 pixels of the 21x21
//     window each (bilinear fixed-point resampling, W_BITS = 14), per-pixel terms go to LDS and lanes
//     0..4 each run one *sequential* float accumulation over the 441 terms -- the reference's sums
//     are row-major float loops (LK:377-407) and float addition does not commute, so bit-identical
//     status codes need the same order.  Exact-integer sums (window mean) use wave reductions.
//   * the fp32 arithmetic is compiled with contraction off (separate mul/add, like the oracle).
#include <type_traits>
#include <algorithm>
#include <cmath>
#include <vector>
#include "nrs_ctx.hpp"
#include "nrs_device.hpp"
#include "nrs_klt_host.hpp"
#include "nrs_reuse_host.hpp"

namespace nrs {

constexpr int KPAD = 21, KMAXL = 8;
constexpr int W_BITS = 14;

struct PyrLevel {
    uint8_t* img;      // (h + 2 pad) x (w + 2 pad)
    short2* der;       // same dims
    int w, h, stride;  // stride = w + 2 pad (elements)
};

struct Pyr {
    PyrLevel L[KMAXL];
    int n_levels;
};
static_assert(std::is_trivially_copyable_v<Pyr>, "passed to kernels by value: plain pointers, never an owner");

// What a kernel is handed of a set of templates: entry e, level l is item e * levels + l of every array (sizes: nrs_klt_host.hpp)
struct TemplateView {
    short* I; short2* D; float* mean; uint8_t* valid;
    int levels;
};
static_assert(std::is_trivially_copyable_v<TemplateView>, "passed to kernels by value: plain pointers, never an owner");

// A set of templates in HBM: the four arrays, `levels` levels an entry, room for `cap` entries, and one side array of side_bytes per
// entry -- the tracker's reference points, or the archive's "has" bytes (side_zero: they read zero wherever the set has grown)
struct TemplateSet {
    DevBuf arr[KLT_ARRAYS], side;
    int levels, cap = 0;
    size_t side_bytes;
    bool side_zero;
    const char* what;                        // names the set in an error text
    TemplateSet(int levels_, size_t side_bytes_, bool side_zero_, const char* what_) : levels(levels_), side_bytes(side_bytes_), side_zero(side_zero_), what(what_) {}
    TemplateView view() const { return TemplateView{arr[0].as<short>(), arr[1].as<short2>(), arr[2].as<float>(), arr[3].as<uint8_t>(), levels}; }
    void clear() { *this = TemplateSet(levels, side_bytes, side_zero, what); }   // holds nothing again: the old buffers are freed here
    // Room for `want` entries, the first `keep` of them carried over.  All or nothing: after a failure the set is what it was, nothing
    // new is left allocated and the context's error is set.  Waits for the stream once, behind the copies
    int reserve(nrs_ctx* c, int want, int keep) {
        if (want <= cap) return NRS_OK;
        hipError_t he = hipSetDevice(c->device);                   // (an entry point may come here without having set it)
        if (he != hipSuccess) return c->fail(NRS_ERR_HIP, "%s: hipSetDevice failed: %s", what, hipGetErrorString(he));
        TemplateSet g(levels, side_bytes, side_zero, what);
        g.cap = klt_grow_capacity(want);
        int rc = NRS_OK;
        for (int a = 0; a < KLT_ARRAYS && rc == NRS_OK; ++a) rc = c->ensure(g.arr[a], klt_entry_bytes(a, levels) * g.cap);
        if (rc == NRS_OK) rc = c->ensure(g.side, side_bytes * g.cap);
        if (rc != NRS_OK) return rc;                               // nothing of a half-made set is kept: g frees what it got
        if (side_zero) {
            he = hipMemsetAsync(g.side.p, 0, side_bytes * g.cap, c->stream);
            if (he != hipSuccess) return c->fail(NRS_ERR_HIP, "%s: clearing the grown buffers failed: %s", what, hipGetErrorString(he));
        }
        if (keep > 0) {
            const size_t m = (size_t)keep;
            for (int a = 0; a < KLT_ARRAYS && he == hipSuccess; ++a)
                he = hipMemcpyAsync(g.arr[a].p, arr[a].p, klt_entry_bytes(a, levels) * m, hipMemcpyDeviceToDevice, c->stream);
            if (he == hipSuccess) he = hipMemcpyAsync(g.side.p, side.p, side_bytes * m, hipMemcpyDeviceToDevice, c->stream);
            if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
            // (the new buffers do not outlive a failed copy; the set stays as it was)
            if (he != hipSuccess) return c->fail(NRS_ERR_HIP, "%s: copy to the grown buffers failed: %s", what, hipGetErrorString(he));
        }
        *this = std::move(g);                                      // the old buffers are freed here, the grown ones move in
        return NRS_OK;
    }
};

struct KltState {
    int win = KW, max_level = 4, max_iters = 10;
    float eps = 1e-4f, min_eig = 1e-4f;
    int n = 0;
    DevBuf pyr_buf, img_in, mask_in;
    Pyr pyr;
    int pyr_w = 0, pyr_h = 0;
    // the tracker's own templates, point-major: n of them, max_level + 1 levels a point; side array: the reference points (`prev`)
    TemplateSet tmpl{5, KLT_XY_BYTES, false, "tracker templates"};
    DevBuf pts, status, misc;
    // the archive: photometric information kept by a caller's key (the map point id) -- what the reference keeps in its Map per map
    // point (GetPhotometricInformation at keyframes, InsertPhotometricInformation when a point is reused: tracking.cc:383-391,457-460)
    // -- in HBM, so that templates never travel to the host and back (nrs_klt_archive_templates / nrs_klt_insert_archived).  Side array:
    // the "has" byte per key, for the kernels that address the archive by key (nrs_point_reuse); a_has is its host copy
    TemplateSet arch{0, KLT_HAS_BYTES, true, "template archive"};
    std::vector<uint8_t> a_has;
    // index lists of the device-to-device copies; the upload, scratch and packed result of nrs_point_reuse
    DevBuf a_idx, reuse_in, reuse_ws, reuse_out;
    float* prev() const { return tmpl.side.as<float>(); }
};

// level 0: caller image -> padded reflect-101 copy
__global__ void k_pyr_copy(const uint8_t* __restrict__ src, int sstride, PyrLevel L) {
    const int xo = blockIdx.x * blockDim.x + threadIdx.x, yo = blockIdx.y;
    if (xo >= L.stride) return;
    const int x = reflect101(xo - KPAD, L.w), y = reflect101(yo - KPAD, L.h);
    L.img[(size_t)yo * L.stride + xo] = src[(size_t)y * sstride + x];
}

// pyrDown of the previous (padded) level into the padded layout of this level
__global__ void k_pyr_down(PyrLevel P, PyrLevel L) {
    const int xo = blockIdx.x * blockDim.x + threadIdx.x, yo = blockIdx.y;
    if (xo >= L.stride) return;
    const int x = reflect101(xo - KPAD, L.w), y = reflect101(yo - KPAD, L.h);
    const int k[5] = {1, 4, 6, 4, 1};
    int acc = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint8_t* row = P.img + (size_t)(2 * y + j - 2 + KPAD) * P.stride + (2 * x - 2 + KPAD);
        acc += k[j] * (row[0] + 4 * row[1] + 6 * row[2] + 4 * row[3] + row[4]);
    }
    L.img[(size_t)yo * L.stride + xo] = (uint8_t)((acc + 128) >> 8);
}

// Scharr pair (calcSharrDeriv): reflect-101 at the image edge comes from the padded image,
// the derivative's own border is zero
__global__ void k_pyr_scharr(PyrLevel L) {
    const int xo = blockIdx.x * blockDim.x + threadIdx.x, yo = blockIdx.y;
    if (xo >= L.stride) return;
    const int x = xo - KPAD, y = yo - KPAD;
    short2 d = make_short2(0, 0);
    if (x >= 0 && x < L.w && y >= 0 && y < L.h) {
        const uint8_t* r0 = L.img + (size_t)(yo - 1) * L.stride + xo;
        const uint8_t* r1 = r0 + L.stride;
        const uint8_t* r2 = r1 + L.stride;
        int t0[3], t1[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            t0[c] = (r0[c - 1] + r2[c - 1]) * 3 + r1[c - 1] * 10;
            t1[c] = r2[c - 1] - r0[c - 1];
        }
        d.x = (short)(t0[2] - t0[0]);
        d.y = (short)((t1[2] + t1[0]) * 3 + t1[1] * 10);
    }
    L.der[(size_t)yo * L.stride + xo] = d;
}

// floor of a window origin, or false where the coordinate is not finite or its floor does not fit an int: such a position counts as
// outside the image (include/nrs.h nrs_klt_track; the reference's cvFloor gives INT_MIN there on x86 and takes its out-of-image
// branch).  Tested BEFORE the float -> int conversion, which is undefined for these values.
__device__ inline bool win_origin(float px, float py, int& ix, int& iy) {
    if (!(px >= -2147483648.f && px < 2147483648.f && py >= -2147483648.f && py < 2147483648.f)) return false;          // NaN compares false
    ix = (int)floorf(px); iy = (int)floorf(py);
    return true;
}

__device__ inline int cv_round(float v) { return __float2int_rn(v); }          // round half to even

__device__ inline void bilinear_weights(float a, float b, int& w00, int& w01, int& w10, int& w11) {
#pragma clang fp contract(off)
    w00 = cv_round((1.f - a) * (1.f - b) * (float)(1 << W_BITS));
    w01 = cv_round(a * (1.f - b) * (float)(1 << W_BITS));
    w10 = cv_round((1.f - a) * b * (float)(1 << W_BITS));
    w11 = (1 << W_BITS) - w00 - w01 - w10;
}

__device__ inline int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

__device__ inline void sample_px(const PyrLevel& L, int ix, int iy, int px, int w00, int w01, int w10, int w11,
                                 int& val, int& dx, int& dy, bool with_deriv) {
    const int y = px / KW, x = px - y * KW;
    const size_t o = (size_t)(iy + y + KPAD) * L.stride + (ix + x + KPAD);
    const uint8_t* s = L.img + o;
    val = descale(s[0] * w00 + s[1] * w01 + s[L.stride] * w10 + s[L.stride + 1] * w11, W_BITS - 5);
    if (with_deriv) {
        const short2 a = L.der[o], b = L.der[o + 1], c = L.der[o + L.stride], d = L.der[o + L.stride + 1];
        dx = descale(a.x * w00 + b.x * w01 + c.x * w10 + d.x * w11, W_BITS);
        dy = descale(a.y * w00 + b.y * w01 + c.y * w10 + d.y * w11, W_BITS);
    }
}

__device__ inline float seq_sum_441(const float* v) {          // row-major sequential accumulation
#pragma clang fp contract(off)
    float s = 0.f;
    for (int i = 0; i < KA; ++i) s += v[i];
    return s;
}

// ---------------------------------------------------------------------------------------------
// a21: SetReferenceImage, one wave per (point, level)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_klt_set_reference(Pyr pyr, int n, TemplateView t, const float* __restrict__ pts,
                                                           const uint8_t* __restrict__ mask, int mw, int mh) {
#pragma clang fp contract(off)
    __shared__ float s_v[KA], s_v2[KA];
    const int lane = threadIdx.x;
    const int i = blockIdx.x / t.levels, level = blockIdx.x % t.levels;
    const size_t slot = (size_t)i * t.levels + level;
    if (lane == 0) { t.valid[slot] = 0; t.mean[2 * slot] = -1.f; t.mean[2 * slot + 1] = -1.f; }
    if (level >= pyr.n_levels) return;
    const PyrLevel L = pyr.L[level];
    const float half = (KW - 1) * 0.5f;
    const float px = pts[2 * i] / (float)(1 << level) - half, py = pts[2 * i + 1] / (float)(1 << level) - half;
    int ix, iy;
    const int gap = KW / 2;                                      // round(winSize.width/2), LK:58
    if (!win_origin(px, py, ix, iy) || ix < -gap || ix >= L.w - gap || iy < -gap || iy >= L.h - gap) return;
    int w00, w01, w10, w11;
    bilinear_weights(px - (float)ix, py - (float)iy, w00, w01, w10, w11);
    bool masked = false;
    for (int p = lane; p < KA; p += 64) {
        int val, dx, dy;
        sample_px(L, ix, iy, p, w00, w01, w10, w11, val, dx, dy, true);
        t.I[slot * KA + p] = (short)val;
        t.D[slot * KA + p] = make_short2((short)dx, (short)dy);
        s_v[p] = (float)val;
        s_v2[p] = (float)(val * val);
        if (mask) {                                              // LK:125-131 (out-of-image reads: not masked)
            const int y = p / KW, x = p - y * KW;
            const int mx = (ix + x) << level, my = (iy + y) << level;
            if (mx >= 0 && mx < mw && my >= 0 && my < mh && mask[(size_t)my * mw + mx] == 0) masked = true;
        }
    }
    __syncthreads();
    if (__any(masked)) return;
    float r = 0.f;
    if (lane == 0) r = seq_sum_441(s_v);
    if (lane == 1) r = seq_sum_441(s_v2);
    const float FLT_SCALE = 1.f / (1 << 20);
    if (lane < 2) t.mean[2 * slot + lane] = (r * FLT_SCALE) / (float)KA;
    if (lane == 0) t.valid[slot] = 1;
}

// ---------------------------------------------------------------------------------------------
// a22: Track (coarse-to-fine iterations), one wave per point
// ---------------------------------------------------------------------------------------------
struct TrackArgs {
    Pyr pyr;
    int n, max_level, max_iters;
    float eps, min_eig;
    int initial_flow;
    const float* prev;
    float* pts;            // in/out
    int* status;           // in/out
    TemplateView t;        // read only
};
static_assert(std::is_trivially_copyable_v<TrackArgs>, "passed to kernels by value: plain pointers, never an owner");

__device__ inline bool usable(int s) { return s == NRS_TRACKED_WITH_3D || s == NRS_TRACKED || s == NRS_JUST_TRIANGULATED; }

// Where point i's templates are: SlotOwn = the tracker's own slots, point-major (slot i, `levels` levels a point); SlotKeyed = the archive
// entry under key[i], read in place (nrs_point_reuse: `levels` is then the archive's level count).  A key nothing was archived under --
// beyond the archive, or its "has" byte zero -- is a template that was never filled at any level.
struct SlotOwn {
    __device__ size_t base(int i, int levels) const { return (size_t)i * levels; }
    __device__ bool has(int) const { return true; }
};
struct SlotKeyed {
    const int* key; const uint8_t* a_has; int a_cap;
    __device__ size_t base(int i, int levels) const { return (size_t)key[i] * levels; }
    __device__ bool has(int i) const { const int k = key[i]; return k >= 0 && k < a_cap && a_has[k] != 0; }
};

template <class Slot>
__device__ inline void klt_track_point(const TrackArgs& a, const Slot sl) {
#pragma clang fp contract(off)
    __shared__ float s_t[5][KA];          // per-pixel terms of b1, b2, A11, A22, A12
    __shared__ float s_j2[KA];
    __shared__ short s_I[KA];
    __shared__ short2 s_D[KA];
    const int lane = threadIdx.x, i = blockIdx.x;
    int st = a.status[i];
    if (!usable(st)) return;
    const float half = (KW - 1) * 0.5f;
    const int gap = KW / 2 + 1;                                   // LK:186
    const float FLT_SCALE = 1.f / (1 << 20);
    float ptx = a.pts[2 * i], pty = a.pts[2 * i + 1];
    const float rx = a.prev[2 * i], ry = a.prev[2 * i + 1];
    // the top level is the highest one the tracked image's pyramid has (a short pyramid: min(w, h) <= 21 * 2^max_level); the initial
    // guess is scaled there (include/nrs.h nrs_klt_track)
    const int top = min(a.max_level, a.pyr.n_levels - 1);
    for (int level = top; level >= 0; --level) {
        if (!usable(st)) break;
        const PyrLevel L = a.pyr.L[level];
        const float inv = (float)(1. / (1 << level));
        float pvx = rx * inv, pvy = ry * inv;
        float nx, ny;
        if (level == top) {
            if (a.initial_flow) { nx = ptx * inv; ny = pty * inv; }
            else { nx = pvx; ny = pvy; }
        } else { nx = ptx * 2.f; ny = pty * 2.f; }
        ptx = nx; pty = ny;
        pvx -= half; pvy -= half;
        int ipx, ipy;
        if (!win_origin(pvx, pvy, ipx, ipy) || ipx < -gap || ipx >= L.w - gap || ipy < -gap || ipy >= L.h - gap) {
            if (level == 0) st = NRS_OUT_IMAGE_BOUNDARIES;
            continue;
        }
        const size_t slot = sl.base(i, a.t.levels) + level;
        if (!sl.has(i) || !a.t.valid[slot]) {
            if (level == 0) st = NRS_OUT_IMAGE_BOUNDARIES;
            continue;
        }
        const float meanI = a.t.mean[2 * slot], meanI2 = a.t.mean[2 * slot + 1];
        __syncthreads();
        for (int p = lane; p < KA; p += 64) { s_I[p] = a.t.I[slot * KA + p]; s_D[p] = a.t.D[slot * KA + p]; }
        const float sx0 = nx, sy0 = ny;                           // startCoordinates
        nx -= half; ny -= half;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < a.max_iters; ++j) {
            int ix, iy;
            if (!win_origin(nx, ny, ix, iy) || ix < -gap || ix >= L.w - gap || iy < -gap || iy >= L.h - gap) {
                if (level == 0) st = NRS_OUT_IMAGE_BOUNDARIES;
                break;
            }
            int w00, w01, w10, w11;
            bilinear_weights(nx - (float)ix, ny - (float)iy, w00, w01, w10, w11);
            int jv[7], jx[7], jy[7];
            int sum = 0;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                const int p = lane + 64 * q;
                jv[q] = jx[q] = jy[q] = 0;
                if (p < KA) {
                    sample_px(L, ix, iy, p, w00, w01, w10, w11, jv[q], jx[q], jy[q], true);
                    sum += jv[q];
                    s_j2[p] = (float)(jv[q] * jv[q]);
                }
            }
            // window mean: every partial sum is an integer < 2^24, so the float loop of the
            // reference (LK:343) is exact and equals this integer reduction
            for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
            __syncthreads();
            float m2 = 0.f;
            if (lane == 0) m2 = seq_sum_441(s_j2);
            m2 = __shfl(m2, 0, 64);
            const float meanJ = ((float)sum * FLT_SCALE) / (float)KA;
            const float meanJ2 = (m2 * FLT_SCALE) / (float)KA;
            const float alpha = sqrtf(meanI2 / meanJ2);
            const float beta = meanI - alpha * meanJ;
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                const int p = lane + 64 * q;
                if (p < KA) {
                    const int diff = (int)((float)jv[q] * alpha - (float)s_I[p] - beta);    // truncation, LK:392
                    const float dx = (float)s_D[p].x + (float)jx[q] * alpha;
                    const float dy = (float)s_D[p].y + (float)jy[q] * alpha;
                    const float fd = (float)diff;
                    s_t[0][p] = fd * dx; s_t[1][p] = fd * dy;
                    s_t[2][p] = dx * dx; s_t[3][p] = dy * dy; s_t[4][p] = dx * dy;
                }
            }
            __syncthreads();
            float acc = 0.f;
            if (lane < 5) acc = seq_sum_441(s_t[lane]);
            const float b1 = __shfl(acc, 0, 64) * FLT_SCALE, b2 = __shfl(acc, 1, 64) * FLT_SCALE;
            const float A11 = __shfl(acc, 2, 64) * FLT_SCALE, A22 = __shfl(acc, 3, 64) * FLT_SCALE;
            const float A12 = __shfl(acc, 4, 64) * FLT_SCALE;
            float D = A11 * A22 - A12 * A12;
            const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * KW * KW);
            if (minEig < a.min_eig || D < 1.1920929e-07f) {
                // reference `continue`s: nothing changed, every remaining iteration repeats this outcome
                if (level == 0) st = NRS_BAD_FEATURE;
                break;
            }
            D = 1.f / D;
            const float dlx = (A12 * b2 - A22 * b1) * D, dly = (A12 * b1 - A11 * b2) * D;
            nx += dlx; ny += dly;
            ptx = nx + half; pty = ny + half;
            if (ptx < gap + 1 || ptx >= L.w - 1 - gap || pty < gap + 1 || pty >= L.h - 1 - gap) {
                if (level == 0) st = NRS_OUT_IMAGE_BOUNDARIES;
                break;
            }
            const double ddx = (double)(ptx - sx0), ddy = (double)(pty - sy0);
            if (sqrt(ddx * ddx + ddy * ddy) > 10) {
                ptx = sx0; pty = sy0;
                if (level == 0) st = NRS_BAD;
                break;
            }
            if ((double)dlx * (double)dlx + (double)dly * (double)dly <= (double)a.eps) break;
            if (j > 0 && fabs((double)(dlx + pdx)) < 0.01 && fabs((double)(dly + pdy)) < 0.01) {
                ptx -= dlx * 0.5f; pty -= dly * 0.5f;
                break;
            }
            pdx = dlx; pdy = dly;
        }
    }
    if (lane == 0) { a.pts[2 * i] = ptx; a.pts[2 * i + 1] = pty; a.status[i] = st; }
}

__global__ __launch_bounds__(64) void k_klt_track(TrackArgs a) { klt_track_point(a, SlotOwn()); }
__global__ __launch_bounds__(64) void k_klt_track_keyed(TrackArgs a, SlotKeyed sl) { klt_track_point(a, sl); }

// ---------------------------------------------------------------------------------------------
// SSIM gate at level 0 (LK:465-592), one wave per point
// ---------------------------------------------------------------------------------------------
__device__ inline int div32_rne(int v) {                         // saturate_cast<short>(v / 32.0), v >= 0
    int q = v >> 5;
    const int r = v & 31;
    if (r > 16 || (r == 16 && (q & 1))) ++q;
    return q;
}

template <class Slot>
__device__ inline void klt_ssim_point(const Pyr& pyr, const TemplateView& t, float* pts, int* status, float min_ssim, float* ssim_out,
                                      int* n_good, const Slot sl) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, i = blockIdx.x;
    int st = status[i];
    if (!usable(st)) return;
    const PyrLevel L = pyr.L[0];
    const float half = (KW - 1) * 0.5f;
    const int gap = KW / 2 + 1;
    const float ptx = pts[2 * i], pty = pts[2 * i + 1];
    const float nx = ptx - half, ny = pty - half;
    int ix, iy;
    if (!win_origin(nx, ny, ix, iy) || ix < -gap || ix >= L.w - gap * 2 || iy < -gap || iy >= L.h - gap * 2) {
        if (lane == 0) status[i] = NRS_OUT_IMAGE_BOUNDARIES;
        return;
    }
    int w00, w01, w10, w11;
    bilinear_weights(nx - (float)ix, ny - (float)iy, w00, w01, w10, w11);
    const size_t slot = sl.base(i, t.levels);
    int cur[7], ref[7], sc = 0, sr = 0;
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        const int p = lane + 64 * q;
        cur[q] = ref[q] = 0;
        if (p < KA) {
            int val, dx, dy;
            sample_px(L, ix, iy, p, w00, w01, w10, w11, val, dx, dy, false);
            cur[q] = min(255, max(0, div32_rne(val)));
            const int rv = t.I[slot * KA + p];
            ref[q] = rv >= 0 ? div32_rne(rv) : -div32_rne(-rv);
            sc += cur[q]; sr += ref[q];
        }
    }
    for (int off = 32; off > 0; off >>= 1) { sc += __shfl_xor(sc, off, 64); sr += __shfl_xor(sr, off, 64); }
    const float N_inv = 1.f / (float)KA, N_inv_1 = 1.f / (float)(KA - 1);
    const float mu_x = (float)sr * N_inv, mu_y = (float)sc * N_inv;
    double xx = 0, yy = 0, xy = 0;
#pragma unroll
    for (int q = 0; q < 7; ++q) {
        const int p = lane + 64 * q;
        if (p < KA) {
            const double xn = (double)((float)ref[q] - mu_x), yn = (double)((float)cur[q] - mu_y);
            xx += xn * xn; yy += yn * yn; xy += xn * yn;
        }
    }
    xx = wave_sum(xx); yy = wave_sum(yy); xy = wave_sum(xy);
    const float sx = sqrtf((float)(xx * (double)N_inv_1)), sy = sqrtf((float)(yy * (double)N_inv_1));
    const float sxy = (float)(xy * (double)N_inv_1);
    const float C1 = (float)((0.01 * 255) * (0.01 * 255)), C2 = (float)((0.03 * 255) * (0.03 * 255));
    const float ssim = ((2.f * mu_x * mu_y + C1) * (2.f * sxy + C2)) /
                       ((mu_x * mu_x + mu_y * mu_y + C1) * (sx * sx + sy * sy + C2));
    if (lane == 0) {
        if (ssim_out) ssim_out[i] = ssim;
        if (ssim < min_ssim) status[i] = NRS_BAD_FEATURE;
        else atomicAdd(n_good, 1);
    }
}

__global__ __launch_bounds__(64) void k_klt_ssim(Pyr pyr, int n, TemplateView t, float* pts, int* status, float min_ssim, float* ssim_out,
                                                  int* n_good) {
    klt_ssim_point(pyr, t, pts, status, min_ssim, ssim_out, n_good, SlotOwn());
}
// (a point that reaches the gate is still usable, so the track kernel found its key's entry: the gate reads no entry that is not there)
__global__ __launch_bounds__(64) void k_klt_ssim_keyed(Pyr pyr, TemplateView t, float* pts, int* status, float min_ssim, int* n_good, SlotKeyed sl) {
    klt_ssim_point(pyr, t, pts, status, min_ssim, nullptr, n_good, sl);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static KltState* klt(nrs_ctx* c) {
    if (!c->klt) c->klt = new (std::nothrow) KltState();
    return c->klt;
}

void klt_free(nrs_ctx* c) {
    delete c->klt;
    c->klt = nullptr;
}

// img: the caller's host image (uploaded into img_in), or -- on_device -- an image the context already holds (nrs_front_process)
static int build_pyramid(nrs_ctx* c, KltState* k, const uint8_t* img, int w, int h, int stride, bool on_device = false) {
    // level sizes (buildOpticalFlowPyramid stops when the next level would not exceed winSize)
    int ws[KMAXL], hs[KMAXL], nl = 1;
    ws[0] = w; hs[0] = h;
    for (int l = 1; l <= k->max_level; ++l) {
        const int nw = (ws[l - 1] + 1) / 2, nh = (hs[l - 1] + 1) / 2;
        if (nw <= KW || nh <= KW) break;
        ws[l] = nw; hs[l] = nh;
        nl = l + 1;
    }
    size_t bytes = 0, off[KMAXL][2];
    for (int l = 0; l < nl; ++l) {
        const size_t px = (size_t)(ws[l] + 2 * KPAD) * (hs[l] + 2 * KPAD);
        off[l][0] = bytes; bytes += (px + 255) / 256 * 256;
        off[l][1] = bytes; bytes += (px * sizeof(short2) + 255) / 256 * 256;
    }
    NRS_TRY(c->ensure(k->pyr_buf, bytes));
    if (!on_device) NRS_TRY(c->ensure(k->img_in, (size_t)stride * h));
    for (int l = 0; l < nl; ++l) {
        PyrLevel& L = k->pyr.L[l];
        L.w = ws[l]; L.h = hs[l]; L.stride = ws[l] + 2 * KPAD;
        L.img = k->pyr_buf.as<uint8_t>() + off[l][0];
        L.der = reinterpret_cast<short2*>(k->pyr_buf.as<char>() + off[l][1]);
    }
    k->pyr.n_levels = nl;
    if (!on_device) NRS_HIP(c, hipMemcpyAsync(k->img_in.p, img, (size_t)stride * h, hipMemcpyHostToDevice, c->stream));
    const uint8_t* d_img = on_device ? img : k->img_in.as<uint8_t>();
    for (int l = 0; l < nl; ++l) {
        const PyrLevel& L = k->pyr.L[l];
        const dim3 b(256), g((L.stride + 255) / 256, L.h + 2 * KPAD);
        if (l == 0) hipLaunchKernelGGL(k_pyr_copy, g, b, 0, c->stream, d_img, stride, L);
        else hipLaunchKernelGGL(k_pyr_down, g, b, 0, c->stream, k->pyr.L[l - 1], L);
        hipLaunchKernelGGL(k_pyr_scharr, g, b, 0, c->stream, L);
    }
    NRS_HIP(c, hipGetLastError());
    return NRS_OK;
}

}  // namespace nrs

using namespace nrs;

extern "C" int nrs_klt_configure(nrs_ctx* c, const nrs_klt_config* cfg) {
    if (!c || !cfg) return NRS_ERR_INVALID;
    if (cfg->win_size != KW) return c->fail(NRS_ERR_INVALID, "only the reference's 21x21 window is supported (SLAM/system.cc:78)");
    if (cfg->max_level < 0 || cfg->max_level >= KMAXL || cfg->max_iters <= 0) return c->fail(NRS_ERR_INVALID, "bad KLT configuration");
    KltState* k = klt(c);
    if (!k) return c->fail(NRS_ERR_ALLOC, "out of host memory");
    if (k->n > 0 && cfg->max_level != k->max_level) return c->fail(NRS_ERR_STATE, "cannot change max_level while templates are stored (call nrs_klt_clear)");
    if (cfg->max_level + 1 != k->tmpl.levels && k->tmpl.cap > 0) {
        // the template buffers are sized cap x levels: another level count invalidates them (k->n == 0 here)
        NRS_HIP(c, hipStreamSynchronize(c->stream));
        k->tmpl.clear();
    }
    k->max_level = cfg->max_level; k->tmpl.levels = cfg->max_level + 1;          // max_level + 1 slots per point
    k->max_iters = cfg->max_iters; k->eps = cfg->epsilon; k->min_eig = cfg->min_eig_threshold;
    return NRS_OK;
}

extern "C" int nrs_klt_clear(nrs_ctx* c) {
    if (!c) return NRS_ERR_INVALID;
    if (c->klt) c->klt->n = 0;
    return NRS_OK;
}

extern "C" int nrs_klt_num_points(nrs_ctx* c) { return (c && c->klt) ? c->klt->n : 0; }

// SetReferenceImage on a host image / mask (uploaded) or on the resident ones of the front end (on_device)
static int klt_set_reference_impl(nrs_ctx* c, const uint8_t* img, int32_t w, int32_t h, int32_t stride, const uint8_t* mask, bool on_device,
                                  int32_t n, const float* xy) {
    NRS_HIP(c, hipSetDevice(c->device));
    KltState* k = klt(c);
    if (!k) return c->fail(NRS_ERR_ALLOC, "out of host memory");
    NRS_TRY(build_pyramid(c, k, img, w, h, stride, on_device));
    k->n = 0;
    NRS_TRY(k->tmpl.reserve(c, n, 0));
    k->n = n;
    if (n == 0) return NRS_OK;
    NRS_HIP(c, hipMemcpyAsync(k->prev(), xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, c->stream));
    const uint8_t* dmask = nullptr;
    if (mask && on_device) dmask = mask;
    else if (mask) {
        NRS_TRY(c->ensure(k->mask_in, (size_t)w * h));
        NRS_HIP(c, hipMemcpyAsync(k->mask_in.p, mask, (size_t)w * h, hipMemcpyHostToDevice, c->stream));
        dmask = k->mask_in.as<uint8_t>();
    }
    hipLaunchKernelGGL(k_klt_set_reference, dim3(n * k->tmpl.levels), dim3(64), 0, c->stream, k->pyr, n, k->tmpl.view(), k->prev(), dmask, w, h);
    NRS_HIP(c, hipGetLastError());
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    return NRS_OK;
}

extern "C" int nrs_klt_set_reference(nrs_ctx* c, const uint8_t* img, int32_t w, int32_t h, int32_t stride,
                                     const uint8_t* mask, int32_t n, const float* xy) {
    if (!c) return NRS_ERR_INVALID;
    if (!img || w <= KW || h <= KW || stride < w || n < 0 || (n > 0 && !xy)) return c->fail(NRS_ERR_INVALID, "nrs_klt_set_reference: bad argument");
    return klt_set_reference_impl(c, img, w, h, stride, mask, false, n, xy);
}

extern "C" int nrs_klt_set_reference_front(nrs_ctx* c, int32_t w, int32_t h, int32_t image, int32_t use_global_mask, int32_t n, const float* xy) {
    if (!c) return NRS_ERR_INVALID;
    const uint8_t *img = nullptr, *mask = nullptr;
    NRS_TRY(front_resident(c, "nrs_klt_set_reference_front", w, h, image, use_global_mask, &img, &mask));
    if (w <= KW || h <= KW || n < 0 || (n > 0 && !xy)) return c->fail(NRS_ERR_INVALID, "nrs_klt_set_reference_front: bad argument");
    return klt_set_reference_impl(c, img, w, h, w, mask, true, n, xy);
}

// Track on a host image (uploaded) or on a resident one of the front end (on_device)
static int klt_track_impl(nrs_ctx* c, const uint8_t* img, int32_t w, int32_t h, int32_t stride, bool on_device, int32_t n,
                          float* xy, int32_t* status, int32_t use_initial_flow, float min_ssim, int32_t* n_good, float* ssim) {
    KltState* k = c->klt;
    if (!k) return c->fail(NRS_ERR_STATE, "nrs_klt_track before nrs_klt_set_reference");
    if (!img || w <= KW || h <= KW || stride < w || n != k->n || (n > 0 && (!xy || !status)))
        return c->fail(NRS_ERR_INVALID, "nrs_klt_track: bad argument (n must equal the number of stored templates: %d)", k->n);
    NRS_HIP(c, hipSetDevice(c->device));
    NRS_TRY(build_pyramid(c, k, img, w, h, stride, on_device));
    if (n_good) *n_good = 0;
    if (n == 0) return NRS_OK;
    NRS_TRY(c->ensure(k->pts, sizeof(float) * 2 * n));
    NRS_TRY(c->ensure(k->status, sizeof(int) * n));
    NRS_TRY(c->ensure(k->misc, sizeof(int) * 4 + sizeof(float) * n));
    NRS_HIP(c, hipMemcpyAsync(k->pts.p, xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(k->status.p, status, sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemsetAsync(k->misc.p, 0, sizeof(int) * 4, c->stream));
    TrackArgs a;
    a.pyr = k->pyr; a.n = n; a.max_level = k->max_level; a.max_iters = k->max_iters;
    a.eps = k->eps; a.min_eig = k->min_eig; a.initial_flow = use_initial_flow ? 1 : 0;
    a.prev = k->prev(); a.pts = k->pts.as<float>(); a.status = k->status.as<int>();
    a.t = k->tmpl.view();
    hipLaunchKernelGGL(k_klt_track, dim3(n), dim3(64), 0, c->stream, a);
    float* d_ssim = reinterpret_cast<float*>(k->misc.as<char>() + sizeof(int) * 4);
    hipLaunchKernelGGL(k_klt_ssim, dim3(n), dim3(64), 0, c->stream, k->pyr, n, a.t, a.pts, a.status, min_ssim, ssim ? d_ssim : nullptr, k->misc.as<int>());
    NRS_HIP(c, hipGetLastError());
    int good = 0;
    NRS_HIP(c, hipMemcpyAsync(xy, k->pts.p, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(status, k->status.p, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipMemcpyAsync(&good, k->misc.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (ssim) NRS_HIP(c, hipMemcpyAsync(ssim, d_ssim, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    if (n_good) *n_good = good;
    return NRS_OK;
}

extern "C" int nrs_klt_track(nrs_ctx* c, const uint8_t* img, int32_t w, int32_t h, int32_t stride, int32_t n,
                             float* xy, int32_t* status, int32_t use_initial_flow, float min_ssim, int32_t* n_good,
                             float* ssim) {
    if (!c) return NRS_ERR_INVALID;
    return klt_track_impl(c, img, w, h, stride, false, n, xy, status, use_initial_flow, min_ssim, n_good, ssim);
}

extern "C" int nrs_klt_track_front(nrs_ctx* c, int32_t w, int32_t h, int32_t image, int32_t n, float* xy, int32_t* status,
                                   int32_t use_initial_flow, float min_ssim, int32_t* n_good, float* ssim) {
    if (!c) return NRS_ERR_INVALID;
    const uint8_t *img = nullptr, *mask = nullptr;
    NRS_TRY(front_resident(c, "nrs_klt_track_front", w, h, image, 0, &img, &mask));
    return klt_track_impl(c, img, w, h, w, true, n, xy, status, use_initial_flow, min_ssim, n_good, ssim);
}

// StereoLucasKanade::ComputeStereo3D (stereo_lucas_kanade.cc:38-75) on the resident pair of cf, in the tracker state of c (c == cf: its
// tracking templates are replaced).  cf's images were complete when nrs_front_process_stereo returned (it synchronises cf's stream), and every
// launch here is waited for on c's stream before the call returns, so nothing reads them afterwards.
extern "C" int nrs_stereo_match_lk_front(nrs_ctx* c, nrs_ctx* cf, const nrs_camera* cam, float bf, int32_t w, int32_t h, int32_t image, int32_t n,
                                         const float* xy, float min_ssim, float* xyz, int32_t* status, float* right_xy, int32_t* track_status) {
    if (!c || !cf) return c ? c->fail(NRS_ERR_INVALID, "nrs_stereo_match_lk_front: no front-end context") : NRS_ERR_INVALID;
    if (c->device != cf->device) return c->fail(NRS_ERR_INVALID, "nrs_stereo_match_lk_front: the two contexts are on different devices");
    const uint8_t *left = nullptr, *right = nullptr;
    const int rc = front_resident_pair(cf, "nrs_stereo_match_lk_front", w, h, image, &left, &right);
    if (rc != NRS_OK) return c == cf ? rc : c->fail(rc, "%s", cf->err);
    if (!cam || w <= KW || h <= KW || n < 0 || (n > 0 && (!xy || !xyz || !status || !right_xy || !track_status)))
        return c->fail(NRS_ERR_INVALID, "nrs_stereo_match_lk_front: bad argument");
    NRS_TRY(klt_set_reference_impl(c, left, w, h, w, nullptr, true, n, xy));                       // SetReferenceImage(left, keypoints), no mask
    for (int i = 0; i < n; ++i) { right_xy[2 * i] = xy[2 * i]; right_xy[2 * i + 1] = xy[2 * i + 1]; track_status[i] = NRS_TRACKED; }
    NRS_TRY(klt_track_impl(c, right, w, h, w, true, n, right_xy, track_status, 1, min_ssim, nullptr, nullptr));   // Track(right), seeded at the keypoints
    return nrs_stereo_from_tracks(cam, bf, n, xy, right_xy, track_status, xyz, status);
}

// `count` templates from slot `first` on, between the tracker's set and the caller's arrays (to_device: into the set).  host: the reference
// points, then the four arrays in the set's order; the callers have checked them and the range
static int klt_transfer(nrs_ctx* c, const TemplateSet& t, int first, int count, bool to_device, void* const host[1 + KLT_ARRAYS]) {
    for (int a = -1; a < KLT_ARRAYS; ++a) {
        const size_t per = a < 0 ? t.side_bytes : klt_entry_bytes(a, t.levels);
        char* dev = (a < 0 ? t.side : t.arr[a]).as<char>() + per * (size_t)first;
        if (to_device) NRS_HIP(c, hipMemcpy(dev, host[a + 1], per * (size_t)count, hipMemcpyHostToDevice));
        else NRS_HIP(c, hipMemcpy(host[a + 1], dev, per * (size_t)count, hipMemcpyDeviceToHost));
    }
    return NRS_OK;
}

// ... appended behind the stored ones (the set grows as needed)
static int klt_append(nrs_ctx* c, int count, const float* xy, const int16_t* gray, const int16_t* grad, const float* mean, const uint8_t* valid) {
    KltState* k = klt(c);
    if (!k) return c->fail(NRS_ERR_ALLOC, "out of host memory");
    NRS_TRY(k->tmpl.reserve(c, k->n + count, k->n));
    void* const host[] = {const_cast<float*>(xy), const_cast<int16_t*>(gray), const_cast<int16_t*>(grad), const_cast<float*>(mean), const_cast<uint8_t*>(valid)};
    NRS_TRY(klt_transfer(c, k->tmpl, k->n, count, true, host));
    k->n += count;
    return NRS_OK;
}

extern "C" int nrs_klt_get_template(nrs_ctx* c, int32_t idx, float xy[2], int16_t* gray, int16_t* grad, float* mean,
                                    uint8_t* valid) {
    if (!c) return NRS_ERR_INVALID;
    KltState* k = c->klt;
    if (!k || idx < 0 || idx >= k->n) return c->fail(NRS_ERR_INVALID, "template index out of range");
    if (!xy || !gray || !grad || !mean || !valid) return c->fail(NRS_ERR_INVALID, "null output");
    void* const host[] = {xy, gray, grad, mean, valid};
    return klt_transfer(c, k->tmpl, idx, 1, false, host);
}

extern "C" int nrs_klt_insert_template(nrs_ctx* c, const float xy[2], const int16_t* gray, const int16_t* grad,
                                       const float* mean, const uint8_t* valid) {
    if (!c) return NRS_ERR_INVALID;
    if (!xy || !gray || !grad || !mean || !valid) return c->fail(NRS_ERR_INVALID, "null input");
    return klt_append(c, 1, xy, gray, grad, mean, valid);
}

extern "C" int nrs_klt_get_templates(nrs_ctx* c, int32_t first, int32_t count, float* xy, int16_t* gray, int16_t* grad,
                                     float* mean, uint8_t* valid) {
    if (!c) return NRS_ERR_INVALID;
    KltState* k = c->klt;
    if (!k || first < 0 || count < 0 || first + count > k->n) return c->fail(NRS_ERR_INVALID, "template range out of bounds");
    if (count == 0) return NRS_OK;
    if (!xy || !gray || !grad || !mean || !valid) return c->fail(NRS_ERR_INVALID, "null output");
    void* const host[] = {xy, gray, grad, mean, valid};
    return klt_transfer(c, k->tmpl, first, count, false, host);
}

extern "C" int nrs_klt_insert_templates(nrs_ctx* c, int32_t count, const float* xy, const int16_t* gray,
                                        const int16_t* grad, const float* mean, const uint8_t* valid) {
    if (!c) return NRS_ERR_INVALID;
    if (count < 0) return c->fail(NRS_ERR_INVALID, "count < 0");
    if (count == 0) return NRS_OK;
    if (!xy || !gray || !grad || !mean || !valid) return c->fail(NRS_ERR_INVALID, "null input");
    return klt_append(c, count, xy, gray, grad, mean, valid);
}

// ---- the template archive (device to device) ----------------------------------------------------------------------------------
// `lv` levels of entry se of s into entry de of d, by one workgroup of 256 threads.  (The source arrays pass through __restrict__
// parameters: a view's members cannot carry the promise, and without it the loops' loads are not batched ahead of the stores.)
__device__ inline void copy_levels(const short* __restrict__ sI, const short2* __restrict__ sD, const float* __restrict__ sM, const uint8_t* __restrict__ sV,
                                   size_t so, const TemplateView& d, size_t d_o, int lv) {
    for (int e = threadIdx.x; e < lv * KA; e += 256) { d.I[d_o * KA + e] = sI[so * KA + e]; d.D[d_o * KA + e] = sD[so * KA + e]; }
    for (int e = threadIdx.x; e < 2 * lv; e += 256) d.mean[2 * d_o + e] = sM[2 * so + e];
    for (int e = threadIdx.x; e < lv; e += 256) d.valid[d_o + e] = sV[so + e];
}
__device__ inline void copy_template(const TemplateView& s, int se, const TemplateView& d, int de, int lv) {
    copy_levels(s.I, s.D, s.mean, s.valid, (size_t)se * s.levels, d, (size_t)de * d.levels, lv);
}

// one workgroup per template: `lv` levels of entry src_idx[i] of s into entry dst_idx[i] of d; d_has (nullable): the destination's
// per-entry "has" byte, set
__global__ __launch_bounds__(256) void k_klt_copy_templates(int n, const int* __restrict__ src_idx, const int* __restrict__ dst_idx, int lv, TemplateView s,
                                                            TemplateView d, uint8_t* d_has) {
    const int i = blockIdx.x;
    if (i >= n) return;
    if (d_has && threadIdx.x == 0) d_has[dst_idx[i]] = 1;
    copy_template(s, src_idx[i], d, dst_idx[i], lv);
}

extern "C" int nrs_klt_archive_templates(nrs_ctx* c, int32_t n, const int32_t* slots, const int32_t* keys) {
    if (!c) return NRS_ERR_INVALID;
    KltState* k = c->klt;
    char msg[256];
    int kmax;
    const int bad = klt_archive_check(n, slots, keys, k != nullptr, k ? k->n : 0, &kmax, msg, sizeof msg);
    if (bad) return c->fail(bad == -2 ? NRS_ERR_STATE : NRS_ERR_INVALID, "%s", msg);
    if (n == 0) return NRS_OK;
    NRS_HIP(c, hipSetDevice(c->device));
    if (k->arch.levels != k->tmpl.levels && k->arch.cap > 0) {     // (another level count: the archive starts over)
        NRS_HIP(c, hipStreamSynchronize(c->stream));
        k->arch.clear();
        k->a_has.clear();
    }
    k->arch.levels = k->tmpl.levels;
    NRS_TRY(k->arch.reserve(c, kmax + 1, k->arch.cap));
    k->a_has.resize((size_t)k->arch.cap, 0);
    std::vector<int> u_slot, u_key;
    klt_archive_last_stands(n, slots, keys, kmax, u_slot, u_key);
    const int m = (int)u_key.size();
    NRS_TRY(c->ensure(k->a_idx, sizeof(int) * 2 * (size_t)m));
    int* d_idx = k->a_idx.as<int>();
    NRS_HIP(c, hipMemcpyAsync(d_idx, u_slot.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(d_idx + m, u_key.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_klt_copy_templates, dim3(m), dim3(256), 0, c->stream, m, d_idx, d_idx + m, k->tmpl.levels, k->tmpl.view(), k->arch.view(),
                       k->arch.side.as<uint8_t>());
    NRS_HIP(c, hipGetLastError());
    NRS_HIP(c, hipStreamSynchronize(c->stream));                   // (the caller's index arrays are free again; the archive is complete for any stream)
    for (int i = 0; i < n; ++i) k->a_has[keys[i]] = 1;
    return NRS_OK;
}

extern "C" int nrs_klt_insert_archived(nrs_ctx* c, nrs_ctx* src, int32_t n, const int32_t* keys, const float* xy) {
    if (!c || !src) return NRS_ERR_INVALID;
    if (n < 0 || (n > 0 && (!keys || !xy))) return c->fail(NRS_ERR_INVALID, "nrs_klt_insert_archived: bad argument");
    if (n == 0) return NRS_OK;
    if (c->device != src->device) return c->fail(NRS_ERR_INVALID, "nrs_klt_insert_archived: the two contexts are on different devices");
    KltState* ks = src->klt;
    if (!ks || ks->arch.cap == 0) return c->fail(NRS_ERR_STATE, "nrs_klt_insert_archived: the source context holds no archive");
    KltState* k = klt(c);
    if (!k) return c->fail(NRS_ERR_ALLOC, "out of host memory");
    if (k->tmpl.levels > ks->arch.levels)
        return c->fail(NRS_ERR_INVALID, "nrs_klt_insert_archived: the archive holds %d levels, this tracker needs %d", ks->arch.levels, k->tmpl.levels);
    for (int i = 0; i < n; ++i)
        if (keys[i] < 0 || keys[i] >= ks->arch.cap || !ks->a_has[keys[i]]) return c->fail(NRS_ERR_INVALID, "nrs_klt_insert_archived: nothing archived under key %d", keys[i]);
    NRS_HIP(c, hipSetDevice(c->device));
    NRS_TRY(k->tmpl.reserve(c, k->n + n, k->n));
    NRS_TRY(c->ensure(k->a_idx, sizeof(int) * 2 * (size_t)n));
    std::vector<int> dst((size_t)n);
    for (int i = 0; i < n; ++i) dst[i] = k->n + i;
    int* d_idx = k->a_idx.as<int>();
    NRS_HIP(c, hipMemcpyAsync(d_idx, keys, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(d_idx + n, dst.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(k->prev() + 2 * (size_t)k->n, xy, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_klt_copy_templates, dim3(n), dim3(256), 0, c->stream, n, d_idx, d_idx + n, k->tmpl.levels, ks->arch.view(), k->tmpl.view(),
                       (uint8_t*)nullptr);
    NRS_HIP(c, hipGetLastError());
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    k->n += n;
    return NRS_OK;
}


// ---- PointReuse in one call (tracking.cc:394-506; include/nrs.h nrs_point_reuse) -------------------------------------------------
// Four launches on the pyramid this context's last Track / SetReferenceImage built: candidates (project, flag, compact), the two-level
// tracker and its SSIM gate on the archive entries read in place by key, the 5.99 gate with the packed result and the ordered list
// of new slots, and the device-to-device append of those slots.  The compactions are stable (candidate order is ascending map index):
// ONE workgroup walks its list in chunks of REUSE_BLOCK and carries the running count, so no second launch and no wait between
// workgroups is needed -- a map holds thousands of points, a handful of chunks.
namespace nrs {

constexpr int REUSE_BLOCK = 1024;

struct ReuseIn {
    Cam cam;
    float R[9], t[3];
    int w, h, n_map;
    const float* map_pos; const int* frame_slot; const int* slot_status; const uint8_t* lost;
};

struct ReusePacked { unsigned cand, seed, xy, status, accepted; };          // word offsets of ReuseLayout

// rank of this thread's flag among the workgroup's set flags (thread order) and their total: wave ballots + one LDS row of wave counts
__device__ inline int block_rank(bool flag, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                                               // (the row's previous use is over)
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int off = 0;
    total = 0;
    for (int k = 0; k < REUSE_BLOCK / 64; ++k) { const int cnt = s_wave[k]; if (k < wv) off += cnt; total += cnt; }
    return off + before;
}

// stages 1 + 2: pc = R X + t in the frame loop's float32 form, uv = project_f32(pc), the flags, and the stable compaction.  A candidate
// leaves with its map index, its seed (reference point AND initial guess) and status TRACKED_WITH_3D.  hdr: n_cand, 0, 0, 0 (n_good)
__global__ __launch_bounds__(REUSE_BLOCK) void k_reuse_candidates(ReuseIn a, int* hdr, int* cand_id, float* seed, float* xy, int* status) {
#pragma clang fp contract(off)
    __shared__ int s_wave[REUSE_BLOCK / 64];
    int base = 0;
    for (int c0 = 0; c0 < a.n_map; c0 += REUSE_BLOCK) {
        const int i = c0 + (int)threadIdx.x;
        bool cand = false;
        float u = 0.f, v = 0.f;
        if (i < a.n_map) {
            const float X0 = a.map_pos[3 * i], X1 = a.map_pos[3 * i + 1], X2 = a.map_pos[3 * i + 2];
            const float pcx = ((a.R[0] * X0 + a.R[1] * X1) + a.R[2] * X2) + a.t[0];
            const float pcy = ((a.R[3] * X0 + a.R[4] * X1) + a.R[5] * X2) + a.t[1];
            const float pcz = ((a.R[6] * X0 + a.R[7] * X1) + a.R[8] * X2) + a.t[2];
            project_f32(a.cam, pcx, pcy, pcz, u, v);
            const bool inside = u >= 0.f && u < (float)a.w && v >= 0.f && v < (float)a.h;          // (NaN compares false)
            const int sl = a.frame_slot[i];
            bool present = false;
            if (sl >= 0) { const int s = a.slot_status[sl]; present = s == NRS_TRACKED_WITH_3D || s == NRS_JUST_TRIANGULATED; }
            cand = (a.lost[i] != 0 || (!present && pcz >= 0.f)) && inside;      // lost points are not tested for z (tracking.cc:397-414)
        }
        int total;
        const int r = block_rank(cand, s_wave, total);
        if (cand) {
            const int o = base + r;
            cand_id[o] = i;
            seed[2 * o] = u; seed[2 * o + 1] = v;
            xy[2 * o] = u; xy[2 * o + 1] = v;
            status[o] = NRS_TRACKED_WITH_3D;
        }
        base += total;
    }
    if (threadIdx.x == 0) { hdr[0] = base; hdr[1] = 0; hdr[2] = 0; hdr[3] = 0; }
}

// stages 4 + 5: accepted = still TRACKED_WITH_3D and within sqrt(5.99) px of the seed; the packed result; with insert_new the accepted
// candidates the frame holds no slot for, in candidate order: their keys, and their xy as the reference points of slots n0, n0 + 1, ...
__global__ __launch_bounds__(REUSE_BLOCK) void k_reuse_gate(int n_cand, const int* __restrict__ cand_id, const float* __restrict__ seed,
                                                             const float* __restrict__ xy, const int* __restrict__ status,
                                                             const int* __restrict__ frame_slot, int insert_new, int n0, float* prev, int* new_key,
                                                             int* out, ReusePacked P) {
#pragma clang fp contract(off)
    __shared__ int s_wave[REUSE_BLOCK / 64];
    int n_acc = 0, n_new = 0;
    for (int c0 = 0; c0 < n_cand; c0 += REUSE_BLOCK) {
        const int i = c0 + (int)threadIdx.x;
        bool acc = false, nw = false;
        int key = 0;
        float x = 0.f, y = 0.f;
        if (i < n_cand) {
            key = cand_id[i];
            x = xy[2 * i]; y = xy[2 * i + 1];
            const float sx = seed[2 * i], sy = seed[2 * i + 1];
            const float ex = sx - x, ey = sy - y;
            const int st = status[i];
            acc = st == NRS_TRACKED_WITH_3D && !(ex * ex + ey * ey > 5.99f);
            nw = insert_new && acc && frame_slot[key] < 0;
            out[P.cand + i] = key;
            out[P.status + i] = st;
            out[P.accepted + i] = acc ? 1 : 0;
            float* of = reinterpret_cast<float*>(out);
            of[P.seed + 2 * i] = sx; of[P.seed + 2 * i + 1] = sy;
            of[P.xy + 2 * i] = x; of[P.xy + 2 * i + 1] = y;
        }
        int tot_a, tot_n;
        block_rank(acc, s_wave, tot_a);
        const int r = block_rank(nw, s_wave, tot_n);
        if (nw) {
            const int o = n_new + r;
            new_key[o] = key;
            prev[2 * (size_t)(n0 + o)] = x; prev[2 * (size_t)(n0 + o) + 1] = y;
        }
        n_acc += tot_a; n_new += tot_n;
    }
    if (threadIdx.x == 0) { out[0] = n_cand; out[1] = n_acc; out[2] = n_new; out[3] = 0; }
}

// stage 6: archive entry new_key[i] -> tracker slot n0 + i, `lv` levels (what nrs_klt_insert_archived copies); one workgroup per
// candidate is launched, the ones at or beyond n_new (out[2]) leave
__global__ __launch_bounds__(256) void k_reuse_append(const int* __restrict__ out, const int* __restrict__ new_key, int n0, int lv, TemplateView s, TemplateView d) {
    const int i = blockIdx.x;
    if (i >= out[2]) return;
    copy_template(s, new_key[i], d, n0 + i, lv);
}

}  // namespace nrs

extern "C" int nrs_point_reuse(nrs_ctx* c, const nrs_camera* cam, const float pose_qt[7], int32_t w, int32_t h, int32_t n_map, const float* map_pos,
                               const int32_t* frame_slot, int32_t n_slots, const int32_t* slot_status, int32_t n_lost, const int32_t* lost_ids,
                               float min_ssim, int32_t insert_new, int32_t* n_cand, int32_t* cand_id, float* seed_xy, float* xy, int32_t* status,
                               int32_t* accepted, int32_t* n_reused, int32_t* n_new) {
    if (!c) return NRS_ERR_INVALID;
    const ReuseArgs ra{cam, cam ? cam->model : 0, pose_qt, w, h, n_map, map_pos, frame_slot, n_slots, slot_status, n_lost, lost_ids,
                       {n_cand, cand_id, seed_xy, xy, status, accepted, n_reused, n_new}};
    char msg[256];
    if (reuse_check_args(ra, msg, sizeof msg) != 0) return c->fail(NRS_ERR_INVALID, "%s", msg);
    KltState* k = c->klt;
    if (!k || k->pyr.n_levels <= 0 || !k->pyr_buf.p)
        return c->fail(NRS_ERR_STATE, "nrs_point_reuse: no pyramid has been built (it tracks on the image of the last nrs_klt_track[_front] / nrs_klt_set_reference[_front])");
    if (w != k->pyr.L[0].w || h != k->pyr.L[0].h)
        return c->fail(NRS_ERR_STATE, "nrs_point_reuse: %d x %d is not the size of the pyramid this context holds (%d x %d)", w, h, k->pyr.L[0].w, k->pyr.L[0].h);
    if (k->arch.cap > 0 && k->arch.levels < 2)
        return c->fail(NRS_ERR_INVALID, "nrs_point_reuse: the archive holds %d level(s), PointReuse's tracker needs 2", k->arch.levels);
    if (insert_new && k->arch.cap > 0 && k->tmpl.levels > k->arch.levels)
        return c->fail(NRS_ERR_INVALID, "nrs_point_reuse: the archive holds %d levels, this tracker needs %d", k->arch.levels, k->tmpl.levels);
    *n_cand = 0; *n_reused = 0; *n_new = 0;
    if (n_map == 0) return NRS_OK;
    NRS_HIP(c, hipSetDevice(c->device));
    const ReuseUpload U((size_t)n_map, (size_t)n_slots);
    const ReuseScratch S((size_t)n_map);
    std::vector<char> up(U.bytes);
    reuse_pack_upload(ra, up.data());
    NRS_TRY(c->ensure(k->reuse_in, U.bytes));
    NRS_TRY(c->ensure(k->reuse_ws, sizeof(int) * S.words));
    NRS_HIP(c, hipMemcpyAsync(k->reuse_in.p, up.data(), U.bytes, hipMemcpyHostToDevice, c->stream));
    char* d_in = k->reuse_in.as<char>();
    int* ws = k->reuse_ws.as<int>();
    ReuseIn in;
    in.cam.model = cam->model;
    for (int i = 0; i < 8; ++i) in.cam.p[i] = cam->params[i];
    reuse_rotation(pose_qt, in.R);
    for (int i = 0; i < 3; ++i) in.t[i] = pose_qt[4 + i];
    in.w = w; in.h = h; in.n_map = n_map;
    in.map_pos = reinterpret_cast<const float*>(d_in + U.pos); in.frame_slot = reinterpret_cast<const int*>(d_in + U.slot);
    in.slot_status = reinterpret_cast<const int*>(d_in + U.status); in.lost = reinterpret_cast<const uint8_t*>(d_in + U.lost);
    int* d_cand = ws + S.cand;
    float *d_seed = reinterpret_cast<float*>(ws + S.seed), *d_xy = reinterpret_cast<float*>(ws + S.xy);
    int *d_status = ws + S.status, *d_new_key = ws + S.new_key;
    hipLaunchKernelGGL(k_reuse_candidates, dim3(1), dim3(REUSE_BLOCK), 0, c->stream, in, ws, d_cand, d_seed, d_xy, d_status);
    NRS_HIP(c, hipGetLastError());
    int n = 0;
    NRS_HIP(c, hipMemcpyAsync(&n, ws, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));                   // the one wait before the last: n_cand sizes the launches below
    if (n < 0 || n > n_map) return c->fail(NRS_ERR_HIP, "nrs_point_reuse: the candidate count came back as %d (map of %d)", n, n_map);
    if (n == 0) return NRS_OK;                                     // (the tracker is untouched)
    const int n0 = k->n;
    if (insert_new) NRS_TRY(k->tmpl.reserve(c, n0 + n, n0));   // (room for every candidate; the buffers grow in amortised steps)
    const ReuseLayout L((size_t)n);
    NRS_TRY(c->ensure(k->reuse_out, sizeof(int) * L.words));
    int* d_out = k->reuse_out.as<int>();
    TrackArgs a;
    a.pyr = k->pyr; a.n = n; a.max_level = 1; a.max_iters = k->max_iters;
    a.eps = k->eps; a.min_eig = k->min_eig; a.initial_flow = 1;
    a.prev = d_seed; a.pts = d_xy; a.status = d_status;
    a.t = k->arch.view();
    const SlotKeyed sl{d_cand, k->arch.side.as<uint8_t>(), k->arch.cap};
    hipLaunchKernelGGL(k_klt_track_keyed, dim3(n), dim3(64), 0, c->stream, a, sl);
    hipLaunchKernelGGL(k_klt_ssim_keyed, dim3(n), dim3(64), 0, c->stream, k->pyr, a.t, d_xy, d_status, min_ssim, ws + 3, sl);
    const ReusePacked P{(unsigned)L.cand, (unsigned)L.seed, (unsigned)L.xy, (unsigned)L.status, (unsigned)L.accepted};
    hipLaunchKernelGGL(k_reuse_gate, dim3(1), dim3(REUSE_BLOCK), 0, c->stream, n, d_cand, d_seed, d_xy, d_status, in.frame_slot, insert_new ? 1 : 0, n0,
                       k->prev(), d_new_key, d_out, P);
    if (insert_new)
        hipLaunchKernelGGL(k_reuse_append, dim3(n), dim3(256), 0, c->stream, d_out, d_new_key, n0, k->tmpl.levels, a.t, k->tmpl.view());
    NRS_HIP(c, hipGetLastError());
    std::vector<int32_t> packed(L.words);
    NRS_HIP(c, hipMemcpyAsync(packed.data(), d_out, sizeof(int) * L.words, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    const ReuseOut out{n_cand, cand_id, seed_xy, xy, status, accepted, n_reused, n_new};
    if (reuse_unpack(packed.data(), n, out) != 0) {
        *n_cand = 0; *n_reused = 0; *n_new = 0;
        return c->fail(NRS_ERR_HIP, "nrs_point_reuse: the packed result's header (%d, %d, %d) contradicts the candidate count %d", packed[0], packed[1], packed[2], n);
    }
    k->n = n0 + *n_new;
    return NRS_OK;
}
