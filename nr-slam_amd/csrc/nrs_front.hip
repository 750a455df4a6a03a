// f5: the image front end -- what System::TrackImage does to a frame before the tracker is entered
// (reference modules/SLAM/system.cc:113-201): cvtColor(RGB2GRAY), CLAHE(3.0, 8x8) and Masker::GetAllMasks
// (modules/masking/masker.cc:94-115 with bright_filter.cc:24-39, border_filter.cc:24-39, predefined_filter.cc:27-39).
//
// One upload per frame; grey, CLAHE and the Global mask stay in the context for nrs_klt_*_front / nrs_shi_extract_front.
// The arithmetic is DEFINED in DESIGN.md "f5" (OpenCV's conventions for the integer steps, the project's own definition of the
// Gaussian) and restated on the CPU in tests/front_oracle.py; the kernels are held to that file byte for byte.
//
//   k_front_gray           8-bit fixed point (R*9798 + G*19235 + B*3735 + 2^14) >> 15, channel 0 = R
//   k_front_clahe_lut      one workgroup per tile: LDS histogram (integer atomics), clip, redistribution, scan, LUT
//   k_front_clahe_apply    bilinear blend of the four neighbouring LUTs, fp32, contraction off
//   k_front_*_pair         the three above over a stereo pair in one launch each, the eye in grid.z (nrs_front_process_stereo)
//   k_front_rect_map       stereo rectification (reference modules/datasets/hamlyn.cc:194-198): both eyes' undistort-rectify maps, once
//                          per configuration, fp64; stored as fp32 and as the fixed-point taps the remap reads
//   k_front_rect_gray_pair hamlyn.cc:226-229 + grey: the raw pair remapped (8-bit INTER_LINEAR, BORDER_CONSTANT 0) and converted in one
//                          launch (nrs_front_process_stereo_raw); DESIGN.md 4 "Stereo rectification", held to tests/rect_oracle.py
//   k_front_resize_gray    the resize of the Endomapper app (reference apps/endomapper.cc:65-69, cv::resize INTER_LINEAR) + grey: the raw frame
//                          resized (2 x 2 box when exactly halved, else 11-bit fixed-point taps) and converted in one launch
//                          (nrs_front_process_raw); DESIGN.md 4 "Frame resize", held to tests/resize_oracle.py
//   k_front_erode_ellipse  union of the element's row spans over a tile staged in LDS (the threshold of BrightFilter is
//                          applied while the tile is loaded)
//   k_front_rowmin/colmin  the rectangles, separably; the row pass reads its source through a functor: a plain image, the
//                          BorderFilter's ROI-and-non-zero image, or the AND of all filter masks (the Global mask)
//   k_front_gauss_h/v      11 taps each, float accumulators in tap order, one rounding at the end
// Pixels outside the image never take part in a minimum (OpenCV's default border value of erode).
#include <algorithm>
#include <cmath>
#include <new>
#include <utility>
#include <vector>
#include "nrs_ctx.hpp"
#include "nrs_device.hpp"
#include "nrs_rect_host.hpp"
#include "nrs_resize_host.hpp"

namespace nrs {

constexpr int FRONT_KMAX = 21;                 // largest structuring element (BorderFilter's 21x21)
constexpr int FRONT_TX = 32, FRONT_TY = 8;     // output tile of the ellipse erosion

struct EllSpans { int k; signed char lo[FRONT_KMAX], hi[FRONT_KMAX]; };     // element row i holds columns lo[i] <= j < hi[i]
struct GaussW { float w[11]; };
struct PlainSrc { const uint8_t* p; };
struct BorderSrc { const uint8_t* gray; int x0, y0, x1, y1; };              // ROI [x0, x1) x [y0, y1)
struct AndSrc { const uint8_t* p[NRS_FRONT_MAX_FILTERS]; int n; };

struct FrontFilter {
    int kind = 0;
    int p[5] = {0, 0, 0, 0, 0};
    int mw = 0, mh = 0;                        // PREDEFINED: size of the caller's mask
};

// Stereo rectification: the maps of nrs_front_rectify_configure.  They belong to the context, not to a filter configuration:
// nrs_front_configure carries them over into the state it builds
struct RectState {
    bool on = false;                           // maps have been built
    int sw = 0, sh = 0, dw = 0, dh = 0;        // raw and rectified size of an eye
    DevBuf taps;                               // [eye][dh x dw] fixed-point taps, 8 bytes each: what the remap reads
    DevBuf maps;                               // [eye][x | y][dh x dw] floats: what nrs_front_rectify_maps hands out
    DevBuf colour, colour_r;                   // the rectified eyes, dw x dh x channels (a rect_*_out pointer, or NRS_RECT_OWN_LAUNCH)
};

// Frame resize: the tap tables of nrs_front_resize_configure.  Like the maps they belong to the context, not to a filter configuration
struct ResizeState {
    bool on = false;                           // tables have been built
    bool box = false;                          // exactly halved: the 2 x 2 box branch (the tables are built all the same)
    int sw = 0, sh = 0, dw = 0, dh = 0;        // raw and resized size of a frame
    DevBuf tabs;                               // sx [dw] | sy [dh][2] (int32), then ax [dw][2] | by [dh][2] (int16): what nrs_front_resize_taps hands out
    DevBuf colour;                             // the resized frame, dw x dh x channels (resized_out, or NRS_RESIZE_OWN_LAUNCH)
};

struct FrontState {
    std::vector<FrontFilter> filters;
    float clip = 3.f;
    int tiles_x = 8, tiles_y = 8;
    int w = 0, h = 0;
    bool valid = false;                        // a frame has been processed under this configuration
    bool valid_right = false;                  // ... and it was a stereo pair: the right eye's grey and CLAHE are resident too
    DevBuf raw, gray, clahe, global, tmp_a, tmp_f, lut, at;
    DevBuf raw_r, gray_r, clahe_r, lut_r;      // the right eye of nrs_front_process_stereo (its 64 LUTs; it has no masks)
    DevBuf fmask[NRS_FRONT_MAX_FILTERS];       // BRIGHT / BORDER: the last frame's mask; PREDEFINED: the eroded mask (made once)
    EllSpans e11, e20;
    GaussW gw;
    RectState rect;
    ResizeState resize;
};

// ---- the three stages both eyes take: one body each, entered by the single-frame kernel and by the pair kernel -----------------------
__device__ inline void front_gray_px(const uint8_t* __restrict__ src, int stride, int ch, int w, uint8_t* __restrict__ dst) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const uint8_t* s = src + (size_t)y * stride + (size_t)x * ch;
    int v = s[0];
    if (ch > 1) v = (s[0] * 9798 + s[1] * 19235 + s[2] * 3735 + (1 << 14)) >> 15;
    dst[(size_t)y * w + x] = (uint8_t)v;
}

__device__ inline uint8_t front_sat_rint(float v) {
    const int i = __float2int_rn(v);           // round half to even
    return (uint8_t)min(255, max(0, i));
}

// CLAHE, one workgroup of 256 per tile, grid.x x grid.y = tiles_x x tiles_y; the tile is cut from the image extended to
// (tw tiles_x) x (th tiles_y) by reflect-101
__device__ inline void front_clahe_lut_tile(const uint8_t* __restrict__ gray, int w, int h, int tw, int th, int clip, uint8_t* __restrict__ lut) {
#pragma clang fp contract(off)
    __shared__ int hist[256];
    __shared__ int s_excess;
    const int tid = threadIdx.x;
    hist[tid] = 0;
    if (tid == 0) s_excess = 0;
    __syncthreads();
    const int area = tw * th;
    for (int i = tid; i < area; i += 256) {
        const int ly = i / tw, lx = i - ly * tw;
        const int gx = reflect101(blockIdx.x * tw + lx, w), gy = reflect101(blockIdx.y * th + ly, h);
        atomicAdd(&hist[gray[(size_t)gy * w + gx]], 1);
    }
    __syncthreads();
    int v = hist[tid];
    if (v > clip) { atomicAdd(&s_excess, v - clip); v = clip; }
    __syncthreads();
    const int excess = s_excess, batch = excess / 256;
    int residual = excess - batch * 256;
    v += batch;
    if (residual > 0) {                        // one more for bins 0, step, 2 step, ... until the residual is used up
        const int step = max(256 / residual, 1);
        if (tid % step == 0 && tid / step < residual) v += 1;
    }
    hist[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {  // inclusive scan (integers: any order)
        const int t = tid >= off ? hist[tid - off] : 0;
        __syncthreads();
        hist[tid] += t;
        __syncthreads();
    }
    const float scale = 255.f / (float)area;
    lut[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + tid] = front_sat_rint((float)hist[tid] * scale);
}

__device__ inline void front_clahe_blend_px(const uint8_t* __restrict__ gray, int w, int h, int tw, int th, int tiles_x, int tiles_y,
                                            const uint8_t* __restrict__ lut, uint8_t* __restrict__ dst) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const float inv_tw = 1.f / (float)tw, inv_th = 1.f / (float)th;
    const float txf = (float)x * inv_tw - 0.5f, tyf = (float)y * inv_th - 0.5f;
    int tx1 = (int)floorf(txf), ty1 = (int)floorf(tyf);
    const float xa = txf - (float)tx1, ya = tyf - (float)ty1;     // before the indices are clamped
    const float xa1 = 1.f - xa, ya1 = 1.f - ya;
    const int tx2 = min(tx1 + 1, tiles_x - 1), ty2 = min(ty1 + 1, tiles_y - 1);
    tx1 = max(tx1, 0); ty1 = max(ty1, 0);
    const int v = gray[(size_t)y * w + x];
    const float l11 = (float)lut[((size_t)ty1 * tiles_x + tx1) * 256 + v], l12 = (float)lut[((size_t)ty1 * tiles_x + tx2) * 256 + v];
    const float l21 = (float)lut[((size_t)ty2 * tiles_x + tx1) * 256 + v], l22 = (float)lut[((size_t)ty2 * tiles_x + tx2) * 256 + v];
    const float res = (l11 * xa1 + l12 * xa) * ya1 + (l21 * xa1 + l22 * xa) * ya;
    dst[(size_t)y * w + x] = front_sat_rint(res);
}

__global__ void k_front_gray(const uint8_t* __restrict__ src, int stride, int ch, int w, int h, uint8_t* __restrict__ dst) {
    front_gray_px(src, stride, ch, w, dst);
}
__global__ __launch_bounds__(256) void k_front_clahe_lut(const uint8_t* __restrict__ gray, int w, int h, int tw, int th, int clip,
                                                         uint8_t* __restrict__ lut) {
    front_clahe_lut_tile(gray, w, h, tw, th, clip, lut);
}
__global__ void k_front_clahe_apply(const uint8_t* __restrict__ gray, int w, int h, int tw, int th, int tiles_x, int tiles_y,
                                    const uint8_t* __restrict__ lut, uint8_t* __restrict__ dst) {
    front_clahe_blend_px(gray, w, h, tw, th, tiles_x, tiles_y, lut, dst);
}

// The pair forms (nrs_front_process_stereo): one launch per stage over both eyes, blockIdx.z is the eye, so an eye's bytes are the bytes of
// that image processed alone.  The LUT stage is 2 x 64 workgroups of 1 KiB LDS each: with one workgroup per tile a single frame fills 64 of
// the 256 CUs, the pair 128, and the LDS histogram atomics of the two eyes never meet (a workgroup owns its tile's 256 bins).
struct Eyes {
    uint8_t* p[2];
    __device__ uint8_t* mine() const { return blockIdx.z ? p[1] : p[0]; }
};

__global__ void k_front_gray_pair(Eyes src, int stride, int ch, int w, int h, Eyes dst) { front_gray_px(src.mine(), stride, ch, w, dst.mine()); }
__global__ __launch_bounds__(256) void k_front_clahe_lut_pair(Eyes grays, int w, int h, int tw, int th, int clip, Eyes luts) {
    front_clahe_lut_tile(grays.mine(), w, h, tw, th, clip, luts.mine());
}
__global__ void k_front_clahe_apply_pair(Eyes grays, int w, int h, int tw, int th, int tiles_x, int tiles_y, Eyes luts, Eyes dsts) {
    front_clahe_blend_px(grays.mine(), w, h, tw, th, tiles_x, tiles_y, luts.mine(), dsts.mine());
}

// ---- stereo rectification (nrs_rect_host.hpp holds the per-pixel bodies: the stand-alone check runs the same ones) ----------------------
struct RectEyes { RectEye e[2]; };

__device__ inline uint2 rect_pack(RectTap t) { uint2 v; __builtin_memcpy(&v, &t, 8); return v; }
__device__ inline RectTap rect_unpack(uint2 v) { RectTap t; __builtin_memcpy(&t, &v, 8); return t; }

// once per configuration: one thread per destination pixel, rows of 256, the eye in grid.z
__global__ __launch_bounds__(256) void k_front_rect_map(RectEyes eyes, int dw, int dh, uint2* __restrict__ taps, float* __restrict__ maps) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, eye = blockIdx.z;
    if (x >= dw) return;
    const size_t n = (size_t)dw * dh, i = (size_t)y * dw + x;
    float mx, my;
    rect_map_px(eye ? eyes.e[1] : eyes.e[0], x, y, &mx, &my);
    maps[(size_t)(2 * eye) * n + i] = mx;
    maps[(size_t)(2 * eye + 1) * n + i] = my;
    taps[(size_t)eye * n + i] = rect_pack(rect_fix(mx, my));
}

// The hot path of a raw pair: one output pixel per thread, rows of 256, the eye in grid.z.  The tap is read coalesced (8 bytes a thread), the
// four source pixels of every channel are gathered from the raw upload (packed rows; at the workload's size an eye lies in L2), the grey byte
// is computed from the ROUNDED channel bytes -- remap first, then front_gray_px's formula: the reference's order -- and written directly.
// COLOUR: the rectified pixel is written too (a rect_*_out pointer was given, or NRS_RECT_OWN_LAUNCH); GRAY = false leaves the grey to
// k_front_gray_pair (NRS_RECT_OWN_LAUNCH).  No LDS staging: neighbouring threads' taps are neighbours in the source, the gather already
// hits the lines its wave has just fetched, and a tile's source footprint is not known before the map is read
template <int CH, bool COLOUR, bool GRAY>
__global__ __launch_bounds__(256) void k_front_rect_gray_pair(Eyes raw, int sw, int sh, const uint2* __restrict__ taps, int dw, int dh, Eyes gray,
                                                              Eyes colour) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= dw) return;
    const size_t n = (size_t)dw * dh, i = (size_t)y * dw + x;
    const RectTap t = rect_unpack(taps[(size_t)blockIdx.z * n + i]);
    int v[CH];
    rect_sample_px<CH>(raw.mine(), sw * CH, sw, sh, t, v);
    if (COLOUR) {
        uint8_t* d = colour.mine() + i * CH;
#pragma unroll
        for (int c = 0; c < CH; ++c) d[c] = (uint8_t)v[c];
    }
    if (GRAY) {
        int g = v[0];
        if constexpr (CH > 1) g = (v[0] * 9798 + v[1] * 19235 + v[2] * 3735 + (1 << 14)) >> 15;
        gray.mine()[i] = (uint8_t)g;
    }
}

// ---- frame resize (nrs_resize_host.hpp holds the tables' rule and the pixel bodies: the stand-alone check runs the same ones) ------------
struct ResizeTabs {
    const int32_t* sx; const int32_t* sy;      // [dw], [dh][2]
    const short2* ax; const short2* by;        // [dw], [dh]: the two weights of a tap, one 4-byte load
};

// The hot path of a raw frame: one output pixel per thread, a workgroup is 256 consecutive pixels of one output row.  Lane-to-pixel mapping:
// the frame is interleaved bytes (1, 3 or 4 a pixel) and the kernel is memory-bound (1440 x 1080 x 3: 4.7 MB in, 0.4 MB grey out).
// Consecutive lanes take consecutive output pixels, so in the box branch a wave reads two contiguous runs of 64 * 2 * CH bytes (one per
// source row) and the workgroup's runs follow each other without a gap: every fetched line is used whole, by this wave or the next.
// The per-lane loads stay byte loads -- a pixel pair is 6 bytes at CH = 3 and a row may begin at any byte, so nothing wider is aligned --
// and what the lanes of a wave do not merge, L2 absorbs: a line is touched by at most two neighbouring waves of one workgroup.  The general
// branch reads the column tap coalesced (4 + 4 bytes a lane), the row tap is the same for the whole workgroup (scalar loads), and the
// source runs are contiguous up to the scale.  The grey byte is computed from the ROUNDED channel bytes -- resize first, then
// front_gray_px's formula: the reference's order.  COLOUR: the resized pixel is written too (resized_out, or NRS_RESIZE_OWN_LAUNCH);
// GRAY = false leaves the grey to k_front_gray (NRS_RESIZE_OWN_LAUNCH).  No LDS: no byte is read twice by one workgroup in the box
// branch, and in the general branch only the shared tap of two neighbouring lanes is
template <int CH, bool BOX, bool COLOUR, bool GRAY>
__global__ __launch_bounds__(256) void k_front_resize_gray(const uint8_t* __restrict__ raw, int stride, ResizeTabs t, int dw, int dh,
                                                           uint8_t* __restrict__ gray, uint8_t* __restrict__ colour) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= dw || y >= dh) return;
    const size_t i = (size_t)y * dw + x;
    int v[CH];
    if constexpr (BOX) {
        resize_box_px<CH>(raw, stride, x, y, v);
    } else {
        const short2 a = t.ax[x], b = t.by[y];
        resize_sample_px<CH>(raw, stride, t.sx[x], a.x, a.y, t.sy[2 * y], t.sy[2 * y + 1], b.x, b.y, v);
    }
    if (COLOUR) {
        uint8_t* d = colour + i * CH;
#pragma unroll
        for (int c = 0; c < CH; ++c) d[c] = (uint8_t)v[c];
    }
    if (GRAY) {
        int g = v[0];
        if constexpr (CH > 1) g = (v[0] * 9798 + v[1] * 19235 + v[2] * 3735 + (1 << 14)) >> 15;
        gray[i] = (uint8_t)g;
    }
}

// ---- morphology -------------------------------------------------------------------------------------------------------------
// block (32, 8); THRESH: the source pixel is replaced by (v > th ? 0 : 255) while it is staged (BrightFilter)
template <bool THRESH>
__global__ __launch_bounds__(FRONT_TX * FRONT_TY) void k_front_erode_ellipse(const uint8_t* __restrict__ src, int w, int h, int th, EllSpans e,
                                                                             uint8_t* __restrict__ dst) {
    __shared__ uint8_t tile[(FRONT_TY + FRONT_KMAX - 1) * (FRONT_TX + FRONT_KMAX - 1)];
    const int a = e.k / 2, tw = FRONT_TX + e.k - 1, thh = FRONT_TY + e.k - 1;
    const int x0 = blockIdx.x * FRONT_TX - a, y0 = blockIdx.y * FRONT_TY - a;
    const int tid = threadIdx.y * FRONT_TX + threadIdx.x;
    for (int i = tid; i < tw * thh; i += FRONT_TX * FRONT_TY) {
        const int ty = i / tw, tx = i - ty * tw, gx = x0 + tx, gy = y0 + ty;
        int v = 255;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            v = src[(size_t)gy * w + gx];
            if (THRESH) v = v > th ? 0 : 255;
        }
        tile[i] = (uint8_t)v;
    }
    __syncthreads();
    const int x = blockIdx.x * FRONT_TX + threadIdx.x, y = blockIdx.y * FRONT_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    int m = 255;
    for (int i = 0; i < e.k; ++i) {
        const uint8_t* row = tile + (threadIdx.y + i) * tw + threadIdx.x;
        for (int j = e.lo[i]; j < e.hi[i]; ++j) m = min(m, (int)row[j]);
    }
    dst[(size_t)y * w + x] = (uint8_t)m;
}

__device__ inline int front_load(const PlainSrc& s, int w, int x, int y) { return s.p[(size_t)y * w + x]; }
__device__ inline int front_load(const BorderSrc& s, int w, int x, int y) {
    return (x >= s.x0 && x < s.x1 && y >= s.y0 && y < s.y1 && s.gray[(size_t)y * w + x] != 0) ? 255 : 0;
}
__device__ inline int front_load(const AndSrc& s, int w, int x, int y) {
    int v = 255;
    for (int i = 0; i < s.n; ++i) v &= s.p[i][(size_t)y * w + x];
    return v;
}

// the window of a k-wide rectangle covers x - k/2 .. x - k/2 + k - 1 (anchor k/2)
template <class S>
__global__ void k_front_rowmin(S s, int w, int h, int k, uint8_t* __restrict__ dst) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const int lo = max(x - k / 2, 0), hi = min(x - k / 2 + k - 1, w - 1);
    int m = 255;
    for (int xx = lo; xx <= hi; ++xx) m = min(m, front_load(s, w, xx, y));
    dst[(size_t)y * w + x] = (uint8_t)m;
}

__global__ void k_front_colmin(const uint8_t* __restrict__ src, int w, int h, int k, uint8_t* __restrict__ dst) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const int lo = max(y - k / 2, 0), hi = min(y - k / 2 + k - 1, h - 1);
    int m = 255;
    for (int yy = lo; yy <= hi; ++yy) m = min(m, (int)src[(size_t)yy * w + x]);
    dst[(size_t)y * w + x] = (uint8_t)m;
}

// ---- the Gaussian of BrightFilter (DESIGN.md "f5": defined here, OpenCV's fixed-point path is not reproduced) ---------------
__global__ void k_front_gauss_h(const uint8_t* __restrict__ src, int w, int h, GaussW g, float* __restrict__ dst) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const uint8_t* row = src + (size_t)y * w;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 11; ++i) acc = acc + g.w[i] * (float)row[reflect101(x + i - 5, w)];
    dst[(size_t)y * w + x] = acc;
}

__global__ void k_front_gauss_v(const float* __restrict__ src, int w, int h, GaussW g, uint8_t* __restrict__ dst) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 11; ++i) acc = acc + g.w[i] * src[(size_t)reflect101(y + i - 5, h) * w + x];
    dst[(size_t)y * w + x] = front_sat_rint(acc);
}

// mask value under each keypoint (Tracking::ExtractFeatures, tracking.cc:126: mask.at<uchar>(pt), coordinates truncated)
__global__ void k_front_mask_at(const uint8_t* __restrict__ mask, int w, int h, const float* __restrict__ xy, int n, uint8_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int x = (int)xy[2 * i], y = (int)xy[2 * i + 1];
    out[i] = (x >= 0 && x < w && y >= 0 && y < h) ? mask[(size_t)y * w + x] : 0;
}

// ---- host side --------------------------------------------------------------------------------------------------------------
void front_free(nrs_ctx* c) {
    delete c->front;
    c->front = nullptr;
}

// getStructuringElement(MORPH_ELLIPSE, Size(k, k)): r = c = k/2, row i spans [max(c-dx,0), min(c+dx+1,k)), dx = rint(c sqrt((r^2-dy^2)/r^2))
static EllSpans ellipse_spans(int k) {
    EllSpans e;
    e.k = k;
    const int r = k / 2, c = k / 2;
    for (int i = 0; i < FRONT_KMAX; ++i) { e.lo[i] = 0; e.hi[i] = 0; }
    for (int i = 0; i < k; ++i) {
        const int dy = i - r;
        if (std::abs(dy) > r) continue;
        const int dx = (int)std::nearbyint((double)c * std::sqrt((double)(r * r - dy * dy) / (double)(r * r)));
        e.lo[i] = (signed char)std::max(c - dx, 0);
        e.hi[i] = (signed char)std::min(c + dx + 1, k);
    }
    return e;
}

// g_i = float(exp(-i^2/50)), their float sum from i = -5 upwards, w_i = g_i / sum in float
static GaussW gauss_weights() {
    GaussW g;
    float s = 0.f;
    for (int i = 0; i < 11; ++i) { g.w[i] = (float)std::exp(-(double)((i - 5) * (i - 5)) / 50.0); s = s + g.w[i]; }
    for (int i = 0; i < 11; ++i) g.w[i] = g.w[i] / s;
    return g;
}

static inline dim3 front_grid(int w, int h) { return dim3((w + 255) / 256, h); }
static inline dim3 front_tiles(int w, int h) { return dim3((w + FRONT_TX - 1) / FRONT_TX, (h + FRONT_TY - 1) / FRONT_TY); }

static FrontState* front_default(nrs_ctx* c) {
    if (!c->front) {
        FrontState* f = new (std::nothrow) FrontState();
        if (!f) return nullptr;
        f->e11 = ellipse_spans(11); f->e20 = ellipse_spans(20); f->gw = gauss_weights();
        c->front = f;
    }
    return c->front;
}

// what is resident (a frame, or -- pair -- both eyes), its size and the image selector
static int front_resident_check(nrs_ctx* c, const char* who, bool pair, int w, int h, int image) {
    const FrontState* f = c->front;
    if (!f || !f->valid || (pair && !f->valid_right))
        return c->fail(NRS_ERR_STATE, "%s: no %s has been processed (nrs_front_process%s)", who, pair ? "stereo pair" : "frame", pair ? "_stereo" : "");
    if (w != f->w || h != f->h) return c->fail(NRS_ERR_STATE, "%s: the resident %s is %d x %d, not %d x %d", who, pair ? "pair" : "frame", f->w, f->h, w, h);
    if (image != NRS_FRONT_IMAGE_GRAY && image != NRS_FRONT_IMAGE_CLAHE) return c->fail(NRS_ERR_INVALID, "%s: image selector must be GRAY or CLAHE", who);
    return NRS_OK;
}

int front_resident(nrs_ctx* c, const char* who, int w, int h, int image, int use_global_mask, const uint8_t** img, const uint8_t** mask) {
    NRS_TRY(front_resident_check(c, who, false, w, h, image));
    const FrontState* f = c->front;
    *img = image == NRS_FRONT_IMAGE_GRAY ? f->gray.as<uint8_t>() : f->clahe.as<uint8_t>();
    *mask = use_global_mask ? f->global.as<uint8_t>() : nullptr;
    return NRS_OK;
}

int front_resident_pair(nrs_ctx* c, const char* who, int w, int h, int image, const uint8_t** left, const uint8_t** right) {
    NRS_TRY(front_resident_check(c, who, true, w, h, image));
    const FrontState* f = c->front;
    *left = image == NRS_FRONT_IMAGE_GRAY ? f->gray.as<uint8_t>() : f->clahe.as<uint8_t>();
    *right = image == NRS_FRONT_IMAGE_GRAY ? f->gray_r.as<uint8_t>() : f->clahe_r.as<uint8_t>();
    return NRS_OK;
}

int front_mask_at(nrs_ctx* c, const uint8_t* d_mask, int w, int h, const float* d_xy, int n, uint8_t* host_out) {
    FrontState* f = c->front;
    if (!f) return c->fail(NRS_ERR_STATE, "no front-end state");
    if (n <= 0) return NRS_OK;
    NRS_TRY(c->ensure(f->at, (size_t)n));
    hipLaunchKernelGGL(k_front_mask_at, dim3((n + 255) / 256), dim3(256), 0, c->stream, d_mask, w, h, d_xy, n, f->at.as<uint8_t>());
    NRS_HIP(c, hipGetLastError());
    NRS_HIP(c, hipMemcpyAsync(host_out, f->at.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    return NRS_OK;
}

}  // namespace nrs

using namespace nrs;

extern "C" int nrs_front_configure(nrs_ctx* c, int32_t n_filters, const nrs_front_filter* filters, float clahe_clip, int32_t tiles_x,
                                   int32_t tiles_y) {
    if (!c) return NRS_ERR_INVALID;
    if (n_filters < 0 || n_filters > NRS_FRONT_MAX_FILTERS || (n_filters > 0 && !filters))
        return c->fail(NRS_ERR_INVALID, "nrs_front_configure: 0..%d filters", NRS_FRONT_MAX_FILTERS);
    if (tiles_x != 8 || tiles_y != 8) return c->fail(NRS_ERR_INVALID, "nrs_front_configure: only the reference's 8x8 CLAHE grid is built (SLAM/system.cc)");
    if (!(clahe_clip > 0.f)) return c->fail(NRS_ERR_INVALID, "nrs_front_configure: clahe_clip must be positive");
    for (int i = 0; i < n_filters; ++i) {
        const nrs_front_filter& q = filters[i];
        if (q.kind == NRS_FRONT_BORDER) {
            if (q.p[0] < 0 || q.p[1] < 0 || q.p[2] < 0 || q.p[3] < 0) return c->fail(NRS_ERR_INVALID, "nrs_front_configure: filter %d: the ROI leaves the image", i);
        } else if (q.kind == NRS_FRONT_PREDEFINED) {
            if (!q.mask || q.w <= 0 || q.h <= 0 || q.stride < q.w) return c->fail(NRS_ERR_INVALID, "nrs_front_configure: filter %d: bad predefined mask", i);
        } else if (q.kind != NRS_FRONT_BRIGHT) {
            return c->fail(NRS_ERR_INVALID, "nrs_front_configure: filter %d: unknown kind %d", i, q.kind);
        }
    }
    NRS_HIP(c, hipSetDevice(c->device));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    // the rectification maps and the resize tables are no part of the filter configuration: they move into whatever state this call
    // leaves (a refusal below leaves the default one)
    struct KeepMaps {
        nrs_ctx* c;
        RectState r;
        ResizeState z;
        ~KeepMaps() {
            if (!r.on && !z.on) return;
            FrontState* s = front_default(c);
            if (s && r.on) s->rect = std::move(r);
            if (s && z.on) s->resize = std::move(z);
        }
    } keep{c, c->front ? std::move(c->front->rect) : RectState(), c->front ? std::move(c->front->resize) : ResizeState()};
    front_free(c);                                                 // a fresh Masker: nothing of the old configuration or its frame is kept
    FrontState* f = front_default(c);
    if (!f) return c->fail(NRS_ERR_ALLOC, "out of host memory");
    f->clip = clahe_clip; f->tiles_x = tiles_x; f->tiles_y = tiles_y;
    f->filters.resize((size_t)n_filters);
    for (int i = 0; i < n_filters; ++i) {
        const nrs_front_filter& q = filters[i];
        FrontFilter& d = f->filters[i];
        d.kind = q.kind;
        for (int j = 0; j < 5; ++j) d.p[j] = q.p[j];
        if (q.kind != NRS_FRONT_PREDEFINED) continue;
        // PredefinedFilter's constructor: the mask eroded once by the 20x20 ellipse (predefined_filter.cc:27-34)
        d.mw = q.w; d.mh = q.h;
        const size_t n = (size_t)q.w * q.h;
        int rc = c->ensure(f->tmp_a, n);
        if (rc == NRS_OK) rc = c->ensure(f->fmask[i], n);
        if (rc != NRS_OK) { front_free(c); return rc; }
        hipError_t he = hipMemcpy2DAsync(f->tmp_a.p, (size_t)q.w, q.mask, (size_t)q.stride, (size_t)q.w, (size_t)q.h, hipMemcpyHostToDevice, c->stream);
        if (he == hipSuccess) {
            hipLaunchKernelGGL(k_front_erode_ellipse<false>, front_tiles(q.w, q.h), dim3(FRONT_TX, FRONT_TY), 0, c->stream, f->tmp_a.as<uint8_t>(), q.w, q.h, 0,
                               f->e20, f->fmask[i].as<uint8_t>());
            he = hipGetLastError();
        }
        if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
        if (he != hipSuccess) { front_free(c); return c->fail(NRS_ERR_HIP, "nrs_front_configure: predefined mask: %s", hipGetErrorString(he)); }
    }
    return NRS_OK;
}

// what a raw pair adds to a pair's arguments: where the rectified eyes go (nullable)
struct RawPair { uint8_t* rect_left_out; uint8_t* rect_right_out; };

// the remap of both eyes: with the grey and, where `colour`, the rectified pixel too; or (gray false) the rectified pixel alone
template <int CH>
static void front_rect_launch(nrs_ctx* c, const RectState& r, bool colour, bool gray, Eyes raws, Eyes grays, Eyes colours) {
    const dim3 grid((r.dw + 255) / 256, r.dh, 2), blk(256);
    const uint2* taps = r.taps.as<uint2>();
    if (colour && gray) hipLaunchKernelGGL((k_front_rect_gray_pair<CH, true, true>), grid, blk, 0, c->stream, raws, r.sw, r.sh, taps, r.dw, r.dh, grays, colours);
    else if (gray) hipLaunchKernelGGL((k_front_rect_gray_pair<CH, false, true>), grid, blk, 0, c->stream, raws, r.sw, r.sh, taps, r.dw, r.dh, grays, colours);
    else hipLaunchKernelGGL((k_front_rect_gray_pair<CH, true, false>), grid, blk, 0, c->stream, raws, r.sw, r.sh, taps, r.dw, r.dh, grays, colours);
}

// what a raw frame adds to a frame's arguments: where the resized frame goes (nullable)
struct RawFrame { uint8_t* resized_out; };

// the resize of a frame: with the grey and, where `colour`, the resized pixel too; or (gray false) the resized pixel alone
template <int CH, bool BOX>
static void front_resize_launch_b(nrs_ctx* c, const ResizeState& z, bool colour, bool gray, const uint8_t* raw, uint8_t* grays, uint8_t* colours) {
    const dim3 grid((z.dw + 255) / 256, z.dh), blk(256);
    const int32_t* i32 = z.tabs.as<int32_t>();
    const short2* i16 = reinterpret_cast<const short2*>(i32 + z.dw + 2 * (size_t)z.dh);
    const ResizeTabs t{i32, i32 + z.dw, i16, i16 + z.dw};
    const int stride = z.sw * CH;
    if (colour && gray) hipLaunchKernelGGL((k_front_resize_gray<CH, BOX, true, true>), grid, blk, 0, c->stream, raw, stride, t, z.dw, z.dh, grays, colours);
    else if (gray) hipLaunchKernelGGL((k_front_resize_gray<CH, BOX, false, true>), grid, blk, 0, c->stream, raw, stride, t, z.dw, z.dh, grays, colours);
    else hipLaunchKernelGGL((k_front_resize_gray<CH, BOX, true, false>), grid, blk, 0, c->stream, raw, stride, t, z.dw, z.dh, grays, colours);
}
template <int CH>
static void front_resize_launch(nrs_ctx* c, const ResizeState& z, bool colour, bool gray, const uint8_t* raw, uint8_t* grays, uint8_t* colours) {
    if (z.box) front_resize_launch_b<CH, true>(c, z, colour, gray, raw, grays, colours);
    else front_resize_launch_b<CH, false>(c, z, colour, gray, raw, grays, colours);
}

// One frame (right == nullptr: nrs_front_process, the single-frame kernels) or a stereo pair (nrs_front_process_stereo: the right eye is
// uploaded next to the left one and takes grey + CLAHE in the same launches; the masks are the left eye's).  Everything else is shared.
// raw != nullptr (nrs_front_process_stereo_raw): img / right are the RAW eyes of w x h; the first stage rectifies them into the configured
// dst_w x dst_h, which is the size of everything after it -- from the CLAHE LUTs onward nothing knows the difference.
// rawf != nullptr (nrs_front_process_raw): img is the RAW frame of w x h; the first stage resizes it into the configured dst_w x dst_h, in the
// same way.
static int front_run(nrs_ctx* c, const char* who, const uint8_t* img, const uint8_t* right, int32_t w, int32_t h, int32_t stride, int32_t stride_r,
                     int32_t channels, uint8_t* gray_out, uint8_t* clahe_out, uint8_t* global_out, uint8_t* const* filter_masks_out,
                     uint8_t* gray_right_out, uint8_t* clahe_right_out, const RawPair* raw = nullptr, const RawFrame* rawf = nullptr) {
    if (!img || w <= 0 || h <= 0) return c->fail(NRS_ERR_INVALID, "%s: empty image", who);
    if (channels != 1 && channels != 3 && channels != 4) return c->fail(NRS_ERR_INVALID, "%s: %d channels (1, 3 or 4)", who, channels);
    if ((int64_t)stride < (int64_t)w * channels || (right && (int64_t)stride_r < (int64_t)w * channels))
        return c->fail(NRS_ERR_INVALID, "%s: stride below the row length", who);
    NRS_HIP(c, hipSetDevice(c->device));
    FrontState* f = front_default(c);                              // (never configured: no filters, clip 3.0, 8x8)
    if (!f) return c->fail(NRS_ERR_ALLOC, "out of host memory");
    const int sw = w, sh = h;                                      // what is uploaded
    if (raw) {
        char msg[256];
        const int bad = rect_check_raw(f->rect.on, f->rect.sw, f->rect.sh, w, h, msg, sizeof msg);
        if (bad) return c->fail(bad == -2 ? NRS_ERR_STATE : NRS_ERR_INVALID, "%s", msg);
        w = f->rect.dw; h = f->rect.dh;                            // ... and what is processed
    }
    if (rawf) {
        char msg[256];
        const int bad = resize_check_raw(f->resize.on, f->resize.sw, f->resize.sh, w, h, msg, sizeof msg);
        if (bad) return c->fail(bad == -2 ? NRS_ERR_STATE : NRS_ERR_INVALID, "%s", msg);
        w = f->resize.dw; h = f->resize.dh;
    }
    const int nf = (int)f->filters.size();
    BorderSrc bsrc[NRS_FRONT_MAX_FILTERS];
    for (int i = 0; i < nf; ++i) {
        const FrontFilter& q = f->filters[i];
        if (q.kind == NRS_FRONT_PREDEFINED && (q.mw != w || q.mh != h))
            return c->fail(NRS_ERR_INVALID, "%s: filter %d: the predefined mask is %d x %d, the image %d x %d", who, i, q.mw, q.mh, w, h);
        if (q.kind == NRS_FRONT_BORDER) {                          // cv::Rect(cb, rb, w - ce - cb, h - re - rb)
            const int rb = q.p[0], re = q.p[1], cb = q.p[2], ce = q.p[3];
            const int64_t rw = (int64_t)w - ce - cb, rh = (int64_t)h - re - rb;
            if (rw <= 0 || rh <= 0 || cb + rw > w || rb + rh > h)
                return c->fail(NRS_ERR_INVALID, "%s: filter %d: the ROI is empty or leaves the %d x %d image", who, i, w, h);
            bsrc[i].x0 = cb; bsrc[i].y0 = rb; bsrc[i].x1 = cb + (int)rw; bsrc[i].y1 = rb + (int)rh;
        }
    }
    f->valid = false; f->valid_right = false;
    const size_t n = (size_t)w * h, row = (size_t)sw * channels;
    // a raw pair: the rectified colour eyes exist only where somebody reads them
    const bool rect_own = raw && c->dbg.is_set(SW_RECT_OWN_LAUNCH), rect_colour = raw && (rect_own || raw->rect_left_out || raw->rect_right_out);
    // a raw frame: the resized colour frame likewise
    const bool resize_own = rawf && c->dbg.is_set(SW_RESIZE_OWN_LAUNCH), resize_colour = rawf && (resize_own || rawf->resized_out);
    NRS_TRY(c->ensure(f->raw, row * sh));
    NRS_TRY(c->ensure(f->gray, n));
    if (resize_colour) NRS_TRY(c->ensure(f->resize.colour, n * channels));
    NRS_TRY(c->ensure(f->clahe, n));
    if (rect_colour) {
        NRS_TRY(c->ensure(f->rect.colour, n * channels));
        NRS_TRY(c->ensure(f->rect.colour_r, n * channels));
    }
    if (right) {
        NRS_TRY(c->ensure(f->raw_r, row * sh));
        NRS_TRY(c->ensure(f->gray_r, n));
        NRS_TRY(c->ensure(f->clahe_r, n));
        NRS_TRY(c->ensure(f->lut_r, (size_t)f->tiles_x * f->tiles_y * 256));
    }
    NRS_TRY(c->ensure(f->global, n));
    NRS_TRY(c->ensure(f->tmp_a, n));
    NRS_TRY(c->ensure(f->lut, (size_t)f->tiles_x * f->tiles_y * 256));
    for (int i = 0; i < nf; ++i) {
        if (f->filters[i].kind != NRS_FRONT_PREDEFINED) NRS_TRY(c->ensure(f->fmask[i], n));
        if (f->filters[i].kind == NRS_FRONT_BRIGHT) NRS_TRY(c->ensure(f->tmp_f, sizeof(float) * n));
    }
    // (packed rows go up as one run of bytes: a 2-D copy of 1081 rows of 4323 bytes was measured at 8 ms against 0.06 ms, DESIGN.md 4 "Frame resize")
    if ((size_t)stride == row) NRS_HIP(c, hipMemcpyAsync(f->raw.p, img, row * sh, hipMemcpyHostToDevice, c->stream));
    else NRS_HIP(c, hipMemcpy2DAsync(f->raw.p, row, img, (size_t)stride, row, (size_t)sh, hipMemcpyHostToDevice, c->stream));
    if (right && (size_t)stride_r == row) NRS_HIP(c, hipMemcpyAsync(f->raw_r.p, right, row * sh, hipMemcpyHostToDevice, c->stream));
    else if (right) NRS_HIP(c, hipMemcpy2DAsync(f->raw_r.p, row, right, (size_t)stride_r, row, (size_t)sh, hipMemcpyHostToDevice, c->stream));
    const dim3 blk(256), grid = front_grid(w, h);
    uint8_t* gray = f->gray.as<uint8_t>();
    uint8_t* tmp = f->tmp_a.as<uint8_t>();
    // CLAHE (createCLAHE(clip, Size(8,8))->apply): tiles of the image extended to multiples of the grid
    int pw = w, ph = h;
    if (w % f->tiles_x != 0 || h % f->tiles_y != 0) { pw = w + f->tiles_x - w % f->tiles_x; ph = h + f->tiles_y - h % f->tiles_y; }
    const int tw = pw / f->tiles_x, th = ph / f->tiles_y;
    const int clip = std::max(1, (int)(f->clip * (float)(tw * th) / 256.f));
    const Eyes raws{{f->raw.as<uint8_t>(), f->raw_r.as<uint8_t>()}}, grays{{gray, f->gray_r.as<uint8_t>()}};
    const Eyes luts{{f->lut.as<uint8_t>(), f->lut_r.as<uint8_t>()}}, clahes{{f->clahe.as<uint8_t>(), f->clahe_r.as<uint8_t>()}};
    if (raw) {                                                     // the first stage of a raw pair: remap + grey, always over both eyes
        const Eyes colours{{f->rect.colour.as<uint8_t>(), f->rect.colour_r.as<uint8_t>()}};
        if (channels == 1) front_rect_launch<1>(c, f->rect, rect_colour, !rect_own, raws, grays, colours);
        else if (channels == 3) front_rect_launch<3>(c, f->rect, rect_colour, !rect_own, raws, grays, colours);
        else front_rect_launch<4>(c, f->rect, rect_colour, !rect_own, raws, grays, colours);
        if (rect_own)                                              // NRS_RECT_OWN_LAUNCH: the grey of the rectified colour eyes, as of any pair
            hipLaunchKernelGGL(k_front_gray_pair, dim3(grid.x, grid.y, 2), blk, 0, c->stream, colours, (int)(w * channels), channels, w, h, grays);
    }
    if (rawf) {                                                    // the first stage of a raw frame: resize + grey
        uint8_t* col = f->resize.colour.as<uint8_t>();
        if (channels == 1) front_resize_launch<1>(c, f->resize, resize_colour, !resize_own, raws.p[0], gray, col);
        else if (channels == 3) front_resize_launch<3>(c, f->resize, resize_colour, !resize_own, raws.p[0], gray, col);
        else front_resize_launch<4>(c, f->resize, resize_colour, !resize_own, raws.p[0], gray, col);
        if (resize_own)                                            // NRS_RESIZE_OWN_LAUNCH: the grey of the resized colour frame, as of any frame
            hipLaunchKernelGGL(k_front_gray, grid, blk, 0, c->stream, col, (int)(w * channels), channels, w, h, gray);
    }
    if (right && !c->dbg.is_set(SW_FRONT_PER_EYE)) {               // the pair: one launch per shared stage, the eye in grid.z
        if (!raw) hipLaunchKernelGGL(k_front_gray_pair, dim3(grid.x, grid.y, 2), blk, 0, c->stream, raws, (int)row, channels, w, h, grays);
        hipLaunchKernelGGL(k_front_clahe_lut_pair, dim3(f->tiles_x, f->tiles_y, 2), blk, 0, c->stream, grays, w, h, tw, th, clip, luts);
        hipLaunchKernelGGL(k_front_clahe_apply_pair, dim3(grid.x, grid.y, 2), blk, 0, c->stream, grays, w, h, tw, th, f->tiles_x, f->tiles_y, luts, clahes);
    } else {
        for (int e = 0; e < (right ? 2 : 1); ++e) {                // a single frame, or NRS_FRONT_PER_EYE: the right eye through the same three kernels
            if (!raw && !rawf) hipLaunchKernelGGL(k_front_gray, grid, blk, 0, c->stream, raws.p[e], (int)row, channels, w, h, grays.p[e]);
            hipLaunchKernelGGL(k_front_clahe_lut, dim3(f->tiles_x, f->tiles_y), blk, 0, c->stream, grays.p[e], w, h, tw, th, clip, luts.p[e]);
            hipLaunchKernelGGL(k_front_clahe_apply, grid, blk, 0, c->stream, grays.p[e], w, h, tw, th, f->tiles_x, f->tiles_y, luts.p[e], clahes.p[e]);
        }
    }
    AndSrc all;
    all.n = nf;
    for (int i = 0; i < NRS_FRONT_MAX_FILTERS; ++i) all.p[i] = nullptr;
    for (int i = 0; i < nf; ++i) {
        const FrontFilter& q = f->filters[i];
        uint8_t* m = f->fmask[i].as<uint8_t>();
        all.p[i] = m;
        if (q.kind == NRS_FRONT_BRIGHT) {
            hipLaunchKernelGGL(k_front_erode_ellipse<true>, front_tiles(w, h), dim3(FRONT_TX, FRONT_TY), 0, c->stream, gray, w, h, q.p[0], f->e11, tmp);
            hipLaunchKernelGGL(k_front_gauss_h, grid, blk, 0, c->stream, tmp, w, h, f->gw, f->tmp_f.as<float>());
            hipLaunchKernelGGL(k_front_gauss_v, grid, blk, 0, c->stream, f->tmp_f.as<float>(), w, h, f->gw, m);
        } else if (q.kind == NRS_FRONT_BORDER) {
            bsrc[i].gray = gray;
            hipLaunchKernelGGL(k_front_rowmin<BorderSrc>, grid, blk, 0, c->stream, bsrc[i], w, h, 21, tmp);
            hipLaunchKernelGGL(k_front_colmin, grid, blk, 0, c->stream, tmp, w, h, 21, m);
        }
    }
    // Global: AND of all masks from 255, eroded by the 10x10 rectangle (masker.cc:98-110)
    hipLaunchKernelGGL(k_front_rowmin<AndSrc>, grid, blk, 0, c->stream, all, w, h, 10, tmp);
    hipLaunchKernelGGL(k_front_colmin, grid, blk, 0, c->stream, tmp, w, h, 10, f->global.as<uint8_t>());
    NRS_HIP(c, hipGetLastError());
    if (gray_out) NRS_HIP(c, hipMemcpyAsync(gray_out, f->gray.p, n, hipMemcpyDeviceToHost, c->stream));
    if (clahe_out) NRS_HIP(c, hipMemcpyAsync(clahe_out, f->clahe.p, n, hipMemcpyDeviceToHost, c->stream));
    if (global_out) NRS_HIP(c, hipMemcpyAsync(global_out, f->global.p, n, hipMemcpyDeviceToHost, c->stream));
    if (filter_masks_out)
        for (int i = 0; i < nf; ++i)
            if (filter_masks_out[i]) NRS_HIP(c, hipMemcpyAsync(filter_masks_out[i], f->fmask[i].p, n, hipMemcpyDeviceToHost, c->stream));
    if (right && gray_right_out) NRS_HIP(c, hipMemcpyAsync(gray_right_out, f->gray_r.p, n, hipMemcpyDeviceToHost, c->stream));
    if (right && clahe_right_out) NRS_HIP(c, hipMemcpyAsync(clahe_right_out, f->clahe_r.p, n, hipMemcpyDeviceToHost, c->stream));
    if (raw && raw->rect_left_out) NRS_HIP(c, hipMemcpyAsync(raw->rect_left_out, f->rect.colour.p, n * channels, hipMemcpyDeviceToHost, c->stream));
    if (raw && raw->rect_right_out) NRS_HIP(c, hipMemcpyAsync(raw->rect_right_out, f->rect.colour_r.p, n * channels, hipMemcpyDeviceToHost, c->stream));
    if (rawf && rawf->resized_out) NRS_HIP(c, hipMemcpyAsync(rawf->resized_out, f->resize.colour.p, n * channels, hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));                  // (also what lets another context read the resident images afterwards)
    f->w = w; f->h = h; f->valid = true; f->valid_right = right != nullptr;
    return NRS_OK;
}

extern "C" int nrs_front_process(nrs_ctx* c, const uint8_t* img, int32_t w, int32_t h, int32_t stride, int32_t channels, uint8_t* gray_out,
                                 uint8_t* clahe_out, uint8_t* global_out, uint8_t* const* filter_masks_out) {
    if (!c) return NRS_ERR_INVALID;
    return front_run(c, "nrs_front_process", img, nullptr, w, h, stride, 0, channels, gray_out, clahe_out, global_out, filter_masks_out, nullptr, nullptr);
}

extern "C" int nrs_front_process_stereo(nrs_ctx* c, const uint8_t* left, const uint8_t* right, int32_t w, int32_t h, int32_t stride_l,
                                        int32_t stride_r, int32_t channels, uint8_t* gray_out, uint8_t* clahe_out, uint8_t* global_out,
                                        uint8_t* const* filter_masks_out, uint8_t* gray_right_out, uint8_t* clahe_right_out) {
    if (!c) return NRS_ERR_INVALID;
    if (!right) return c->fail(NRS_ERR_INVALID, "nrs_front_process_stereo: empty image");
    return front_run(c, "nrs_front_process_stereo", left, right, w, h, stride_l, stride_r, channels, gray_out, clahe_out, global_out, filter_masks_out,
                     gray_right_out, clahe_right_out);
}

// hamlyn.cc:194-198 (initUndistortRectifyMap per eye, once): both maps in one launch
extern "C" int nrs_front_rectify_configure(nrs_ctx* c, int32_t src_w, int32_t src_h, int32_t dst_w, int32_t dst_h, const nrs_rect_eye* left,
                                           const nrs_rect_eye* right) {
    if (!c) return NRS_ERR_INVALID;
    RectEyes eyes;
    char msg[256];
    if (rect_check_configure(src_w, src_h, dst_w, dst_h, left, right, eyes.e, msg, sizeof msg) != 0) return c->fail(NRS_ERR_INVALID, "%s", msg);
    NRS_HIP(c, hipSetDevice(c->device));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    FrontState* f = front_default(c);
    if (!f) return c->fail(NRS_ERR_ALLOC, "out of host memory");
    f->valid = false; f->valid_right = false;                      // the resident frame is dropped; the filters stay
    RectState& r = f->rect;
    r.on = false;
    const size_t n = (size_t)dst_w * dst_h;
    NRS_TRY(c->ensure(r.taps, 2 * n * sizeof(uint2)));
    NRS_TRY(c->ensure(r.maps, 4 * n * sizeof(float)));
    hipLaunchKernelGGL(k_front_rect_map, dim3((dst_w + 255) / 256, dst_h, 2), dim3(256), 0, c->stream, eyes, dst_w, dst_h, r.taps.as<uint2>(), r.maps.as<float>());
    NRS_HIP(c, hipGetLastError());
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    r.sw = src_w; r.sh = src_h; r.dw = dst_w; r.dh = dst_h; r.on = true;
    return NRS_OK;
}

extern "C" int nrs_front_rectify_maps(nrs_ctx* c, int32_t eye, float* map_x, float* map_y) {
    if (!c) return NRS_ERR_INVALID;
    const char* who = "nrs_front_rectify_maps";
    if (eye != 0 && eye != 1) return c->fail(NRS_ERR_INVALID, RECT_MSG_EYE, who, eye);
    const FrontState* f = c->front;
    if (!f || !f->rect.on) return c->fail(NRS_ERR_STATE, RECT_MSG_NONE, who);
    NRS_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)f->rect.dw * f->rect.dh;
    const float* m = f->rect.maps.as<float>() + (size_t)(2 * eye) * n;
    if (map_x) NRS_HIP(c, hipMemcpyAsync(map_x, m, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (map_y) NRS_HIP(c, hipMemcpyAsync(map_y, m + n, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    return NRS_OK;
}

// hamlyn.cc:226-229 (cv::remap of both eyes) in front of nrs_front_process_stereo
extern "C" int nrs_front_process_stereo_raw(nrs_ctx* c, const uint8_t* left, const uint8_t* right, int32_t src_w, int32_t src_h, int32_t stride_l,
                                            int32_t stride_r, int32_t channels, uint8_t* gray_out, uint8_t* clahe_out, uint8_t* global_out,
                                            uint8_t* const* filter_masks_out, uint8_t* gray_right_out, uint8_t* clahe_right_out,
                                            uint8_t* rect_left_out, uint8_t* rect_right_out) {
    if (!c) return NRS_ERR_INVALID;
    if (!right) return c->fail(NRS_ERR_INVALID, "nrs_front_process_stereo_raw: empty image");
    const RawPair raw{rect_left_out, rect_right_out};
    return front_run(c, "nrs_front_process_stereo_raw", left, right, src_w, src_h, stride_l, stride_r, channels, gray_out, clahe_out, global_out,
                     filter_masks_out, gray_right_out, clahe_right_out, &raw);
}

// apps/endomapper.cc:65-69 (cv::resize to the configured size, once per frame): the tap tables, computed on the host and uploaded
extern "C" int nrs_front_resize_configure(nrs_ctx* c, int32_t src_w, int32_t src_h, int32_t dst_w, int32_t dst_h) {
    if (!c) return NRS_ERR_INVALID;
    char msg[256];
    if (resize_check_configure(src_w, src_h, dst_w, dst_h, msg, sizeof msg) != 0) return c->fail(NRS_ERR_INVALID, "%s", msg);
    NRS_HIP(c, hipSetDevice(c->device));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    FrontState* f = front_default(c);
    if (!f) return c->fail(NRS_ERR_ALLOC, "out of host memory");
    f->valid = false; f->valid_right = false;                      // the resident frame is dropped; the filters and the maps stay
    ResizeState& z = f->resize;
    z.on = false;
    const size_t n32 = (size_t)dst_w + 2 * (size_t)dst_h, n16 = 2 * ((size_t)dst_w + (size_t)dst_h);
    std::vector<int32_t> i32;
    std::vector<int16_t> i16;
    try { i32.resize(n32); i16.resize(n16); } catch (const std::bad_alloc&) { return c->fail(NRS_ERR_ALLOC, "out of host memory"); }
    resize_build_taps(src_w, src_h, dst_w, dst_h, i32.data(), i16.data(), i32.data() + dst_w, i16.data() + 2 * (size_t)dst_w);
    NRS_TRY(c->ensure(z.tabs, n32 * sizeof(int32_t) + n16 * sizeof(int16_t)));
    NRS_HIP(c, hipMemcpyAsync(z.tabs.p, i32.data(), n32 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipMemcpyAsync(z.tabs.as<int32_t>() + n32, i16.data(), n16 * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));                   // (the vectors go when this returns)
    z.sw = src_w; z.sh = src_h; z.dw = dst_w; z.dh = dst_h; z.box = resize_is_box(src_w, src_h, dst_w, dst_h); z.on = true;
    return NRS_OK;
}

extern "C" int nrs_front_resize_taps(nrs_ctx* c, int32_t* sx, int16_t* ax, int32_t* sy, int16_t* by, int32_t* box) {
    if (!c) return NRS_ERR_INVALID;
    const FrontState* f = c->front;
    if (!f || !f->resize.on) return c->fail(NRS_ERR_STATE, RESIZE_MSG_NONE, "nrs_front_resize_taps");
    NRS_HIP(c, hipSetDevice(c->device));
    const ResizeState& z = f->resize;
    const size_t dw = (size_t)z.dw, dh = (size_t)z.dh;
    const int32_t* i32 = z.tabs.as<int32_t>();
    const int16_t* i16 = reinterpret_cast<const int16_t*>(i32 + dw + 2 * dh);
    if (sx) NRS_HIP(c, hipMemcpyAsync(sx, i32, dw * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (sy) NRS_HIP(c, hipMemcpyAsync(sy, i32 + dw, 2 * dh * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (ax) NRS_HIP(c, hipMemcpyAsync(ax, i16, 2 * dw * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    if (by) NRS_HIP(c, hipMemcpyAsync(by, i16 + 2 * dw, 2 * dh * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    if (box) *box = z.box ? 1 : 0;
    return NRS_OK;
}

// apps/endomapper.cc:65-69 (cv::resize of the frame) in front of nrs_front_process
extern "C" int nrs_front_process_raw(nrs_ctx* c, const uint8_t* img, int32_t src_w, int32_t src_h, int32_t stride, int32_t channels,
                                     uint8_t* gray_out, uint8_t* clahe_out, uint8_t* global_out, uint8_t* const* filter_masks_out,
                                     uint8_t* resized_out) {
    if (!c) return NRS_ERR_INVALID;
    const RawFrame rawf{resized_out};
    return front_run(c, "nrs_front_process_raw", img, nullptr, src_w, src_h, stride, 0, channels, gray_out, clahe_out, global_out, filter_masks_out,
                     nullptr, nullptr, nullptr, &rawf);
}
