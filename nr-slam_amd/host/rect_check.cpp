// Stand-alone check of the host half of the stereo rectification (csrc/nrs_rect_host.hpp) under AddressSanitizer + UBSan: `make rect_check`
// (builds and runs it).  No HIP, no library.  The per-pixel bodies checked here -- the map, the fixed-point tap, the blend -- are the ones
// the kernels of nrs_front.hip run.  The expected values of the tiny remap at the end come from tests/rect_oracle.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "../csrc/nrs_rect_host.hpp"

using namespace nrs;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

static nrs_rect_eye make_eye(double f, double cx, double cy) {
    nrs_rect_eye e;
    memset(&e, 0, sizeof e);
    e.K[0] = e.K[4] = f; e.K[2] = cx; e.K[5] = cy; e.K[8] = 1;
    memcpy(e.P, e.K, sizeof e.P);
    e.R[0] = e.R[4] = e.R[8] = 1;
    return e;
}

static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

int main() {
    char msg[256];
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    RectEye out[2];
    // ---- nrs_front_rectify_configure's refusals
    {
        const nrs_rect_eye good = make_eye(64, 32, 24);
        auto cfg = [&](int sw, int sh, int dw, int dh, const nrs_rect_eye* l, const nrs_rect_eye* r) { return rect_check_configure(sw, sh, dw, dh, l, r, out, msg, sizeof msg); };
        CHECK(cfg(64, 48, 70, 52, &good, &good) == 0);
        CHECK(cfg(1, 1, RECT_MAX_SIZE, RECT_MAX_SIZE, &good, &good) == 0);
        CHECK(cfg(64, 48, 70, 52, nullptr, &good) != 0 && strcmp(msg, "nrs_front_rectify_configure: null eye record") == 0);
        CHECK(cfg(64, 48, 70, 52, &good, nullptr) != 0);
        CHECK(cfg(0, 48, 70, 52, &good, &good) != 0 && strcmp(msg, "nrs_front_rectify_configure: raw size 0 x 48 (1 .. 16384 each)") == 0);
        CHECK(cfg(64, -1, 70, 52, &good, &good) != 0 && cfg(RECT_MAX_SIZE + 1, 48, 70, 52, &good, &good) != 0 && cfg(64, RECT_MAX_SIZE + 1, 70, 52, &good, &good) != 0);
        CHECK(cfg(64, 48, 0, 52, &good, &good) != 0 && cfg(64, 48, 70, 0, &good, &good) != 0 && cfg(64, 48, RECT_MAX_SIZE + 1, 52, &good, &good) != 0);
        CHECK(cfg(64, 48, 70, RECT_MAX_SIZE + 1, &good, &good) != 0 && strcmp(msg, "nrs_front_rectify_configure: rectified size 70 x 16385 (1 .. 16384 each)") == 0);
        for (double bad : {inf, -inf, nan})
            for (int field = 0; field < 4; ++field)
                for (int side = 0; side < 2; ++side) {
                    nrs_rect_eye e = good;
                    (field == 0 ? e.K[2] : field == 1 ? e.dist[7] : field == 2 ? e.R[4] : e.P[8]) = bad;
                    CHECK(cfg(64, 48, 70, 52, side ? &good : &e, side ? &e : &good) != 0 && strstr(msg, "is not finite") && strstr(msg, side ? "right eye" : "left eye"));
                }
        nrs_rect_eye flat = good;
        flat.P[8] = 0; flat.P[2] = 0; flat.P[5] = 0;                                          // a P without a third column
        CHECK(cfg(64, 48, 70, 52, &flat, &good) != 0 && strstr(msg, "left eye: det(P R) is 0"));
        memset(flat.R, 0, sizeof flat.R);
        CHECK(cfg(64, 48, 70, 52, &good, &flat) != 0 && strstr(msg, "right eye: det(P R)"));
        // the raw call's own checks
        CHECK(rect_check_raw(false, 0, 0, 64, 48, msg, sizeof msg) == -2 && strstr(msg, "no rectification has been configured"));
        CHECK(rect_check_raw(true, 64, 48, 64, 48, msg, sizeof msg) == 0);
        CHECK(rect_check_raw(true, 64, 48, 70, 48, msg, sizeof msg) == -1 && strcmp(msg, "nrs_front_process_stereo_raw: the raw eyes are 70 x 48, the configured ones 64 x 48") == 0);
        CHECK(rect_check_raw(true, 64, 48, 64, 52, msg, sizeof msg) == -1);
    }
    // ---- P R and the inverse, in the stated order: a product with known entries, the inverse of a camera matrix
    {
        const double P[9] = {2, 0, 3, 0, 4, 5, 0, 0, 1}, R[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
        double M[9], I[9];
        rect_mul3(P, R, M);
        const double want[9] = {0, -2, 3, 4, 0, 5, 0, 0, 1};
        for (int i = 0; i < 9; ++i) CHECK(M[i] == want[i]);
        CHECK(rect_inv3(M, I) == 8.0);
        const double winv[9] = {0, 0.25, -1.25, -0.5, 0, 1.5, 0, 0, 1};
        for (int i = 0; i < 9; ++i) CHECK(I[i] == winv[i]);
        const double Z[9] = {1, 2, 3, 2, 4, 6, 0, 1, 0};
        I[0] = 77;
        CHECK(rect_inv3(Z, I) == 0.0 && I[0] == 77);                                            // singular: nothing is written
    }
    // ---- the identity: K = P, R = I, no distortion, powers of two: the map is (u, v) to the last bit, every fraction 0
    {
        const nrs_rect_eye l = make_eye(64, 32, 24), r = make_eye(128, 16, 8);
        CHECK(rect_check_configure(64, 48, 64, 48, &l, &r, out, msg, sizeof msg) == 0);
        for (int e = 0; e < 2; ++e)
            for (int v = 0; v < 48; ++v)
                for (int u = 0; u < 64; ++u) {
                    float mx, my;
                    rect_map_px(out[e], u, v, &mx, &my);
                    const RectTap t = rect_fix(mx, my);
                    CHECK(mx == (float)u && my == (float)v && t.ix == u && t.iy == v && t.frac == 0 && t.pad == 0);
                }
    }
    // ---- the weights: exact integers, their sum is 2^15 at every fraction index
    for (int frac = 0; frac < RECT_TAB * RECT_TAB; ++frac) {
        int w[4];
        rect_weights(frac, w);
        const int fx = frac % 32, fy = frac / 32;
        CHECK(w[0] + w[1] + w[2] + w[3] == 1 << RECT_ONE_BITS && w[0] >= 0 && w[1] >= 0 && w[2] >= 0 && w[3] >= 0);
        CHECK(w[0] == (32 - fx) * (32 - fy) * 32 && w[1] == fx * (32 - fy) * 32 && w[2] == (32 - fx) * fy * 32 && w[3] == fx * fy * 32);
    }
    // ---- rounding half to even, the arithmetic shift, saturation to int16, the non-finite rule
    {
        RectTap t = rect_fix(5.f + 1.f / 64, 7.f + 3.f / 64);                                   // .5 -> 0 (even), 1.5 -> 2
        CHECK(t.ix == 5 && t.iy == 7 && t.frac == 2 * 32 + 0);
        t = rect_fix(5.f + 5.f / 64, 7.f + 7.f / 64);                                           // 2.5 -> 2, 3.5 -> 4
        CHECK(t.ix == 5 && t.iy == 7 && t.frac == 4 * 32 + 2);
        t = rect_fix(-1.f / 64, -3.f / 64);                                                     // -.5 -> -0: pixel 0; -1.5 -> -2: pixel -1, fraction 30
        CHECK(t.ix == 0 && t.iy == -1 && t.frac == 30 * 32 + 0);
        t = rect_fix(-0.25f, 47.96875f);
        CHECK(t.ix == -1 && t.iy == 47 && t.frac == 31 * 32 + 24);
        t = rect_fix(32767.f, -32768.f);
        CHECK(t.ix == 32767 && t.iy == -32768 && t.frac == 0);
        t = rect_fix(32768.5f, -32769.25f);                                                     // one past either end
        CHECK(t.ix == 32767 && t.iy == -32768);
        t = rect_fix(1e9f, -1e9f);                                                              // far past: the product is clamped before it becomes an integer
        CHECK(t.ix == 32767 && t.iy == -32768);
        t = rect_fix(3e38f, -3e38f);                                                            // the fp32 product overflows to an infinity
        CHECK(t.ix == 32767 && t.iy == -32768);
        const float finf = std::numeric_limits<float>::infinity(), fnan = std::numeric_limits<float>::quiet_NaN();
        const uint8_t img[4] = {255, 255, 255, 255};
        for (float bad : {finf, -finf, fnan})
            for (int axis = 0; axis < 2; ++axis) {
                t = axis ? rect_fix(0.5f, bad) : rect_fix(bad, 0.5f);
                CHECK(t.ix == -32768 && t.iy == -32768 && t.frac == 0 && t.pad == 0);
                int px = -1;
                rect_sample_px<1>(img, 2, 2, 2, t, &px);
                CHECK(px == 0);
            }
        int px = -1;
        rect_sample_px<1>(img, 2, 2, 2, rect_fix(0.5f, 0.5f), &px);                             // (the same image does give 255 inside)
        CHECK(px == 255);
        rect_sample_px<1>(img, 2, 2, 2, rect_fix(-0.5f, 0.f), &px);                             // half of the weight outside: (255 * 16384 + 2^14) >> 15
        CHECK(px == 128);
        rect_sample_px<1>(img, 2, 2, 2, rect_fix(32767.f, 0.f), &px);
        CHECK(px == 0);
    }
    // ---- a tiny remap: rotation, all eight coefficients, 5 x 4 -> 6 x 5, rows padded; maps and bytes from tests/rect_oracle.py
    {
        nrs_rect_eye e = make_eye(1, 0, 0);
        const double K[9] = {3.5, 0, 2.2, 0, 3.25, 1.6, 0, 0, 1}, P[9] = {4, 0, 2, 0, 4, 1.5, 0, 0, 1};
        const double R[9] = {0.9942082680739207, -0.10169729973082767, -0.03475023627133056, 0.09975356056184054, 0.9935611387343747,
                             -0.05371676416248484, 0.03998933418663416, 0.04993919126608886, 0.9979513667143298};
        const double dist[8] = {-0.2, 0.05, 0.01, -0.02, 0.003, 0.04, -0.01, 0.002};
        memcpy(e.K, K, sizeof K); memcpy(e.P, P, sizeof P); memcpy(e.R, R, sizeof R); memcpy(e.dist, dist, sizeof dist);
        CHECK(rect_check_configure(5, 4, 6, 5, &e, &e, out, msg, sizeof msg) == 0);
        const double iR[9] = {0.24855206701848018, 0.024938390140460134, -0.49452238506101637, -0.025424324932706903, 0.2483902846835936,
                              -0.27179758589388775, -0.00868755906783264, -0.013429191040621206, 1.0354702714109267};
        for (int i = 0; i < 9; ++i) CHECK(out[0].iR[i] == iR[i] && out[1].iR[i] == iR[i]);
        const uint32_t mx[30] = {0x3f17f3b5u, 0x3fb018a6u, 0x400ce6afu, 0x40407cecu, 0x406e8efau, 0x408a3a5fu, 0x3f1fff72u, 0x3fb7d497u, 0x4012e214u, 0x40486d24u,
                                 0x4077dc63u, 0x408f1ce7u, 0x3f309f5bu, 0x3fc19d96u, 0x40186ceeu, 0x404e68c5u, 0x407dfe64u, 0x40922871u, 0x3f488ea2u, 0x3fcc9ec2u,
                                 0x401cfcb5u, 0x4051cf77u, 0x40802ebeu, 0x40933102u, 0x3f640201u, 0x3fd77550u, 0x402026aeu, 0x405292d8u, 0x407f71ceu, 0x4092da16u};
        const uint32_t my[30] = {0x3f4ce73eu, 0x3f30da0cu, 0x3f1aa28cu, 0x3f0cd86eu, 0x3f089854u, 0x3f0c905bu, 0x3fc46fceu, 0x3fb90ad6u, 0x3fae3428u, 0x3fa4eafbu,
                                 0x3f9e0934u, 0x3f99dd66u, 0x4013cd2au, 0x400fcd9cu, 0x400ac4d5u, 0x4004fb1du, 0x3ffdf97bu, 0x3ff2e5d6u, 0x40444b34u, 0x4041dc0fu,
                                 0x403d3da9u, 0x40367a64u, 0x402e3f2cu, 0x4025c469u, 0x4070c935u, 0x406f2a60u, 0x406abdf1u, 0x406356c2u, 0x4059d01cu, 0x40500d1eu};
        const int o3[90] = {107, 160, 213, 124, 177, 164, 146, 170, 100, 173, 82, 135, 197, 114, 81, 145, 82, 41, 173, 141, 143, 146, 136, 126, 125, 133, 71, 171, 40, 93,
                            204, 65, 118, 116, 34, 62, 167, 99, 97, 111, 68, 121, 39, 92, 145, 62, 115, 164, 89, 134, 187, 44, 57, 80, 53, 103, 153, 84, 136, 187,
                            115, 168, 221, 135, 188, 180, 150, 203, 72, 56, 78, 38, 15, 29, 42, 23, 36, 49, 41, 60, 78, 65, 89, 80, 105, 136, 15, 54, 70, 8};
        const int o1[30] = {107, 124, 146, 173, 197, 145, 173, 146, 125, 171, 204, 116, 167, 111, 39, 62, 89, 44, 53, 84, 115, 135, 150, 56, 15, 23, 41, 65, 105, 54};
        const int stride3 = 5 * 3 + 4, stride1 = 5 + 3;                                         // padding of 0xEE that no tap may read
        std::vector<uint8_t> s3((size_t)stride3 * 4, 0xEE), s1((size_t)stride1 * 4, 0xEE);
        for (int y = 0; y < 4; ++y)
            for (int x = 0; x < 5; ++x) {
                for (int c = 0; c < 3; ++c) s3[(size_t)y * stride3 + x * 3 + c] = (uint8_t)((x * 37 + y * 91 + c * 53 + 11) & 255);
                s1[(size_t)y * stride1 + x] = (uint8_t)((x * 37 + y * 91 + 11) & 255);
            }
        for (int v = 0; v < 5; ++v)
            for (int u = 0; u < 6; ++u) {
                float fx, fy;
                rect_map_px(out[0], u, v, &fx, &fy);
                CHECK(bits(fx) == mx[v * 6 + u] && bits(fy) == my[v * 6 + u]);
                const RectTap t = rect_fix(fx, fy);
                int p3[3], p1;
                rect_sample_px<3>(s3.data(), stride3, 5, 4, t, p3);
                rect_sample_px<1>(s1.data(), stride1, 5, 4, t, &p1);
                for (int c = 0; c < 3; ++c) CHECK(p3[c] == o3[(v * 6 + u) * 3 + c]);
                CHECK(p1 == o1[v * 6 + u]);
            }
    }
    printf(fails ? "rect_check: %d check(s) FAILED\n" : "rect_check OK\n", fails);
    return fails ? 1 : 0;
}
