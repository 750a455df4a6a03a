// Stand-alone check of the host half of the frame resize (csrc/nrs_resize_host.hpp) under AddressSanitizer + UBSan: `make resize_check`
// (builds and runs it).  No HIP, no library.  The tables built here are the ones the library uploads, and the two pixel bodies checked here
// -- the fixed-point blend and the 2 x 2 box -- are the ones the kernel of nrs_front.hip runs.  The expected values of the tiny resizes at
// the end come from tests/resize_oracle.py.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../csrc/nrs_resize_host.hpp"

using namespace nrs;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

struct Taps {
    std::vector<int32_t> sx, sy;
    std::vector<int16_t> ax, by;
    Taps(int sw, int sh, int dw, int dh) : sx((size_t)dw), sy(2 * (size_t)dh), ax(2 * (size_t)dw), by(2 * (size_t)dh) {      // (exact sizes: ASan sees any overrun)
        resize_build_taps(sw, sh, dw, dh, sx.data(), ax.data(), sy.data(), by.data());
    }
};

int main() {
    char msg[256];
    // ---- the refusals
    {
        CHECK(resize_check_configure(1440, 1080, 720, 540, msg, sizeof msg) == 0);
        CHECK(resize_check_configure(1, 1, RESIZE_MAX_SIZE, RESIZE_MAX_SIZE, msg, sizeof msg) == 0 && resize_check_configure(RESIZE_MAX_SIZE, RESIZE_MAX_SIZE, 1, 1, msg, sizeof msg) == 0);
        CHECK(resize_check_configure(0, 48, 32, 24, msg, sizeof msg) != 0 && strcmp(msg, "nrs_front_resize_configure: raw size 0 x 48 (1 .. 16384 each)") == 0);
        CHECK(resize_check_configure(64, -1, 32, 24, msg, sizeof msg) != 0 && resize_check_configure(RESIZE_MAX_SIZE + 1, 48, 32, 24, msg, sizeof msg) != 0);
        CHECK(resize_check_configure(64, RESIZE_MAX_SIZE + 1, 32, 24, msg, sizeof msg) != 0);
        CHECK(resize_check_configure(1, 1, 0, 0, msg, sizeof msg) != 0 && strcmp(msg, "nrs_front_resize_configure: resized size 0 x 0 (1 .. 16384 each)") == 0);      // half_size(1, 1)
        CHECK(resize_check_configure(64, 48, 32, 0, msg, sizeof msg) != 0 && resize_check_configure(64, 48, RESIZE_MAX_SIZE + 1, 24, msg, sizeof msg) != 0);
        CHECK(resize_check_configure(64, 48, 32, RESIZE_MAX_SIZE + 1, msg, sizeof msg) != 0 && strcmp(msg, "nrs_front_resize_configure: resized size 32 x 16385 (1 .. 16384 each)") == 0);
        CHECK(resize_check_raw(false, 0, 0, 64, 48, msg, sizeof msg) == -2 && strstr(msg, "no resize has been configured"));
        CHECK(resize_check_raw(true, 64, 48, 64, 48, msg, sizeof msg) == 0);
        CHECK(resize_check_raw(true, 64, 48, 32, 24, msg, sizeof msg) == -1 && strcmp(msg, "nrs_front_process_raw: the raw frame is 32 x 24, the configured one 64 x 48") == 0);
        CHECK(resize_check_raw(true, 64, 48, 64, 47, msg, sizeof msg) == -1);
    }
    // ---- the box test: exactly halved in BOTH directions
    CHECK(resize_is_box(64, 48, 32, 24) && resize_is_box(2, 2, 1, 1) && resize_is_box(1440, 1080, 720, 540) && resize_is_box(530, 70, 265, 35));
    CHECK(!resize_is_box(66, 29, 33, 14) && !resize_is_box(29, 66, 14, 33) && !resize_is_box(37, 29, 18, 14) && !resize_is_box(40, 30, 40, 30) && !resize_is_box(32, 24, 64, 48));
    CHECK(!resize_is_box(1441, 1081, 720, 540) && !resize_is_box(1, 1, 5, 4));
    // ---- the tap rule
    {
        Taps id(40, 30, 40, 30);                                                                // scale 1: (x, 2048, 0)
        for (int x = 0; x < 40; ++x) CHECK(id.sx[x] == x && id.ax[2 * x] == 2048 && id.ax[2 * x + 1] == 0);
        for (int y = 0; y < 30; ++y) CHECK(id.sy[2 * y] == y && id.sy[2 * y + 1] == (y < 29 ? y + 1 : 29) && id.by[2 * y] == 2048 && id.by[2 * y + 1] == 0);
        Taps half(37, 29, 18, 14);                                                              // half_size of an odd frame: two taps to the last column
        CHECK(half.sx[0] == 0 && half.ax[0] == 967 && half.ax[1] == 1081 && half.sx[17] == 35 && half.ax[34] == 1081 && half.ax[35] == 967);
        Taps up(20, 12, 45, 31);
        CHECK(up.sx[0] == 0 && up.ax[0] == 2048 && up.ax[1] == 0);                              // sx = -1: index and fraction zeroed
        CHECK(up.sx[1] == 0 && up.ax[2] == 1707 && up.ax[3] == 341);
        CHECK(up.sx[43] == 18 && up.ax[86] == 341 && up.ax[87] == 1707);
        CHECK(up.sx[44] == 19 && up.ax[88] == 2048 && up.ax[89] == 0);                          // the last source column: one tap
        CHECK(up.sy[0] == 0 && up.sy[1] == 0 && up.by[0] == 628 && up.by[1] == 1420);           // sy = -1: the fraction STAYS, both rows clamp to row 0
        CHECK(up.sy[60] == 11 && up.sy[61] == 11 && up.by[60] == 1420 && up.by[61] == 628);     // and both to the last row
        Taps one(1, 1, 5, 4);
        for (int x = 0; x < 5; ++x) CHECK(one.sx[x] == 0 && one.ax[2 * x] == 2048 && one.ax[2 * x + 1] == 0);
        for (int y = 0; y < 4; ++y) CHECK(one.sy[2 * y] == 0 && one.sy[2 * y + 1] == 0 && one.by[2 * y] + one.by[2 * y + 1] == 2048);
        CHECK(one.by[0] == 768 && one.by[1] == 1280);
        Taps ties(1023, 1023, 2048, 2048);                                                      // every product ends in .5: half to even, each weight on its own
        CHECK(ties.by[0] == 512 && ties.by[1] == 1536 && ties.ax[2] == 1538 && ties.ax[3] == 510 && ties.ax[4] == 514 && ties.ax[5] == 1534);
        for (int x = 1; x < 2047; ++x) CHECK(ties.ax[2 * x] + ties.ax[2 * x + 1] == 2048 && (ties.ax[2 * x] & 1) == 0);
        // what the kernel relies on, over many pairs of sizes: indices inside the source, a second column tap wherever it carries weight,
        // non-negative weights that sum to 2^11
        const int sizes[] = {1, 2, 3, 5, 8, 17, 37, 64, 100, 255, 256, 257, 531, 720, 1440, 1441, 4097, RESIZE_MAX_SIZE};
        for (int s : sizes)
            for (int d : sizes) {
                Taps t(s, s, d, d);
                for (int i = 0; i < d; ++i) {
                    CHECK(t.sx[i] >= 0 && t.sx[i] <= s - 1 && (t.ax[2 * i + 1] == 0 || t.sx[i] + 1 <= s - 1));
                    CHECK(t.ax[2 * i] >= 0 && t.ax[2 * i + 1] >= 0 && t.ax[2 * i] + t.ax[2 * i + 1] == 1 << RESIZE_COEF_BITS);
                    CHECK(t.sy[2 * i] >= 0 && t.sy[2 * i] <= t.sy[2 * i + 1] && t.sy[2 * i + 1] <= s - 1 && t.sy[2 * i + 1] - t.sy[2 * i] <= 1);
                    CHECK(t.by[2 * i] >= 0 && t.by[2 * i + 1] >= 0 && t.by[2 * i] + t.by[2 * i + 1] == 1 << RESIZE_COEF_BITS);
                }
            }
    }
    // ---- the pixel bodies
    {
        CHECK(resize_box(0, 0, 0, 0) == 0 && resize_box(255, 255, 255, 255) == 255 && resize_box(255, 0, 0, 255) == 128);      // the checkerboard: 510 + 2 >> 2
        CHECK(resize_box(1, 1, 0, 0) == 1 && resize_box(1, 0, 0, 0) == 0 && resize_box(1, 1, 1, 0) == 1);                      // a sum of 2 mod 4 rounds up
        CHECK(resize_blend(255, 255, 255, 255, 2048, 0, 2048, 0) == 255 && resize_blend(255, 255, 255, 255, 1024, 1024, 1024, 1024) == 255);
        CHECK(resize_blend(7, 99, 99, 99, 2048, 0, 2048, 0) == 7 && resize_blend(0, 0, 0, 0, 967, 1081, 628, 1420) == 0);
        // two weights on ONE row are not one whole weight: 77 through (628, 1420) truncates twice
        CHECK(resize_blend(77, 77, 77, 77, 2048, 0, 2048, 0) == 77 && (((628 * ((77 * 2048) >> 4)) >> 16) + ((1420 * ((77 * 2048) >> 4)) >> 16)) == 4 * 77 - 1);
        int differ = 0;
        for (int v = 0; v < 256; ++v) {                                                        // ... and behind a column blend that costs a grey level
            const int w = 255 - v, d = v * 878 + w * 1170, whole = (((2048 * (d >> 4)) >> 16) + 2) >> 2, split = resize_blend(v, w, v, w, 878, 1170, 628, 1420);
            CHECK(split == whole || split == whole - 1);
            differ += split != whole;
        }
        CHECK(differ > 0);
        // exactly halved, the general rule has weights (1024, 1024) on both axes and gives the box's bytes: the branch saves the tables
        for (int a = 0; a < 256; a += 5)
            for (int b = 0; b < 256; b += 7)
                for (int c2 = 0; c2 < 256; c2 += 51)
                    for (int d = 0; d < 256; d += 85) CHECK(resize_blend(a, b, c2, d, 1024, 1024, 1024, 1024) == resize_box(a, b, c2, d));
        CHECK(resize_sat8(-1) == 0 && resize_sat8(256) == 255 && resize_sat8(255) == 255 && resize_sat16(40000) == 32767 && resize_sat16(-40000) == -32768);
    }
    // ---- tiny resizes, rows padded with 0xEE that no tap may read; bytes from tests/resize_oracle.py
    {
        const int o3[63] = {26, 79, 132, 47, 100, 153, 74, 126, 167, 100, 153, 163, 126, 149, 190, 153, 163, 125, 174, 184, 24,
                            148, 201, 126, 169, 148, 147, 158, 120, 136, 94, 147, 72, 120, 81, 98, 146, 71, 124, 168, 93, 146,
                            55, 108, 119, 76, 105, 140, 91, 113, 166, 87, 140, 193, 113, 166, 219, 140, 192, 154, 161, 214, 53};
        const int o1[21] = {26, 47, 74, 100, 126, 153, 174, 148, 169, 158, 94, 120, 146, 168, 55, 76, 91, 87, 113, 140, 161};
        const int stride3 = 5 * 3 + 4, stride1 = 5 + 3;
        std::vector<uint8_t> s3((size_t)stride3 * 4, 0xEE), s1((size_t)stride1 * 4, 0xEE);
        for (int y = 0; y < 4; ++y)
            for (int x = 0; x < 5; ++x) {
                for (int c = 0; c < 3; ++c) s3[(size_t)y * stride3 + x * 3 + c] = (uint8_t)((x * 37 + y * 91 + c * 53 + 11) & 255);
                s1[(size_t)y * stride1 + x] = (uint8_t)((x * 37 + y * 91 + 11) & 255);
            }
        Taps t(5, 4, 7, 3);                                                                     // 5 x 4 -> 7 x 3: up in x, down in y
        const int sx[7] = {0, 0, 1, 2, 2, 3, 4}, ax[14] = {2048, 0, 878, 1170, 1463, 585, 2048, 0, 585, 1463, 1170, 878, 2048, 0};
        const int sy[6] = {0, 1, 1, 2, 2, 3}, by[6] = {1707, 341, 1024, 1024, 341, 1707};
        for (int i = 0; i < 7; ++i) CHECK(t.sx[i] == sx[i] && t.ax[2 * i] == ax[2 * i] && t.ax[2 * i + 1] == ax[2 * i + 1]);
        for (int i = 0; i < 6; ++i) CHECK(t.sy[i] == sy[i] && t.by[i] == by[i]);
        for (int y = 0; y < 3; ++y)
            for (int x = 0; x < 7; ++x) {
                int p3[3], p1;
                resize_sample_px<3>(s3.data(), stride3, t.sx[x], t.ax[2 * x], t.ax[2 * x + 1], t.sy[2 * y], t.sy[2 * y + 1], t.by[2 * y], t.by[2 * y + 1], p3);
                resize_sample_px<1>(s1.data(), stride1, t.sx[x], t.ax[2 * x], t.ax[2 * x + 1], t.sy[2 * y], t.sy[2 * y + 1], t.by[2 * y], t.by[2 * y + 1], &p1);
                for (int c = 0; c < 3; ++c) CHECK(p3[c] == o3[(y * 7 + x) * 3 + c]);
                CHECK(p1 == o1[y * 7 + x]);
            }
        // 6 x 4 -> 3 x 2: the box branch, and the general rule on the same image
        const int ob[18] = {75, 128, 181, 149, 138, 127, 159, 148, 73, 129, 118, 107, 75, 128, 181, 149, 138, 127};
        const int strideb = 6 * 3 + 5;
        std::vector<uint8_t> b3((size_t)strideb * 4, 0xEE);
        for (int y = 0; y < 4; ++y)
            for (int x = 0; x < 6; ++x)
                for (int c = 0; c < 3; ++c) b3[(size_t)y * strideb + x * 3 + c] = (uint8_t)((x * 37 + y * 91 + c * 53 + 11) & 255);
        Taps g(6, 4, 3, 2);
        for (int y = 0; y < 2; ++y)
            for (int x = 0; x < 3; ++x) {
                int pb[3], pg[3];
                resize_box_px<3>(b3.data(), strideb, x, y, pb);
                resize_sample_px<3>(b3.data(), strideb, g.sx[x], g.ax[2 * x], g.ax[2 * x + 1], g.sy[2 * y], g.sy[2 * y + 1], g.by[2 * y], g.by[2 * y + 1], pg);
                for (int c = 0; c < 3; ++c) CHECK(pb[c] == ob[(y * 3 + x) * 3 + c] && pg[c] == pb[c]);
            }
    }
    printf(fails ? "resize_check: %d check(s) FAILED\n" : "resize_check OK\n", fails);
    return fails ? 1 : 0;
}
