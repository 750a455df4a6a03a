// Stand-alone check of the host half of nrs_dbscan3d / nrs_init_stereo (csrc/nrs_sinit_host.hpp) under AddressSanitizer + UBSan:
// `make sinit_check` (builds and runs it).  No HIP, no library: hand-made buffers, every array exactly as long as the interface says.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../csrc/nrs_sinit_host.hpp"

using namespace nrs;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

int main() {
    char msg[256];
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- nrs_dbscan3d's checks
    {
        float xyz[6] = {0, 0, 0, 1, 1, 1};
        int32_t label[2], counts[3];
        CHECK(dbscan_check_args(2, xyz, 2.5, 5, label, counts, msg, sizeof msg) == 0);
        CHECK(dbscan_check_args(0, nullptr, 2.5, 5, nullptr, counts, msg, sizeof msg) == 0);           // an empty set is a valid call
        CHECK(dbscan_check_args(-1, xyz, 2.5, 5, label, counts, msg, sizeof msg) != 0 && strstr(msg, "n = -1"));
        CHECK(dbscan_check_args(SINIT_MAX, xyz, 2.5, 5, label, counts, msg, sizeof msg) == 0);         // (refusals read no array)
        CHECK(dbscan_check_args(SINIT_MAX + 1, xyz, 2.5, 5, label, counts, msg, sizeof msg) != 0 && strstr(msg, "16384"));
        CHECK(dbscan_check_args(2, nullptr, 2.5, 5, label, counts, msg, sizeof msg) != 0 && strstr(msg, "null pointer"));
        CHECK(dbscan_check_args(2, xyz, 2.5, 5, nullptr, counts, msg, sizeof msg) != 0);
        CHECK(dbscan_check_args(2, xyz, 2.5, 5, label, nullptr, msg, sizeof msg) != 0);
        for (double e : {0.0, -1.0, inf, -inf, nan}) CHECK(dbscan_check_args(2, xyz, e, 5, label, counts, msg, sizeof msg) != 0 && strstr(msg, "eps"));
        CHECK(dbscan_check_args(2, xyz, 2.5, 0, label, counts, msg, sizeof msg) != 0 && strstr(msg, "min_points = 0"));
        CHECK(dbscan_check_args(2, xyz, 2.5, 1, label, counts, msg, sizeof msg) == 0);
    }
    // ---- the defaults (tracking.cc:226-233, dbscan.cc:63) and nrs_init_stereo's own checks
    nrs_init_stereo_options o;
    sinit_options_init(&o);
    CHECK(o.struct_size == sizeof o && o.bf == 3886.37f && o.z_min == 35.5f && o.z_max == 70.5f && o.eps == 2.5 && o.min_points == 5 && o.noise_competes == 1);
    nrs_init_stereo_result r;
    memset(&r, 0, sizeof r);
    r.struct_size = (uint32_t)sizeof r;
    CHECK(sinit_check_args(&o, &r, 100, msg, sizeof msg) == 0);
    CHECK(sinit_check_args(&o, &r, 0, msg, sizeof msg) == 0);
    CHECK(sinit_check_args(&o, &r, SINIT_MAX, msg, sizeof msg) == 0);
    CHECK(sinit_check_args(nullptr, &r, 1, msg, sizeof msg) != 0 && strstr(msg, "null pointer"));
    CHECK(sinit_check_args(&o, nullptr, 1, msg, sizeof msg) != 0);
    CHECK(sinit_check_args(&o, &r, SINIT_MAX + 1, msg, sizeof msg) != 0 && strstr(msg, "16385"));
    { auto b = o; b.struct_size = 0; CHECK(sinit_check_args(&b, &r, 1, msg, sizeof msg) != 0 && strstr(msg, "options struct_size 0")); }
    { auto b = o; b.struct_size += 4; CHECK(sinit_check_args(&b, &r, 1, msg, sizeof msg) != 0); }
    { auto b = r; b.struct_size -= 8; CHECK(sinit_check_args(&o, &b, 1, msg, sizeof msg) != 0 && strstr(msg, "result struct_size")); }
    for (double e : {0.0, -2.5, inf, nan}) { auto b = o; b.eps = e; CHECK(sinit_check_args(&b, &r, 1, msg, sizeof msg) != 0 && strstr(msg, "eps")); }
    { auto b = o; b.min_points = 0; CHECK(sinit_check_args(&b, &r, 1, msg, sizeof msg) != 0 && strstr(msg, "min_points")); }
    { auto b = o; b.z_min = b.z_max; CHECK(sinit_check_args(&b, &r, 1, msg, sizeof msg) != 0 && strstr(msg, "gate")); }
    { auto b = o; b.z_min = 80.f; CHECK(sinit_check_args(&b, &r, 1, msg, sizeof msg) != 0); }
    { auto b = o; b.z_max = (float)nan; CHECK(sinit_check_args(&b, &r, 1, msg, sizeof msg) != 0); }
    { auto b = o; b.z_min = (float)nan; CHECK(sinit_check_args(&b, &r, 1, msg, sizeof msg) != 0); }
    // ---- the upload: rows taken at their stride, the gaps zeroed, every byte written
    {
        const size_t w = 5, h = 3, n = 2, sl = 7, sr = 5;
        std::vector<uint8_t> left(sl * (h - 1) + w), right(sr * (h - 1) + w);                          // the last row ends at its w-th byte
        for (size_t i = 0; i < left.size(); ++i) left[i] = (uint8_t)(i + 1);
        for (size_t i = 0; i < right.size(); ++i) right[i] = (uint8_t)(100 + i);
        const float xy[4] = {1.5f, 2.5f, 3.5f, 4.5f};
        const SinitUpload U(w, h, n);
        CHECK(U.left == 0 && U.right == 256 && U.xy == 512 && U.bytes == 512 + 16);
        std::vector<char> buf(U.bytes, (char)0x5A);
        sinit_pack_upload(U, left.data(), sl, right.data(), sr, xy, buf.data());
        for (size_t y = 0; y < h; ++y)
            for (size_t x = 0; x < w; ++x) {
                CHECK((uint8_t)buf[U.left + y * w + x] == left[y * sl + x]);
                CHECK((uint8_t)buf[U.right + y * w + x] == right[y * sr + x]);
            }
        for (size_t i = w * h; i < 256; ++i) CHECK(buf[U.left + i] == 0 && buf[U.right + i] == 0);
        CHECK(memcmp(buf.data() + U.xy, xy, 16) == 0);
        const SinitUpload U2(16, 16, 0);                                                               // an image that fills its piece: no gap
        CHECK(U2.right == 256 && U2.bytes == 512);
        std::vector<uint8_t> im(256, 9);
        std::vector<char> buf2(U2.bytes, (char)0x5A);
        sinit_pack_upload(U2, im.data(), 16, im.data(), 16, nullptr, buf2.data());
        for (char ch : buf2) CHECK(ch == 9);
    }
    // ---- the median: nth_element at n / 2 (the upper median of an even count)
    {
        const float nanf_ = std::numeric_limits<float>::quiet_NaN();
        std::vector<float> p = {0, 0, 5.f, 0, 0, 1.f, 0, 0, 4.f, 0, 0, 2.f};
        CHECK(sinit_median_depth(p.data(), 4) == 4.f);
        CHECK(sinit_median_depth(p.data(), 3) == 4.f);
        CHECK(sinit_median_depth(p.data(), 1) == 5.f);
        CHECK(std::isnan(sinit_median_depth(nullptr, 0)));
        (void)nanf_;
    }
    // ---- the layout and the unpacking, arrays of exactly n (x 3) entries, every output pointer optional
    for (int n : {0, 1, 5, 65}) {
        const SinitLayout L((size_t)n);
        CHECK(L.words == (size_t)SINIT_HDR + 11 * (size_t)n);              // two arrays of 3n floats, five of n words
        std::vector<int32_t> pk(L.words);
        for (size_t i = 0; i < L.words; ++i) pk[i] = (int32_t)(1000 + i);
        float* pf = reinterpret_cast<float*>(pk.data());
        const int n_gated = n - n / 3, n_sel = n_gated / 2;
        for (int i = 0; i < n_sel; ++i) pf[L.sel_xyz + 3 * (size_t)i + 2] = 40.f + (float)((i * 7) % n_sel);
        pk[0] = n; pk[1] = n_gated; pk[2] = n_gated / 4; pk[3] = n_gated / 5; pk[4] = n_sel; pk[5] = n_sel;
        std::vector<float> xyz(3 * n), sxyz(3 * n);
        std::vector<int32_t> st(n), code(n), raw(n), lab(n), sel(n);
        nrs_init_stereo_result out;
        memset(&out, 0, sizeof out);
        out.struct_size = (uint32_t)sizeof out;
        out.xyz = xyz.data(); out.match_status = st.data(); out.code = code.data(); out.raw_label = raw.data(); out.label = lab.data();
        out.selected = sel.data(); out.selected_xyz = sxyz.data();
        CHECK(sinit_unpack(pk.data(), n, &out) == 0);
        CHECK(out.n_matched == n && out.n_gated == n_gated && out.n_clusters == n_gated / 4 && out.n_noise == n_gated / 5 && out.n_selected == n_sel);
        CHECK(out.verdict == (n_gated == 0 ? 1 : 0));
        if (n_sel) CHECK(out.median_depth == 40.f + (float)(n_sel / 2)); else CHECK(std::isnan(out.median_depth));
        if (n) {
            CHECK(memcmp(xyz.data(), &pk[L.xyz], 12 * (size_t)n) == 0 && memcmp(st.data(), &pk[L.status], 4 * (size_t)n) == 0);
            CHECK(memcmp(code.data(), &pk[L.code], 4 * (size_t)n) == 0 && memcmp(raw.data(), &pk[L.raw], 4 * (size_t)n) == 0);
            CHECK(memcmp(lab.data(), &pk[L.label], 4 * (size_t)n) == 0);
        }
        if (n_sel) CHECK(memcmp(sel.data(), &pk[L.selected], 4 * (size_t)n_sel) == 0 && memcmp(sxyz.data(), &pk[L.sel_xyz], 12 * (size_t)n_sel) == 0);
        nrs_init_stereo_result bare;                                   // no arrays wanted: the scalars alone
        memset(&bare, 0, sizeof bare);
        bare.struct_size = (uint32_t)sizeof bare;
        CHECK(sinit_unpack(pk.data(), n, &bare) == 0 && bare.n_selected == n_sel);
        // headers that contradict themselves: refused, nothing copied
        const int32_t keep[6] = {pk[0], pk[1], pk[2], pk[3], pk[4], pk[5]};
        auto bad = [&](int k, int32_t v) { pk[k] = v; CHECK(sinit_unpack(pk.data(), n, &out) != 0); pk[k] = keep[k]; };
        bad(0, n + 1); bad(0, -1); bad(1, n + 1); bad(2, n_gated + 1); bad(3, n_gated + 1); bad(4, n_gated + 1); bad(5, n_sel + 1); bad(3, -1);
    }
    {
        nrs_init_stereo_result c;
        memset(&c, 0x5A, sizeof c);
        sinit_clear(&c);
        CHECK(c.verdict == 1 && c.n_matched == 0 && c.n_gated == 0 && c.n_clusters == 0 && c.n_noise == 0 && c.n_selected == 0 && std::isnan(c.median_depth));
    }
    printf(fails ? "sinit_check: %d check(s) FAILED\n" : "sinit_check OK\n", fails);
    return fails ? 1 : 0;
}
