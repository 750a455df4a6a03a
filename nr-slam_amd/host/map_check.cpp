// Stand-alone check of the host half of nrs_map_frame (csrc/nrs_map_host.hpp) under AddressSanitizer + UBSan:
// `make map_check` (builds and runs it).  No HIP, no library: hand-made buffers, every array exactly as long as the interface says.
#include <cstdio>
#include <limits>
#include <vector>
#include "../csrc/nrs_map_host.hpp"

using namespace nrs;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

int main() {
    const int F = 3, n = 5;
    std::vector<float> poses(7 * F, 0.f), kp(2 * F * n, 1.f), lm(3 * F * n, 0.f), mag(F, 0.001f);
    std::vector<uint8_t> has_kp(F * n, 1), has_lm(F * n, 1);
    std::vector<int32_t> status = {0, 1, 3, 1, 1};
    int cam = 0, dummy = 0;
    char msg[256];
    auto in = [&]() {
        MapIn a{&cam, 0, F, n, poses.data(), has_kp.data(), kp.data(), has_lm.data(), lm.data(), status.data(), mag.data(), 0.0013f, 0.004f, -1,
                {&dummy, &dummy, &dummy, &dummy, &dummy, &dummy, &dummy, &dummy, &dummy, &dummy}};
        return a;
    };
    int nc = -1;
    // ---- the checks
    MapIn a = in();
    CHECK(map_check_args(a, &nc, msg, sizeof msg) == 0 && nc == 3);
    a = in(); a.n_frames = MAP_MAXF + 1;
    CHECK(map_check_args(a, &nc, msg, sizeof msg) != 0 && strstr(msg, "at most 21"));
    a = in(); a.n_frames = 0;
    CHECK(map_check_args(a, &nc, msg, sizeof msg) != 0);
    a = in(); a.deform_mag = nullptr;
    CHECK(map_check_args(a, &nc, msg, sizeof msg) != 0);
    a = in(); a.outs[4] = nullptr;
    CHECK(map_check_args(a, &nc, msg, sizeof msg) != 0);
    a = in(); a.outs[9] = nullptr;
    CHECK(map_check_args(a, &nc, msg, sizeof msg) != 0);
    a = in(); a.cam_model = 5;
    CHECK(map_check_args(a, &nc, msg, sizeof msg) != 0 && strstr(msg, "camera model"));
    a = in(); a.rad_per_pixel = std::numeric_limits<float>::quiet_NaN();
    CHECK(map_check_args(a, &nc, msg, sizeof msg) != 0 && strstr(msg, "finite"));
    a = in(); a.rigidity_th = std::numeric_limits<float>::infinity();
    CHECK(map_check_args(a, &nc, msg, sizeof msg) != 0);
    a = in(); a.index_snapshot = F;
    CHECK(map_check_args(a, &nc, msg, sizeof msg) != 0 && strstr(msg, "index_snapshot"));
    a = in(); a.index_snapshot = F - 1;
    CHECK(map_check_args(a, &nc, msg, sizeof msg) == 0);
    has_kp[(F - 1) * n + 3] = 0;                                   // a TRACKED id without a keypoint in the last snapshot
    a = in();
    CHECK(map_check_args(a, &nc, msg, sizeof msg) != 0 && strstr(msg, "candidate 3"));
    has_kp[(F - 1) * n + 3] = 1;
    status.assign(n, 0);                                           // no candidates at all
    a = in();
    CHECK(map_check_args(a, &nc, msg, sizeof msg) == 0 && nc == 0);
    // ---- the packed layout and its unpacking, arrays of exactly n_cand (x 3) entries
    for (int ncand : {0, 1, 3, 65}) {
        const MapLayout L((size_t)ncand);
        CHECK(L.words == (size_t)MAP_HDR + 13 * (size_t)ncand);
        std::vector<int32_t> pk(L.words);
        for (size_t i = 0; i < L.words; ++i) pk[i] = (int32_t)(1000 + i);
        const int nacc = ncand / 2;
        pk[0] = ncand; pk[1] = 7; pk[2] = 9; pk[3] = MAP_MODE_RIGID; pk[4] = nacc;
        std::vector<int32_t> c(ncand), rs(ncand), ds(ncand), ai(nacc);
        std::vector<float> rx(3 * ncand), dx(3 * ncand), ax(3 * nacc);
        int32_t o_nc = -1, o_na = -1, counts[3] = {0, 0, 0};
        const MapOut out{&o_nc, c.data(), rs.data(), rx.data(), ds.data(), dx.data(), counts, &o_na, ai.data(), ax.data()};
        CHECK(map_unpack(pk.data(), ncand, out) == 0);
        CHECK(o_nc == ncand && o_na == nacc && counts[0] == 7 && counts[1] == 9 && counts[2] == MAP_MODE_RIGID);
        if (ncand) {
            CHECK(c[0] == pk[L.cand] && c[ncand - 1] == pk[L.cand + ncand - 1] && rs[0] == pk[L.r_st] && ds[ncand - 1] == pk[L.d_st + ncand - 1]);
            CHECK(memcmp(rx.data(), &pk[L.r_xyz], 12 * (size_t)ncand) == 0 && memcmp(dx.data(), &pk[L.d_xyz], 12 * (size_t)ncand) == 0);
        }
        if (nacc) CHECK(ai[nacc - 1] == pk[L.a_id + nacc - 1] && memcmp(ax.data(), &pk[L.a_xyz], 12 * (size_t)nacc) == 0);
        pk[4] = ncand + 1;                                         // a header that contradicts the count: refused, nothing copied
        CHECK(map_unpack(pk.data(), ncand, out) != 0);
        pk[4] = nacc; pk[0] = ncand + 1;
        CHECK(map_unpack(pk.data(), ncand, out) != 0);
        pk[0] = ncand; pk[3] = 3;
        CHECK(map_unpack(pk.data(), ncand, out) != 0);
    }
    printf(fails ? "map_check: %d check(s) FAILED\n" : "map_check OK\n", fails);
    return fails ? 1 : 0;
}
