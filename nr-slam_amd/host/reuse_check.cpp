// Stand-alone check of the host half of nrs_point_reuse (csrc/nrs_reuse_host.hpp) under AddressSanitizer + UBSan:
// `make reuse_check` (builds and runs it).  No HIP, no library: hand-made buffers, every array exactly as long as the interface says.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../csrc/nrs_reuse_host.hpp"

using namespace nrs;

static int fails = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } } while (0)

int main() {
    const int n = 6, ns = 4;
    std::vector<float> pos(3 * n, 1.f), qt = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    std::vector<int32_t> slot = {0, -1, 2, 3, -1, 1}, status = {0, 1, 2, 3}, lost = {5, 1, 5};
    int cam = 0, dummy = 0;
    char msg[256];
    auto in = [&]() {
        ReuseArgs a{&cam, 0, qt.data(), 96, 80, n, pos.data(), slot.data(), ns, status.data(), (int)lost.size(), lost.data(),
                    {&dummy, &dummy, &dummy, &dummy, &dummy, &dummy, &dummy, &dummy}};
        return a;
    };
    // ---- the checks
    ReuseArgs a = in();
    CHECK(reuse_check_args(a, msg, sizeof msg) == 0);
    a = in(); a.cam = nullptr;
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0 && strstr(msg, "null pointer"));
    a = in(); a.pose_qt = nullptr;
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0);
    for (int k = 0; k < 8; ++k) { a = in(); a.outs[k] = nullptr; CHECK(reuse_check_args(a, msg, sizeof msg) != 0 && strstr(msg, "null pointer")); }
    a = in(); a.cam_model = 7;
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0 && strstr(msg, "camera model 7"));
    a = in(); a.n_map = -1;
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0 && strstr(msg, "negative count"));
    a = in(); a.n_slots = -2;
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0);
    a = in(); a.n_lost = -1;
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0);
    a = in(); a.w = 0;
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0);
    a = in(); a.n_map = REUSE_MAX_MAP;                             // (refused before any array is read)
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0 && strstr(msg, "1048576"));
    a = in(); a.map_pos = nullptr;
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0);
    a = in(); a.frame_slot = nullptr;
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0);
    a = in(); a.slot_status = nullptr;
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0);
    a = in(); a.lost_ids = nullptr;
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0);
    slot[3] = ns;                                                  // a slot the frame does not have
    a = in();
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0 && strstr(msg, "frame_slot[3] = 4"));
    slot[3] = 3;
    lost[1] = n;
    a = in();
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0 && strstr(msg, "lost id 6"));
    lost[1] = -1;
    a = in();
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0 && strstr(msg, "lost id -1"));
    lost[1] = 1;
    a = in(); a.n_map = 0; a.n_lost = 0; a.map_pos = nullptr; a.frame_slot = nullptr; a.lost_ids = nullptr;      // an empty map is a valid call
    CHECK(reuse_check_args(a, msg, sizeof msg) == 0);
    a = in(); a.n_slots = 0; a.slot_status = nullptr;              // ... a frame without slots is one only when no point claims a slot
    CHECK(reuse_check_args(a, msg, sizeof msg) != 0 && strstr(msg, "frame_slot[0]"));
    // ---- the rotation: identity, a half turn about z, and a general unit quaternion against the double-precision matrix
    float R[9];
    reuse_rotation(qt.data(), R);
    for (int i = 0; i < 9; ++i) CHECK(R[i] == (i % 4 == 0 ? 1.f : 0.f));
    const float qz[4] = {0.f, 0.f, 1.f, 0.f};
    reuse_rotation(qz, R);
    CHECK(R[0] == -1.f && R[4] == -1.f && R[8] == 1.f && R[1] == 0.f && R[3] == 0.f);
    const double qd[4] = {0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214};
    const float qf[4] = {(float)qd[0], (float)qd[1], (float)qd[2], (float)qd[3]};
    reuse_rotation(qf, R);
    const double x = qd[0], y = qd[1], z = qd[2], w = qd[3];
    const double Rd[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                          2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    for (int i = 0; i < 9; ++i) CHECK(std::fabs((double)R[i] - Rd[i]) < 1e-6);
    // ---- the upload: every byte written, the lost flags scattered (an id listed twice is one flag)
    {
        a = in();
        const ReuseUpload U((size_t)n, (size_t)ns);
        CHECK(U.bytes == 12u * n + 4u * n + 4u * ns + n);
        std::vector<char> buf(U.bytes, (char)0x5A);
        reuse_pack_upload(a, buf.data());
        CHECK(memcmp(buf.data() + U.pos, pos.data(), 12 * n) == 0 && memcmp(buf.data() + U.slot, slot.data(), 4 * n) == 0);
        CHECK(memcmp(buf.data() + U.status, status.data(), 4 * ns) == 0);
        const char want[n] = {0, 1, 0, 0, 0, 1};
        CHECK(memcmp(buf.data() + U.lost, want, n) == 0);
        a.n_map = 0; a.n_slots = 0; a.n_lost = 0;
        const ReuseUpload U0(0, 0);
        CHECK(U0.bytes == 0);
        reuse_pack_upload(a, nullptr);                             // nothing to write: the buffer is not touched
    }
    // ---- the layouts and the unpacking, arrays of exactly n_cand (x 2) entries
    CHECK(ReuseScratch(10).words == (size_t)REUSE_HDR + 70);
    for (int ncand : {0, 1, 3, 65}) {
        const ReuseLayout L((size_t)ncand);
        CHECK(L.words == (size_t)REUSE_HDR + 7 * (size_t)ncand);
        std::vector<int32_t> pk(L.words);
        for (size_t i = 0; i < L.words; ++i) pk[i] = (int32_t)(1000 + i);
        const int nre = ncand / 2, nnew = ncand / 3;
        pk[0] = ncand; pk[1] = nre; pk[2] = nnew;
        std::vector<int32_t> c(ncand), st(ncand), acc(ncand);
        std::vector<float> sd(2 * ncand), xy(2 * ncand);
        int32_t o_nc = -1, o_nr = -1, o_nn = -1;
        const ReuseOut out{&o_nc, c.data(), sd.data(), xy.data(), st.data(), acc.data(), &o_nr, &o_nn};
        CHECK(reuse_unpack(pk.data(), ncand, out) == 0);
        CHECK(o_nc == ncand && o_nr == nre && o_nn == nnew);
        if (ncand) {
            CHECK(c[0] == pk[L.cand] && c[ncand - 1] == pk[L.cand + ncand - 1] && st[0] == pk[L.status] && acc[ncand - 1] == pk[L.accepted + ncand - 1]);
            CHECK(memcmp(sd.data(), &pk[L.seed], 8 * (size_t)ncand) == 0 && memcmp(xy.data(), &pk[L.xy], 8 * (size_t)ncand) == 0);
        }
        pk[1] = ncand + 1;                                         // headers that contradict the count: refused, nothing copied
        CHECK(reuse_unpack(pk.data(), ncand, out) != 0);
        pk[1] = nre; pk[2] = nre + 1;
        CHECK(reuse_unpack(pk.data(), ncand, out) != 0);
        pk[2] = nnew; pk[0] = ncand + 1;
        CHECK(reuse_unpack(pk.data(), ncand, out) != 0);
    }
    printf(fails ? "reuse_check: %d check(s) FAILED\n" : "reuse_check OK\n", fails);
    return fails ? 1 : 0;
}
