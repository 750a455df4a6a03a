// Stand-alone check of the host pieces of the BA-window entry points (csrc/nrs_dba_host.hpp) for a sanitizer build:
// `make dba_check && ./dba_check`.  No HIP, no library.
//   validators   every refusal of window_validate_kf / window_validate with its code and its exact text, under two entry-point names and
//                both kinds of bound: null arguments, n_kf = 0, an unknown camera, an empty window, kf_rowptr[0] != 0, a decreasing kf_rowptr,
//                an index equal to n_points; null / decreasing / out-of-range neighbour lists.  Windows that pass: n_kf = 1, an empty
//                keyframe in the middle -- and the keyframe of every observation they leave
//   gather, scatter   gather_obs over a hand-made index list with an unbound observation, then points_to_float back: the identity on the
//                bound rows, the unbound row untouched; the dense form
//   constants    ba_constants against the literal doubles of the float expressions of OPT:958-973 for scale = 1 and scale = 0.37f
//   builder      embwin_builder over its whole truth table (world 1..9, n_kf 1..9) against the conditions written out
//   poses        qt -> Pose -> qt with a counting normaliser
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../csrc/nrs_dba_host.hpp"

using namespace nrs_dba;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "dba_check: %s:%d: %s\n", __FILE__, __LINE__, #x); std::abort(); } } while (0)

static bool is(const Refusal& r, const char* text) { return r.code == NRS_ERR_INVALID && r.text == text; }

struct Win {                                                        // 3 keyframes, 5 observations of 4 map points; keyframe 1 is empty
    nrs_camera cam;
    int32_t n_kf = 3, n_points = 4;
    std::vector<double> qt = std::vector<double>(21, 0.0);
    std::vector<int32_t> rowptr = {0, 3, 3, 5}, pt = {0, 1, 3, 2, 3};
    std::vector<float> xyz = std::vector<float>(15, 1.f), uv = std::vector<float>(10, 2.f);
    std::vector<int32_t> nrp = {0, 1, 2, 3, 4}, col = {1, 0, 3, 2}, st = {0, 0, 0, 0};
    std::vector<float> w = {1, 1, 1, 1}, d0 = {1, 1, 1, 1};
    Win() { std::memset(&cam, 0, sizeof(cam)); cam.model = NRS_CAM_PINHOLE; }
    Refusal kf(const char* who, Bound b, std::vector<int32_t>& lm_kf) const {
        return window_validate_kf(who, b, &cam, n_kf, qt.data(), rowptr.data(), pt.data(), xyz.data(), uv.data(), n_points, lm_kf);
    }
    Refusal full(const char* who, std::vector<int32_t>& lm_kf) const {
        return window_validate(who, &cam, n_kf, qt.data(), rowptr.data(), pt.data(), xyz.data(), uv.data(), n_points, nrp.data(), col.data(), w.data(), d0.data(), st.data(), lm_kf);
    }
};

static void check_validators() {
    std::vector<int32_t> lm_kf;
    const Win ok;
    // windows that pass, and the keyframe of every observation (the empty keyframe in the middle owns none)
    CHECK(ok.kf("A", MAP_POINTS, lm_kf).ok() && ok.kf("A", MAP_POINTS, lm_kf).text.empty() && lm_kf == (std::vector<int32_t>{0, 0, 0, 2, 2}));
    lm_kf.clear();
    CHECK(ok.full("A", lm_kf).ok() && lm_kf == (std::vector<int32_t>{0, 0, 0, 2, 2}));
    { Win x; x.n_kf = 1; x.rowptr = {0, 5}; lm_kf.clear(); CHECK(x.full("A", lm_kf).ok() && lm_kf == (std::vector<int32_t>(5, 0))); }
    // the keyframe side: every null, every count
    for (int k = 0; k < 8; ++k) {
        const Win x;
        const Refusal r = window_validate_kf("nrs_dba_solve_window_rg", GRAPH_CAPACITY, k == 0 ? nullptr : &x.cam, k == 1 ? 0 : x.n_kf, k == 2 ? nullptr : x.qt.data(),
                                             k == 3 ? nullptr : x.rowptr.data(), k == 4 ? nullptr : x.pt.data(), k == 5 ? nullptr : x.xyz.data(),
                                             k == 6 ? nullptr : x.uv.data(), k == 7 ? 0 : x.n_points, lm_kf);
        CHECK(is(r, "nrs_dba_solve_window_rg: bad argument"));
    }
    { Win x; x.cam.model = 7; CHECK(is(x.kf("A", MAP_POINTS, lm_kf), "unknown camera model 7")); }
    { Win x; x.rowptr = {0, 0, 0, 0}; CHECK(is(x.kf("nrs_dba_solve_window_rg", GRAPH_CAPACITY, lm_kf), "nrs_dba_solve_window_rg: empty window")); }
    { Win x; x.rowptr = {0, 0, 0, 0}; CHECK(is(x.full("nrs_dba_solve_window_embedded", lm_kf), "nrs_dba_solve_window_embedded: empty window")); }
    { Win x; x.rowptr = {1, 3, 3, 5}; CHECK(is(x.kf("nrs_dba_solve_window", MAP_POINTS, lm_kf), "nrs_dba_solve_window: empty window")); }     // kf_rowptr[0] != 0
    { Win x; x.rowptr = {0, 3, 2, 5}; CHECK(is(x.kf("A", MAP_POINTS, lm_kf), "kf_rowptr must be non-decreasing")); }
    { Win x; x.pt[4] = 4; CHECK(is(x.kf("A", MAP_POINTS, lm_kf), "map point index out of range")); }                                           // = n_points
    { Win x; x.pt[0] = -1; CHECK(is(x.full("A", lm_kf), "map point index out of range")); }
    { Win x; x.pt[4] = 4;
      CHECK(is(x.kf("nrs_dba_solve_window_rg_embedded", GRAPH_CAPACITY, lm_kf), "nrs_dba_solve_window_rg_embedded: map point index 4 is beyond the graph's capacity 4")); }
    { Win x; x.pt[1] = -2; CHECK(is(x.kf("nrs_dba_solve_window_rg", GRAPH_CAPACITY, lm_kf), "nrs_dba_solve_window_rg: map point index -2 is beyond the graph's capacity 4")); }
    // the neighbour side
    for (int k = 0; k < 5; ++k) {
        const Win x;
        const Refusal r = window_validate("nrs_dba_solve_window_embedded", &x.cam, x.n_kf, x.qt.data(), x.rowptr.data(), x.pt.data(), x.xyz.data(), x.uv.data(), x.n_points,
                                          k == 0 ? nullptr : x.nrp.data(), k == 1 ? nullptr : x.col.data(), k == 2 ? nullptr : x.w.data(), k == 3 ? nullptr : x.d0.data(),
                                          k == 4 ? nullptr : x.st.data(), lm_kf);
        CHECK(is(r, "nrs_dba_solve_window_embedded: bad argument"));
    }
    { Win x; x.n_points = 0; CHECK(is(x.full("nrs_dba_solve_window", lm_kf), "nrs_dba_solve_window: bad argument")); }                        // (before nbr_rowptr is read)
    { Win x; x.nrp[0] = 1; CHECK(is(x.full("A", lm_kf), "nbr_rowptr must start at 0")); }
    { Win x; x.nrp = {0, 2, 1, 3, 4}; CHECK(is(x.full("A", lm_kf), "nbr_rowptr must be non-decreasing")); }
    { Win x; x.col[3] = 4; CHECK(is(x.full("A", lm_kf), "neighbour index out of range")); }
    { Win x; x.col[0] = -1; CHECK(is(x.full("A", lm_kf), "neighbour index out of range")); }
    { Win x; x.nrp = {0, 0, 0, 0, 0}; CHECK(x.full("A", lm_kf).ok()); }                                                                        // empty lists pass
}

static void check_gather_scatter() {
    const int n_obs = 6;                                            // observation 3 is bound to nothing
    std::vector<float> obs_xyz(3 * n_obs), obs_uv(2 * n_obs);
    std::vector<int32_t> obs_kf = {0, 0, 1, 1, 2, 2};
    for (int i = 0; i < 3 * n_obs; ++i) obs_xyz[i] = 0.1f * (float)(i + 1);
    for (int i = 0; i < 2 * n_obs; ++i) obs_uv[i] = 100.f + (float)i;
    const std::vector<int32_t> lm = {4, 0}, sk = {5, 1, 2};
    std::vector<float> lx(6), lu(4), sx(9), su(6);
    std::vector<int32_t> lk(2), skf(3);
    gather_obs(2, lm.data(), obs_xyz.data(), obs_uv.data(), obs_kf.data(), lx.data(), lu.data(), lk.data());
    gather_obs(3, sk.data(), obs_xyz.data(), obs_uv.data(), obs_kf.data(), sx.data(), su.data(), skf.data());
    gather_obs(0, nullptr, obs_xyz.data(), obs_uv.data(), obs_kf.data(), nullptr, nullptr, nullptr);
    CHECK(lk == (std::vector<int32_t>{2, 0}) && skf == (std::vector<int32_t>{2, 0, 1}));
    for (int a = 0; a < 3; ++a) CHECK(lx[a] == obs_xyz[12 + a] && lx[3 + a] == obs_xyz[a] && sx[a] == obs_xyz[15 + a] && sx[3 + a] == obs_xyz[3 + a] && sx[6 + a] == obs_xyz[6 + a]);
    for (int a = 0; a < 2; ++a) CHECK(lu[a] == obs_uv[8 + a] && lu[2 + a] == obs_uv[a] && su[a] == obs_uv[10 + a] && su[2 + a] == obs_uv[2 + a] && su[4 + a] == obs_uv[4 + a]);
    // the way back, through double as the download has them: the identity, observation 3 as it was
    std::vector<double> ld(lx.begin(), lx.end()), sd(sx.begin(), sx.end());
    std::vector<float> out(3 * n_obs, -7.f);
    points_to_float(2, lm.data(), ld.data(), out.data());
    points_to_float(3, sk.data(), sd.data(), out.data());
    points_to_float(0, nullptr, nullptr, out.data());
    for (int i = 0; i < 3 * n_obs; ++i) CHECK(out[i] == (i / 3 == 3 ? -7.f : obs_xyz[i]));
    // the dense form, and the cast (the nearest float)
    const std::vector<double> d = {1.0, 0.1, -2.5, 3.0000000001, 1e-50, 16777217.0};
    std::vector<float> f(6, 0.f);
    points_to_float(2, nullptr, d.data(), f.data());
    for (int i = 0; i < 6; ++i) CHECK(f[i] == (float)d[i]);
    CHECK(f[1] == 0.1f && f[3] == 3.f && f[4] == 0.f && f[5] == 16777216.f);
}

static void check_constants() {
    // sqrtf(5.99f), sqrtf(0.584f), 1 / 0.25f, 1 / (0.1f * 0.1f), 1.1f and 1 / (s * s) with s = (float)(0.1 * scale): the nearest floats, widened
    const BaConstants a = ba_constants(1.f), b = ba_constants(0.37f);
    CHECK(a.info_reproj == 4.0 && a.delta_reproj == 2.4474475383758544921875 && a.info_pos == 99.99999237060546875 && a.delta_spatial == 0.76419889926910400390625);
    CHECK(a.k_spring == 1.10000002384185791015625 && a.info_spatial == 99.99999237060546875);
    CHECK(b.info_reproj == a.info_reproj && b.delta_reproj == a.delta_reproj && b.info_pos == a.info_pos && b.delta_spatial == a.delta_spatial && b.k_spring == a.k_spring);
    CHECK(b.info_spatial == 730.46014404296875);
}

static void check_builder() {
    int n = 0;
    for (int comm = 0; comm < 2; ++comm)
        for (int world = 1; world <= 9; ++world)
            for (int n_kf = 1; n_kf <= 9; ++n_kf)
                for (int sw = 0; sw < 8; ++sw, ++n) {
                    const bool shard_sw = sw & 1, host_sw = sw & 2, nnz = sw & 4;
                    const EmbwinBuilder by = embwin_builder(comm, world, n_kf, shard_sw, host_sw, nnz);
                    bool shard = false, device = false;
                    if (comm && shard_sw && world <= 8 && n_kf >= world) shard = true;
                    if (!host_sw && nnz) device = comm ? shard : true;
                    CHECK(by.shard == shard && by.device == device);
                    if (!comm) CHECK(!by.shard);                     // one GPU: never a share
                }
    CHECK(n == 2 * 9 * 9 * 8);
    CHECK(embwin_builder(true, 9, 9, true, false, true).device == false && embwin_builder(true, 8, 8, true, false, true).shard == true);
    CHECK(embwin_builder(true, 3, 2, true, false, true).device == false && embwin_builder(true, 2, 4, false, false, true).device == false);
}

struct P { double q[4], t[3]; };
static void check_poses() {
    const double qt[14] = {1, 2, 3, 4, 5, 6, 7, -1, -2, -3, -4, -5, -6, -7};
    P p[2];
    int calls = 0;
    poses_from_qt(2, qt, p, [&](double* q) { ++calls; q[0] += 0.5; });
    CHECK(calls == 2 && p[0].q[0] == 1.5 && p[0].q[3] == 4 && p[0].t[0] == 5 && p[0].t[2] == 7 && p[1].q[0] == -0.5 && p[1].q[1] == -2 && p[1].t[1] == -6);
    double back[14];
    poses_to_qt(2, p, back);
    for (int i = 0; i < 14; ++i) CHECK(back[i] == (i % 7 == 0 ? qt[i] + 0.5 : qt[i]));
    poses_from_qt(0, nullptr, (P*)nullptr, [](double*) {});
    poses_to_qt(0, (const P*)nullptr, (double*)nullptr);
}

int main() {
    check_validators();
    check_gather_scatter();
    check_constants();
    check_builder();
    check_poses();
    std::printf("dba_check OK: the refusals of the two window validators with code and text under the entry points' names and both bounds, windows that "
                "pass (n_kf = 1, an empty keyframe in the middle); gather then scatter over an index list with an unbound observation; the constants "
                "for scale 1 and 0.37; the embedded builder's truth table; qt <-> Pose\n");
    return 0;
}
