// Stand-alone check of the host half of the evaluation (csrc/nrs_eval_host.hpp: nrs_eval_rmse, nrs_stereo_from_tracks and the SE3f pieces)
// for a sanitizer build: `make eval_check && ./eval_check`.  It walks the inputs where an index could leave its array: empty input, no valid
// point, n = 1 .. 3 (n_inliers 0 and 1, the unaligned form's sorted[n_inliers]), ties at the inlier threshold, gross outliers.
#include <cstdio>
#include <cstdlib>
#include "../csrc/nrs_eval_host.hpp"

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static int run(const std::vector<float>& est, const std::vector<float>& gt, const std::vector<uint8_t>& ok, int align, int pre, float* rmse,
               float* scale, int32_t* counts) {
    std::vector<uint8_t> inl(est.size() + 1, 7);                     // one guard byte behind the mask
    const int rc = nrs_eval::eval_rmse((int)est.size(), est.data(), gt.data(), ok.data(), align, pre, rmse, scale, counts, inl.data());
    EXPECT(inl[est.size()] == 7);
    return rc;
}

int main() {
    float rmse, scale;
    int32_t counts[3];
    for (int align = 0; align < 2; ++align)
        for (int pre = 0; pre < 2; ++pre) {
            EXPECT(run({}, {}, {}, align, pre, &rmse, &scale, counts) == NRS_ERR_INVALID && std::isnan(rmse) && std::isnan(scale));
            EXPECT(run({1.f, 2.f}, {1.f, 2.f}, {0, 0}, align, pre, &rmse, &scale, counts) == NRS_ERR_INVALID && counts[0] == 0);
            const int rc1 = run({2.f}, {3.f}, {1}, align, pre, &rmse, &scale, counts);       // n = 1: (int)(1 * 0.9f) = 0 inliers
            EXPECT(rc1 == NRS_ERR_INVALID && counts[0] == 1 && counts[2] == 0 && std::isnan(rmse));
            for (int n = 2; n <= 12; ++n) {
                std::vector<float> e(n), g(n);
                std::vector<uint8_t> ok(n, 1);
                for (int i = 0; i < n; ++i) { e[i] = 1.f + 0.25f * i; g[i] = 1.7f * e[i] + ((i % 3) ? 0.01f : -0.02f); }
                const int rc = run(e, g, ok, align, pre, &rmse, &scale, counts);
                EXPECT(rc == NRS_OK && std::isfinite(rmse) && counts[2] >= 1 && counts[2] <= counts[1]);
                if (align) EXPECT(std::fabs(scale - 1.7f) < 0.05f);
            }
            // exact ties at the inlier threshold: every squared residual equal
            std::vector<float> e(10, 2.f), g(10, 2.5f);
            std::vector<uint8_t> ok(10, 1);
            EXPECT(run(e, g, ok, align, pre, &rmse, &scale, counts) == NRS_OK && counts[2] == 9);
            // gross outliers behind the IQR gate
            std::vector<float> e2(40), g2(40);
            std::vector<uint8_t> ok2(40, 1);
            for (int i = 0; i < 40; ++i) { e2[i] = 3.f + 0.1f * i; g2[i] = e2[i] + 0.001f * (i % 5) + (i % 13 == 0 ? 50.f : 0.f); }
            EXPECT(run(e2, g2, ok2, align, pre, &rmse, &scale, counts) == NRS_OK);
            EXPECT((align && pre) ? counts[1] == 40 : counts[1] == 36);
        }
    // nrs_stereo_from_tracks: the 2.0 / 2.0001 row difference, a zero disparity, an untracked point, n = 0
    nrs_camera cam;
    cam.model = NRS_CAM_PINHOLE;
    const float prm[8] = {400.f, 410.f, 320.f, 240.f, 0, 0, 0, 0};
    for (int i = 0; i < 8; ++i) cam.params[i] = prm[i];
    const float l[8] = {100.f, 50.f, 120.f, 60.f, 140.f, 70.f, 160.f, 80.f}, r[8] = {90.f, 52.f, 110.f, 62.0001f, 140.f, 70.5f, 150.f, 80.f};
    const int32_t ts[4] = {NRS_TRACKED, NRS_TRACKED, NRS_TRACKED, NRS_BAD};
    float xyz[12];
    int32_t st[4];
    EXPECT(nrs_eval::stereo_from_tracks(&cam, 5.f, 4, l, r, ts, xyz, st) == NRS_OK);
    EXPECT(st[0] == NRS_EVAL_OK && st[1] == NRS_EVAL_ROW_DIFFERENCE && st[2] == NRS_EVAL_ZERO_DISPARITY && st[3] == NRS_EVAL_NOT_TRACKED);
    EXPECT(xyz[2] == 0.5f && std::isnan(xyz[5]));
    EXPECT(nrs_eval::stereo_from_tracks(&cam, 5.f, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == NRS_OK);
    // SE3f: T^-1 * (T * X) returns X to fp32 accuracy
    const float qt[7] = {0.1f, -0.2f, 0.05f, 0.9734f, 0.3f, -0.1f, 2.f}, X[3] = {0.4f, -0.7f, 3.f};
    float Y[3], Z[3];
    nrs_eval::se3f_act(nrs_eval::se3f(qt), X, Y);
    nrs_eval::se3f_act(nrs_eval::se3f_inv(qt), Y, Z);
    EXPECT(std::fabs(Z[0] - X[0]) < 1e-3f && std::fabs(Z[1] - X[1]) < 1e-3f && std::fabs(Z[2] - X[2]) < 1e-3f);
    std::printf(failures ? "eval_check: %d FAILED\n" : "eval_check: all passed\n", failures);
    return failures ? 1 : 0;
}
