// What nrs_triang.hip (f2: DeformableTriangulation) and nrs_map.hip (Mapping::LandmarkTriangulation) share: the device-side flat
// TemporalBuffer, the keypoint distance of GetClosestMapPointsToFeature, and the upload + launch of k_triangulate.
#pragma once
#include <type_traits>
#include "nrs_ctx.hpp"
#include "nrs_device.hpp"

namespace nrs {

constexpr int TR_MAXF = 21;                 // TemporalBuffer size (SLAM/system.cc:42: 20, + the current frame)
enum { TR_OK = 0, TR_CLOSE, TR_REPROJ1, TR_REPROJ2, TR_PARALLAX, TR_NO_NEIGHBOUR, TR_NEG_DEPTH, TR_EMPTY, TR_BAD_NEIGHBOURS,
       TR_BAD_ERROR, TR_SHORT, TR_NAN };

struct TriArgs {
    Cam cam;
    int F, n, n_cand, min_track;
    const float* poses;          // F x 7: camera_transform_world (qx qy qz qw tx ty tz), Sophus::SE3f
    const uint8_t* has_kp;       // F x n
    const float* kp_xy;          // F x n x 2
    const uint8_t* has_lm;       // F x n
    const float* lm_xyz;         // F x n x 3
    const int* status;           // n: LandmarkStatus in the last snapshot
    const int* cand;             // n_cand
    int* o_status;               // n_cand
    float* o_xyz;                // n_cand x 3
    double* o_dbg;               // n_cand x 4 or null: final chi2, LM iterations, trials, regulariser edges
    const uint8_t* close_bits;   // n_cand or null: tb_scan_close of every candidate, computed by an earlier launch (nrs_map.hip)
};
static_assert(std::is_trivially_copyable_v<TriArgs>, "passed to kernels by value: plain pointers, never an owner");

// GetClosestMapPointsToFeature (temporal_buffer.cc:97-141) on the last snapshot: which ids are looked at, and their distance
__device__ inline bool tb_eligible(const TriArgs& A, int cand, int j) {
    return j != cand && A.has_kp[(size_t)(A.F - 1) * A.n + j] && A.status[j] == 0;
}
__device__ inline float tb_dist(const TriArgs& A, int cand, int j) {
    const float* kl = A.kp_xy + 2 * (size_t)(A.F - 1) * A.n;
    const double ddx = (double)(kl[2 * cand] - kl[2 * j]), ddy = (double)(kl[2 * cand + 1] - kl[2 * j + 1]);
    return (float)sqrt(ddx * ddx + ddy * ddy);                    // cv::norm(Point2f) -> double, stored as float
}
// The part of that function that does not depend on the order of the map: over ids first, first + stride, ...: bit 0 = a
// TRACKED_WITH_3D neighbour closer than 20 px (the function returns an empty list at once), bit 1 = one that enters the list.
__device__ inline int tb_scan_close(const TriArgs& A, int cand, int first, int stride) {
    int bits = 0;
    for (int j = first; j < A.n; j += stride)
        if (tb_eligible(A, cand, j)) {
            const float d = tb_dist(A, cand, j);
            if (!(d > 500.f)) bits |= d < 20.f ? 1 : 2;
        }
    return bits;
}

// Uploads the flat TemporalBuffer into `big` (grown to hold `extra` more bytes) and fills A's camera, sizes and input pointers;
// *rest = the first free byte behind it, 256-byte aligned.  The caller owns `big`.
int tri_upload(nrs_ctx* c, DevBuf& big, size_t extra, const nrs_camera* cam, int n_frames, const float* poses, int n_ids, const uint8_t* has_kp,
               const float* kp_xy, const uint8_t* has_lm, const float* lm_xyz, const int32_t* last_status, int min_track, TriArgs& A, char** rest);
// k_triangulate over A.cand[0 .. A.n_cand) on the context's stream (cand, o_status, o_xyz, o_dbg are device pointers)
int tri_launch(nrs_ctx* c, const TriArgs& A);

// nrs_map.hip, for both forms of frame mapping (nrs_map_frame on a flat buffer from the host, nrs_map_frame_tbuf on the resident one,
// nrs_tbuf.hip): the launches behind the upload, the download of the packed result and its unpacking
struct MapOut;
size_t map_ws_bytes(int n_cand);
int map_run(nrs_ctx* c, const char* who, const TriArgs& T, const float* d_deform_mag, char* ws, int n_cand, float rad_per_pixel, float rigidity_th,
            int index_snapshot, const int* d_row_id, const MapOut& out);

}  // namespace nrs
