// a3, the host pieces of the BA-window entry points (nrs_dba.hip): the argument checks of a window with their texts, the constants of
// OPT:958-973, the qt <-> Pose packing, the per-observation gather and scatter of an embedded window, and which builder makes its lists.
// Plain C++17, no HIP and no context: nrs_dba.hip turns a Refusal into the context's error text; host/dba_check.cpp runs all of it under
// sanitizers (`make dba_check`).
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>
#include "../../include/nrs.h"

namespace nrs_dba {

// ---- constants of OPT:958-973 (float arithmetic, widened to double like g2o does)
struct BaConstants { double info_reproj, delta_reproj, info_pos, info_spatial, delta_spatial, k_spring; };
inline BaConstants ba_constants(float scale) {
    const float th2 = sqrtf(5.99f), th3 = sqrtf(0.584f);
    const float sigma_rep = 0.5f, sigma_pos = 0.1f;
    const float sigma_spatial = (float)(0.1 * (double)scale);
    BaConstants k;
    k.info_reproj = (double)(1.0f / (sigma_rep * sigma_rep));
    k.delta_reproj = (double)th2;
    k.info_pos = (double)(1.0f / (sigma_pos * sigma_pos));
    k.info_spatial = (double)(1.0f / (sigma_spatial * sigma_spatial));
    k.delta_spatial = (double)th3;
    k.k_spring = (double)1.1f;
    return k;
}

// ---- poses as the C ABI has them (n_kf x 7: quaternion x y z w, translation) <-> the engine's Pose (q[4], t[3]); normalize: the SE3Quat
// constructor's (se3quat.h:56-58), nrs_device.hpp quat_normalize in the library
template <class PoseT, class Normalize> inline void poses_from_qt(int32_t n_kf, const double* qt, PoseT* poses, Normalize normalize) {
    for (int k = 0; k < n_kf; ++k) {
        for (int i = 0; i < 4; ++i) poses[k].q[i] = qt[7 * k + i];
        for (int i = 0; i < 3; ++i) poses[k].t[i] = qt[7 * k + 4 + i];
        normalize(poses[k].q);
    }
}
template <class PoseT> inline void poses_to_qt(int32_t n_kf, const PoseT* poses, double* qt) {
    for (int k = 0; k < n_kf; ++k) {
        for (int i = 0; i < 4; ++i) qt[7 * k + i] = poses[k].q[i];
        for (int i = 0; i < 3; ++i) qt[7 * k + 4 + i] = poses[k].t[i];
    }
}

// ---- rows of the per-observation arrays selected by an index list (the node copies / the skinned observations of an embedded window) ...
inline void gather_obs(int32_t n, const int32_t* idx, const float* obs_xyz, const float* obs_uv, const int32_t* obs_kf, float* xyz, float* uv, int32_t* kf) {
    for (int32_t i = 0; i < n; ++i) {
        const size_t o = (size_t)idx[i];
        for (int a = 0; a < 3; ++a) xyz[3 * (size_t)i + a] = obs_xyz[3 * o + a];
        for (int a = 0; a < 2; ++a) uv[2 * (size_t)i + a] = obs_uv[2 * o + a];
        kf[i] = obs_kf[o];
    }
}
// ... and the way back for the solved points: row i of xyz to row idx[i] of out (idx null: row i), observations no index names untouched
inline void points_to_float(int32_t n, const int32_t* idx, const double* xyz, float* out) {
    for (int32_t i = 0; i < n; ++i) {
        const size_t o = idx ? (size_t)idx[i] : (size_t)i;
        for (int a = 0; a < 3; ++a) out[3 * o + a] = (float)xyz[3 * (size_t)i + a];          // OPT:1158 cast<float>
    }
}

// ---- which builder makes the lists of nrs_dba_solve_window_embedded.  device: engine_build_embedded_window_device, else the host's
// nrs_dba_build_edges_embedded (the same lists); shard: on the device, every rank its own share (NRS_SHARD_EMBWIN_DEVICE on a
// communicator).  More ranks than keyframes, more than 8 ranks: the set-up refuses those alike on every rank -- reached through the host builder
struct EmbwinBuilder { bool device, shard; };
inline EmbwinBuilder embwin_builder(bool comm, int world, int32_t n_kf, bool shard_switch, bool host_pack_switch, bool any_neighbour) {
    const bool shard = comm && shard_switch && world <= 8 && n_kf >= world;
    return {(!comm || shard) && !host_pack_switch && any_neighbour, shard};
}

// ---- the argument checks of a window, in two levels: the keyframe side (every window call) and the neighbour side (the calls that take the
// caller's CSR lists).  A Refusal is the code and the text the context reports; every text that names a call names `who`, the entry point called
struct Refusal {
    int code = NRS_OK;
    std::string text;
    bool ok() const { return code == NRS_OK; }
};
inline Refusal refuse(std::string text) { return {NRS_ERR_INVALID, std::move(text)}; }
// what the map-point indices of kf_pt are bounded by: the caller's n_points lists, or the capacity of the device-resident graph
enum Bound { MAP_POINTS, GRAPH_CAPACITY };

// lm_kf: the keyframe of every observation, filled when the window passes
inline Refusal window_validate_kf(const char* who, Bound bound, const nrs_camera* cam, int32_t n_kf, const double* poses_qt, const int32_t* kf_rowptr, const int32_t* kf_pt,
                                  const float* lm_xyz, const float* lm_uv, int32_t n_points, std::vector<int32_t>& lm_kf) {
    if (!cam || n_kf <= 0 || !poses_qt || !kf_rowptr || !kf_pt || !lm_xyz || !lm_uv || n_points <= 0) return refuse(std::string(who) + ": bad argument");
    if (cam->model != NRS_CAM_PINHOLE && cam->model != NRS_CAM_KB8) return refuse("unknown camera model " + std::to_string(cam->model));
    const int32_t n_lm = kf_rowptr[n_kf];
    if (kf_rowptr[0] != 0 || n_lm <= 0) return refuse(std::string(who) + ": empty window");
    for (int k = 0; k < n_kf; ++k) if (kf_rowptr[k + 1] < kf_rowptr[k]) return refuse("kf_rowptr must be non-decreasing");
    for (int32_t i = 0; i < n_lm; ++i)
        if (kf_pt[i] < 0 || kf_pt[i] >= n_points)
            return bound == MAP_POINTS ? refuse("map point index out of range")
                                       : refuse(std::string(who) + ": map point index " + std::to_string(kf_pt[i]) + " is beyond the graph's capacity " + std::to_string(n_points));
    lm_kf.resize(n_lm);
    for (int k = 0; k < n_kf; ++k) for (int32_t i = kf_rowptr[k]; i < kf_rowptr[k + 1]; ++i) lm_kf[i] = k;
    return {};
}

inline Refusal window_validate(const char* who, const nrs_camera* cam, int32_t n_kf, const double* poses_qt, const int32_t* kf_rowptr, const int32_t* kf_pt,
                               const float* lm_xyz, const float* lm_uv, int32_t n_points, const int32_t* nbr_rowptr, const int32_t* nbr_col, const float* nbr_w,
                               const float* nbr_d0, const int32_t* nbr_status, std::vector<int32_t>& lm_kf) {
    if (!nbr_rowptr || !nbr_col || !nbr_w || !nbr_d0 || !nbr_status) return refuse(std::string(who) + ": bad argument");
    const Refusal r = window_validate_kf(who, MAP_POINTS, cam, n_kf, poses_qt, kf_rowptr, kf_pt, lm_xyz, lm_uv, n_points, lm_kf);
    if (!r.ok()) return r;
    if (nbr_rowptr[0] != 0) return refuse("nbr_rowptr must start at 0");
    for (int32_t p = 0; p < n_points; ++p) if (nbr_rowptr[p + 1] < nbr_rowptr[p]) return refuse("nbr_rowptr must be non-decreasing");
    for (int32_t i = 0; i < nbr_rowptr[n_points]; ++i) if (nbr_col[i] < 0 || nbr_col[i] >= n_points) return refuse("neighbour index out of range");
    return {};
}

}  // namespace nrs_dba
