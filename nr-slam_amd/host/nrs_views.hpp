// Host-side mirror of the reference's module interface for the hot path, on flat views.
//
// The reference functions take Frame / Map / KeyFrame objects (modules/optimization/
// g2o_optimization.h:27-40).  A drop-in keeps those signatures and does three things: flatten the
// containers into the views below, call the C ABI, write the results back.  This header holds the
// compilable, reference-type-free half (views + calls, same names / argument meaning / error
// behaviour as the reference); INTEGRATION.md shows the ~40-line flattening stubs that use the
// reference's own accessors.
#pragma once
#include <cstdint>
#include <fstream>
#include <functional>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/nrs.h"

namespace nrs_host {

struct CameraView {                       // CameraModel::GetParameters() (calibration/camera_model.h:60-62)
    nrs_camera cam;
    static CameraView PinHole(float fx, float fy, float cx, float cy) {
        CameraView v{};
        v.cam.model = NRS_CAM_PINHOLE;
        v.cam.params[0] = fx; v.cam.params[1] = fy; v.cam.params[2] = cx; v.cam.params[3] = cy;
        return v;
    }
    static CameraView KannalaBrandt8(const float p[8]) {
        CameraView v{};
        v.cam.model = NRS_CAM_KB8;
        for (int i = 0; i < 8; ++i) v.cam.params[i] = p[i];
        return v;
    }
};

// Frame arrays in index order (map/frame.h:108-123): keypoints, landmark positions, statuses and
// the map-point index of every slot (-1 when the slot has no map point).
struct FrameView {
    std::vector<float> uv;                // n x 2   cv::KeyPoint::pt
    std::vector<float> pos;               // n x 3   LandmarkPositions()
    std::vector<int32_t> status;          // n       LandmarkStatuses()
    std::vector<int32_t> map_index;       // n       MapPointIdToIndex() inverted
    double pose_qt[7];                    // CameraTransformationWorld() as (unit quaternion xyzw, translation)
    float deformation_magnitude = 0.f;    // SetDeformationMaginitud
};

// RegularizationGraph (map/regularization_graph.h:49-96) + MapPoint::GetLastWorldPosition
struct MapView {
    std::vector<int32_t> rowptr, col, eid;
    std::vector<float> e_w, e_d0, e_max, e_min;
    std::vector<int32_t> e_status;
    std::vector<float> last_world_position;   // n_points x 3
    float sigma = 0.f, stretch_th = 1.1f, scale = 1.f;
    nrs_graph c_graph() {
        nrs_graph g;
        g.n_points = (int32_t)rowptr.size() - 1;
        g.rowptr = rowptr.data(); g.col = col.data(); g.eid = eid.data();
        g.n_edges = (int32_t)e_w.size();
        g.e_w = e_w.data(); g.e_d0 = e_d0.data(); g.e_max = e_max.data(); g.e_min = e_min.data();
        g.e_status = e_status.data();
        g.sigma = sigma; g.stretch_th = stretch_th;
        return g;
    }
};

struct KeyFrameWindow {                   // the BA window, oldest keyframe first (OPT:894-952)
    std::vector<double> poses_qt;         // n_kf x 7
    std::vector<int32_t> kf_rowptr, kf_pt;  // TRACKED_WITH_3D observations per keyframe -> map index
    std::vector<float> lm_uv, lm_xyz;     // per (keyframe, point) landmark, keyframe-major
};

// TemporalBuffer flattened (map/temporal_buffer.h:43-63): n_frames snapshots, oldest first; per snapshot the camera pose
// and, per keypoint id, the keypoint (keypoint_tracks) and the landmark position (mapppoint_tracks_) when present.
// This is the wire form nrs_triangulate_batch reads (and what tests/golden stores for f2).
struct TemporalBufferView {
    int32_t n_frames = 0, n_ids = 0;
    std::vector<float> poses;             // n_frames x 7   Snapshot::camera_transform_world (qx qy qz qw tx ty tz)
    std::vector<uint8_t> has_kp, has_lm;  // n_frames x n_ids
    std::vector<float> kp_xy;             // n_frames x n_ids x 2
    std::vector<float> lm_xyz;            // n_frames x n_ids x 3
    std::vector<int32_t> last_status;     // n_ids          keypoint_tracks_status of the last snapshot
};

// KeyFrame snapshot (map/keyframe.cc:26-55): what a keyframe keeps of its frame, i.e. one block of KeyFrameWindow
struct KeyFrameView {
    double pose_qt[7];
    std::vector<int32_t> map_index;       // TRACKED_WITH_3D observations in keyframe index order
    std::vector<float> uv, xyz;
    void append_to(KeyFrameWindow& w) const;
};

class Engine {                            // owns one nrs_ctx; not thread-safe, like the reference's callers
public:
    explicit Engine(int device = -1) {
        nrs_options opt;
        nrs_options_init(&opt);
        opt.device = device;
        if (nrs_create(&ctx_, &opt) != NRS_OK) throw std::runtime_error("nrs_create: no usable HIP device");
    }
    ~Engine() { nrs_destroy(ctx_); }
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;

    // void CameraPoseOptimization(Frame&, const Sophus::SE3f&)   g2o_optimization.h:27
    void CameraPoseOptimization(const CameraView& cam, FrameView& f) {
        std::vector<float> uv, X;
        for (size_t i = 0; i < f.status.size(); ++i)
            if (f.status[i] == NRS_TRACKED_WITH_3D) {
                uv.insert(uv.end(), {f.uv[2 * i], f.uv[2 * i + 1]});
                X.insert(X.end(), {f.pos[3 * i], f.pos[3 * i + 1], f.pos[3 * i + 2]});
            }
        check(nrs_pose_only_solve(ctx_, &cam.cam, (int32_t)(uv.size() / 2), uv.data(), X.data(), f.pose_qt, nullptr, nullptr));
    }

    // absl::flat_hash_set<ID> CameraPoseAndDeformationOptimization(Frame&, shared_ptr<Map>, const SE3f&, float)
    // g2o_optimization.h:29-32.  Returns the re-located lost map points.
    std::vector<int32_t> CameraPoseAndDeformationOptimization(const CameraView& cam, FrameView& f, MapView& m) {
        nrs_graph g = m.c_graph();
        std::vector<int32_t> lost((size_t)g.n_points);
        int32_t n_lost = 0;
        check(nrs_track_deform_solve(ctx_, &cam.cam, &g, m.last_world_position.data(), (int32_t)f.status.size(),
                                     f.map_index.data(), f.status.data(), f.uv.data(), f.pos.data(), f.pose_qt, m.scale,
                                     &f.deformation_magnitude, &n_lost, lost.data(), nullptr));
        lost.resize((size_t)n_lost);
        return lost;
    }

    // The same with the map's graph kept as a device-resident RegularizationGraph (all-pairs density): GetEdges / UpdateVertex
    // of OPT:252,468,496 are served there.  cap_per_point = how much of each sorted neighbour list is fetched.
    inline std::vector<int32_t> CameraPoseAndDeformationOptimization(const CameraView& cam, FrameView& f, MapView& m, class RegularizationGraph& graph,
                                                                     int cap_per_point = 64);

    // Skinned mode (include/nrs.h N2): M farthest-point graph nodes among the eligible map points (pick order)
    std::vector<int32_t> SelectGraphNodes(const std::vector<float>& positions, const std::vector<uint8_t>& eligible, int n_nodes) {
        std::vector<int32_t> nodes((size_t)n_nodes);
        check(nrs_skin_select_nodes(ctx_, (int32_t)(positions.size() / 3), positions.data(), eligible.empty() ? nullptr : eligible.data(), n_nodes, nodes.data()));
        return nodes;
    }

    // void LocalDeformableBundleAdjustment(shared_ptr<Map>, float scale)   g2o_optimization.h:39-40
    void LocalDeformableBundleAdjustment(const CameraView& cam, KeyFrameWindow& w, MapView& m, int iterations = 5) {
        const int32_t n_kf = (int32_t)w.kf_rowptr.size() - 1;
        if (n_kf < 3) return;                                              // OPT:922-924
        nrs_graph g = m.c_graph();
        std::vector<int32_t> orp((size_t)g.n_points + 1), ocol(m.col.size()), oeid(m.col.size());
        check(nrs_graph_select_neighbours(ctx_, &g, orp.data(), ocol.data(), oeid.data()));
        std::vector<float> nw(ocol.size()), nd0(ocol.size());
        std::vector<int32_t> nst(ocol.size());
        for (int32_t a = 0; a < orp.back(); ++a) { nw[a] = m.e_w[oeid[a]]; nd0[a] = m.e_d0[oeid[a]]; nst[a] = m.e_status[oeid[a]]; }
        int32_t ns = 0, nd = 0;
        check(nrs_dba_build_edges(n_kf, w.kf_rowptr.data(), w.kf_pt.data(), g.n_points, orp.data(), ocol.data(), nw.data(),
                                  nd0.data(), nst.data(), &ns, nullptr, nullptr, &nd, nullptr, nullptr));
        std::vector<int32_t> sp(2 * (size_t)ns), dm(4 * (size_t)nd), lm_kf(w.kf_pt.size());
        std::vector<float> d0((size_t)ns), dw((size_t)nd);
        check(nrs_dba_build_edges(n_kf, w.kf_rowptr.data(), w.kf_pt.data(), g.n_points, orp.data(), ocol.data(), nw.data(),
                                  nd0.data(), nst.data(), &ns, sp.data(), d0.data(), &nd, dm.data(), dw.data()));
        for (int32_t k = 0; k < n_kf; ++k)
            for (int32_t l = w.kf_rowptr[k]; l < w.kf_rowptr[k + 1]; ++l) lm_kf[l] = k;
        check(nrs_dba_solve(ctx_, &cam.cam, n_kf, w.poses_qt.data(), (int32_t)lm_kf.size(), w.lm_xyz.data(), lm_kf.data(),
                            w.lm_uv.data(), ns, sp.data(), d0.data(), nd, dm.data(), dw.data(), m.scale, iterations, nullptr));
    }

    // The EMBEDDED form of the same call (include/nrs.h N2b; BASELINE configs[1] "points x graph nodes x keyframes"): is_node flags the
    // map points that carry vertices (e.g. SelectGraphNodes once per map); the other observations of the window are skinned to the
    // <= 11 node copies of their keyframe their walk accepts and keep their reprojection edges.  The walks see GetEdges lists with
    // everything but the nodes passed over: here they are cut out of the flat graph's ordered lists.  w.lm_xyz comes back with the
    // node copies' and the skinned points' new positions.
    void LocalDeformableBundleAdjustmentEmbedded(const CameraView& cam, KeyFrameWindow& w, MapView& m, const std::vector<uint8_t>& is_node, int iterations = 5) {
        const int32_t n_kf = (int32_t)w.kf_rowptr.size() - 1;
        if (n_kf < 3) return;                                              // OPT:922-924
        nrs_graph g = m.c_graph();
        std::vector<int32_t> orp((size_t)g.n_points + 1), ocol(m.col.size()), oeid(m.col.size());
        check(nrs_graph_select_neighbours(ctx_, &g, orp.data(), ocol.data(), oeid.data()));
        std::vector<int32_t> nrp((size_t)g.n_points + 1, 0), ncol, nst;
        std::vector<float> nw, nd0;
        for (int32_t p = 0; p < g.n_points; ++p) {                           // node neighbours only, GetEdges order kept
            for (int32_t a = orp[p]; a < orp[p + 1]; ++a)
                if (is_node[ocol[a]]) { ncol.push_back(ocol[a]); nw.push_back(m.e_w[oeid[a]]); nd0.push_back(m.e_d0[oeid[a]]); nst.push_back(m.e_status[oeid[a]]); }
            nrp[p + 1] = (int32_t)ncol.size();
        }
        if (ncol.empty()) { ncol.push_back(0); nw.push_back(0.f); nd0.push_back(0.f); nst.push_back(0); }
        int32_t nl = 0, ns = 0, nd = 0, nk = 0;
        check(nrs_dba_build_edges_embedded(n_kf, w.kf_rowptr.data(), w.kf_pt.data(), g.n_points, is_node.data(), nrp.data(), ncol.data(), nw.data(), nd0.data(),
                                           nst.data(), &nl, nullptr, &ns, nullptr, nullptr, &nd, nullptr, nullptr, &nk, nullptr, nullptr, nullptr));
        std::vector<int32_t> lm_obs((size_t)nl + 1), sp(2 * (size_t)ns + 2), dm(4 * (size_t)nd + 4), sk_obs((size_t)nk + 1), sk_node(11 * (size_t)nk + 11);
        std::vector<float> d0((size_t)ns + 1), dw((size_t)nd + 1);
        std::vector<double> sk_om(11 * (size_t)nk + 11);
        check(nrs_dba_build_edges_embedded(n_kf, w.kf_rowptr.data(), w.kf_pt.data(), g.n_points, is_node.data(), nrp.data(), ncol.data(), nw.data(), nd0.data(),
                                           nst.data(), &nl, lm_obs.data(), &ns, sp.data(), d0.data(), &nd, dm.data(), dw.data(), &nk, sk_obs.data(), sk_node.data(), sk_om.data()));
        std::vector<int32_t> obs_kf(w.kf_pt.size());
        for (int32_t k = 0; k < n_kf; ++k)
            for (int32_t l = w.kf_rowptr[k]; l < w.kf_rowptr[k + 1]; ++l) obs_kf[l] = k;
        std::vector<float> lxyz(3 * (size_t)nl + 3), luv(2 * (size_t)nl + 2), sxyz(3 * (size_t)nk + 3), suv(2 * (size_t)nk + 2);
        std::vector<int32_t> lkf((size_t)nl + 1), skf((size_t)nk + 1);
        for (int32_t i = 0; i < nl; ++i) { const int32_t o = lm_obs[i]; lkf[i] = obs_kf[o]; for (int c = 0; c < 3; ++c) lxyz[3 * i + c] = w.lm_xyz[3 * o + c]; luv[2 * i] = w.lm_uv[2 * o]; luv[2 * i + 1] = w.lm_uv[2 * o + 1]; }
        for (int32_t i = 0; i < nk; ++i) { const int32_t o = sk_obs[i]; skf[i] = obs_kf[o]; for (int c = 0; c < 3; ++c) sxyz[3 * i + c] = w.lm_xyz[3 * o + c]; suv[2 * i] = w.lm_uv[2 * o]; suv[2 * i + 1] = w.lm_uv[2 * o + 1]; }
        check(nrs_dba_solve_embedded(ctx_, &cam.cam, n_kf, w.poses_qt.data(), nl, lxyz.data(), lkf.data(), luv.data(), ns, sp.data(), d0.data(), nd, dm.data(), dw.data(),
                                     nk, skf.data(), suv.data(), sxyz.data(), sk_node.data(), sk_om.data(), m.scale, iterations, nullptr));
        for (int32_t i = 0; i < nl; ++i) for (int c = 0; c < 3; ++c) w.lm_xyz[3 * (size_t)lm_obs[i] + c] = lxyz[3 * i + c];      // OPT:1145-1160
        for (int32_t i = 0; i < nk; ++i) for (int c = 0; c < 3; ++c) w.lm_xyz[3 * (size_t)sk_obs[i] + c] = sxyz[3 * i + c];
    }

    // ShiTomasi::Extract(const cv::Mat&, std::vector<cv::KeyPoint>&)  features/shi_tomasi.h:45 followed by the
    // mask filter of Tracking::ExtractFeatures (tracking.cc:118-134): `keypoints` holds the frame's keypoints on
    // entry and the NEW ones (x, y) on return, `ids` their class ids.  The extractor's buffers live in the context
    // like the reference object's members; ShiTomasi(Options) = ConfigureShiTomasi.
    void ConfigureShiTomasi(int non_max_suppression_window = 5) { check(nrs_shi_configure(ctx_, non_max_suppression_window)); }
    void ExtractFeatures(const uint8_t* im, int w, int h, int stride, const uint8_t* mask, int mask_stride,
                         std::vector<float>& keypoints, std::vector<int32_t>& ids) {
        std::vector<float> held = keypoints;
        int32_t n = 0;
        std::vector<float> xy(2 * 4096);
        std::vector<int32_t> id(4096);
        for (;;) {
            check(nrs_shi_extract(ctx_, im, w, h, stride, mask, mask_stride, (int32_t)(held.size() / 2), held.data(),
                                  (int32_t)id.size(), xy.data(), id.data(), &n));
            if ((size_t)n <= id.size()) break;
            // truncated: the call has consumed ids and left its marks, like a reference Extract would; a larger
            // buffer cannot replay it.  4096 new corners per 640x480 keyframe are never reached (31x31 exclusion).
            throw std::runtime_error("nrs_shi_extract: more keypoints than the shim's buffer");
        }
        keypoints.assign(xy.begin(), xy.begin() + 2 * (size_t)n);
        ids.assign(id.begin(), id.begin() + n);
    }

    // absl::StatusOr<Eigen::Vector3f> DeformableTriangulation(TemporalBuffer&, int candidate_id, shared_ptr<CameraModel>, float)
    // g2o_optimization.h:34-37, for every candidate of Mapping::LandmarkTriangulation at once (mapping.cc:65-116):
    // status[i] = 0 (ok) or the InternalError code of include/nrs.h; xyz = the triangulated positions.
    void DeformableTriangulation(const CameraView& cam, const TemporalBufferView& tb, const std::vector<int32_t>& candidate_ids,
                                 std::vector<int32_t>& status, std::vector<float>& xyz, int min_track = 5) {
        status.assign(candidate_ids.size(), 0);
        xyz.assign(3 * candidate_ids.size(), 0.f);
        check(nrs_triangulate_batch(ctx_, &cam.cam, tb.n_frames, tb.poses.data(), tb.n_ids, tb.has_kp.data(), tb.kp_xy.data(),
                                    tb.has_lm.data(), tb.lm_xyz.data(), tb.last_status.data(), (int32_t)candidate_ids.size(),
                                    candidate_ids.data(), min_track, status.data(), xyz.data(), nullptr));
    }

    nrs_ctx* raw() { return ctx_; }
    void check_rc(int rc) { check(rc); }

private:
    void check(int rc) {
        // the reference signals trouble with LOG(FATAL) (regularization_graph.cc:93,125); the shim throws
        if (rc != NRS_OK) throw std::runtime_error(std::string("nrs: ") + nrs_last_error(ctx_));
    }
    nrs_ctx* ctx_ = nullptr;
};

inline void KeyFrameView::append_to(KeyFrameWindow& w) const {
    if (w.kf_rowptr.empty()) w.kf_rowptr.push_back(0);
    w.poses_qt.insert(w.poses_qt.end(), pose_qt, pose_qt + 7);
    w.kf_pt.insert(w.kf_pt.end(), map_index.begin(), map_index.end());
    w.lm_uv.insert(w.lm_uv.end(), uv.begin(), uv.end());
    w.lm_xyz.insert(w.lm_xyz.end(), xyz.begin(), xyz.end());
    w.kf_rowptr.push_back((int32_t)w.kf_pt.size());
}

// LucasKanadeTracker (modules/matching/lucas_kanade_tracker.h:55-70): same method names and argument meaning; the
// template caches the reference keeps as public members (Iref_, Idref_, vMeanI_, vMeanI2_, prevPts_) live in the context.
struct PhotometricInformation {           // lucas_kanade_tracker.h:38-45, all pyramid levels of one point
    float xy[2];
    std::vector<int16_t> gray, grad;
    std::vector<float> mean;
    std::vector<uint8_t> valid;
};

class LucasKanadeTracker {
public:
    // LucasKanadeTracker(cv::Size winSize, int maxLevel, int maxIters, float epsilon, float minEigThreshold)
    LucasKanadeTracker(Engine& e, int win_size = 21, int max_level = 4, int max_iters = 10, float epsilon = 1e-4f, float min_eig = 1e-4f)
        : e_(e), levels_(max_level + 1) {
        nrs_klt_config cfg{win_size, max_level, max_iters, epsilon, min_eig};
        e_.check_rc(nrs_klt_configure(e_.raw(), &cfg));
    }
    // void SetReferenceImage(cv::Mat& refIm, std::vector<cv::KeyPoint>& refPts, cv::Mat mask)
    void SetReferenceImage(const uint8_t* im, int w, int h, int stride, const std::vector<float>& ref_pts, const uint8_t* mask = nullptr) {
        e_.check_rc(nrs_klt_set_reference(e_.raw(), im, w, h, stride, mask, (int32_t)(ref_pts.size() / 2), ref_pts.data()));
    }
    // int Track(cv::Mat& newIm, std::vector<cv::KeyPoint>& nextPts, std::vector<LandmarkStatus>& status,
    //           const bool bInitialFlow, const float minSSIM, cv::Mat mask)
    int Track(const uint8_t* im, int w, int h, int stride, std::vector<float>& next_pts, std::vector<int32_t>& status,
              bool initial_flow, float min_ssim) {
        int32_t good = 0;
        e_.check_rc(nrs_klt_track(e_.raw(), im, w, h, stride, (int32_t)status.size(), next_pts.data(), status.data(), initial_flow ? 1 : 0,
                                  min_ssim, &good, nullptr));
        return good;
    }
    PhotometricInformation GetPhotometricInformationOfPoint(int idx) {
        PhotometricInformation p;
        p.gray.resize((size_t)levels_ * 441); p.grad.resize((size_t)levels_ * 882); p.mean.resize((size_t)levels_ * 2); p.valid.resize((size_t)levels_);
        e_.check_rc(nrs_klt_get_template(e_.raw(), idx, p.xy, p.gray.data(), p.grad.data(), p.mean.data(), p.valid.data()));
        return p;
    }
    void InsertPhotometricInformation(const PhotometricInformation& p) {
        e_.check_rc(nrs_klt_insert_template(e_.raw(), p.xy, p.gray.data(), p.grad.data(), p.mean.data(), p.valid.data()));
    }
    // (no reference counterpart: the photometric information of map points kept in device memory by id instead of in MapPoint --
    // ArchivePhotometricInformation at a keyframe, InsertArchived where the reference inserts a stored PhotometricInformation)
    void ArchivePhotometricInformation(const std::vector<int32_t>& slots, const std::vector<int32_t>& ids) {
        e_.check_rc(nrs_klt_archive_templates(e_.raw(), (int32_t)slots.size(), slots.data(), ids.data()));
    }
    void InsertArchived(LucasKanadeTracker& from, const std::vector<int32_t>& ids, const std::vector<float>& xy) {
        e_.check_rc(nrs_klt_insert_archived(e_.raw(), from.e_.raw(), (int32_t)ids.size(), ids.data(), xy.data()));
    }
    void clear() { e_.check_rc(nrs_klt_clear(e_.raw())); }
    int size() { return nrs_klt_num_points(e_.raw()); }

private:
    Engine& e_;
    int levels_;
};

// EssentialMatrixInitialization (modules/tracking/essential_matrix_initialization.h): ChangeReference / Initialize on flat keypoint arrays.
// Initialize returns the verdict of include/nrs.h (0 = absl::OkStatus; 1 "Not enough matches"; 2 / 3 "Not enough triangulated landmarks");
// landmarks_code[i] == 0 where landmarks_position[i] holds a value (the reference's StatusOr), else the reason.
class EssentialMatrixInitialization {
public:
    struct Options {                      // essential_matrix_initialization.h Options + what the reference hard-codes
        float epipolar_threshold = 0.005f, radians_per_pixel = 0.0025f;
        int n_hypotheses = 0;             // 0 = ComputeMaxTries(0.8, 0.95) = 16
        int min_triangulated = 100;       // :401
        float max_low_parallax = 0.25f;   // :405
        bool compact_indexing = false;    // false = the inlier flags indexed as the reference writes it (include/nrs.h "the indexing quirk")
        uint64_t seed = 4;
    };
    EssentialMatrixInitialization(Engine& e, const Options& options, const CameraView& calibration) : e_(e), options_(options), cam_(calibration) {}
    // void ChangeReference(std::vector<cv::KeyPoint>& keypoints)
    void ChangeReference(const std::vector<float>& keypoints_xy) { reference_keypoints_ = keypoints_xy; }
    // absl::Status Initialize(const std::vector<cv::KeyPoint>&, const std::vector<LandmarkStatus>&, const int n_matches,
    //                         Sophus::SE3f& camera_transform_world, std::vector<absl::StatusOr<Eigen::Vector3f>>& landmarks_position)
    int Initialize(const std::vector<float>& current_keypoints_xy, const std::vector<int32_t>& keypoint_statuses, int n_matches,
                   float camera_transform_world[7], std::vector<float>& landmarks_position, std::vector<int32_t>& landmarks_code) {
        const size_t n = keypoint_statuses.size();
        if (reference_keypoints_.size() != 2 * n || current_keypoints_xy.size() != 2 * n) throw std::runtime_error("EssentialMatrixInitialization: sizes differ");
        nrs_init_options opt;
        nrs_init_options_init(&opt);
        opt.n_hypotheses = options_.n_hypotheses;
        opt.epipolar_threshold = options_.epipolar_threshold;
        opt.radians_per_pixel = options_.radians_per_pixel;
        opt.min_triangulated = options_.min_triangulated;
        opt.max_low_parallax = options_.max_low_parallax;
        opt.compact_indexing = options_.compact_indexing ? 1 : 0;
        opt.seed = options_.seed;
        landmarks_position.assign(3 * n, 0.f);
        landmarks_code.assign(n, 1);
        nrs_init_result out{};
        out.struct_size = (uint32_t)sizeof(out);
        out.xyz = landmarks_position.data();
        out.code = landmarks_code.data();
        e_.check_rc(nrs_init_essential(e_.raw(), &cam_.cam, &opt, (int32_t)n, reference_keypoints_.data(), current_keypoints_xy.data(),
                                       keypoint_statuses.data(), n_matches, nullptr, &out));
        for (int i = 0; i < 7; ++i) camera_transform_world[i] = out.pose_qt[i];
        last_ = out;
        last_.xyz = nullptr; last_.code = nullptr;
        return out.verdict;
    }
    const nrs_init_result& last() const { return last_; }   // score, counters, E of the last call (no arrays)

private:
    Engine& e_;
    Options options_;
    CameraView cam_;
    std::vector<float> reference_keypoints_;
    nrs_init_result last_{};
};

// Tracking::StereoMapInitialization (modules/tracking/tracking.cc:216-263) on flat arrays: the stereo matcher, the depth gate, Dbscan3D and
// the selection of the winning class in one call (include/nrs.h nrs_init_stereo).  Initialize returns the verdict (0 ok; 1 no keypoint
// passed the gate); the caller then inserts one map point per selected keypoint with status TRACKED_WITH_3D, builds the graph at 10.5 and
// makes the keyframe (:254-288).  Images are grey bytes, strides in bytes.
class StereoMapInitialization {
public:
    struct Options {                      // what the reference hard-codes (tracking.cc:226-233, dbscan.cc:63)
        float bf = 3886.37f, z_min = 35.5f, z_max = 70.5f;
        double eps = 2.5;
        int min_points = 5;
        bool noise_competes = true;       // the reference's std::map counts noise as a class
    };
    StereoMapInitialization(Engine& e, const Options& options, const CameraView& calibration) : e_(e), options_(options), cam_(calibration) {}
    int Initialize(const uint8_t* im_left, const uint8_t* im_right, int w, int h, int stride_left, int stride_right,
                   const std::vector<float>& keypoints_xy, std::vector<int32_t>& selected, std::vector<float>& landmarks_position,
                   std::vector<int32_t>& keypoint_code) {
        const size_t n = keypoints_xy.size() / 2;
        nrs_init_stereo_options opt;
        nrs_init_stereo_options_init(&opt);
        opt.bf = options_.bf; opt.z_min = options_.z_min; opt.z_max = options_.z_max;
        opt.eps = options_.eps; opt.min_points = options_.min_points; opt.noise_competes = options_.noise_competes ? 1 : 0;
        selected.assign(n, -1);
        landmarks_position.assign(3 * n, 0.f);
        keypoint_code.assign(n, 1);
        nrs_init_stereo_result out{};
        out.struct_size = (uint32_t)sizeof(out);
        out.selected = selected.data();
        out.selected_xyz = landmarks_position.data();
        out.code = keypoint_code.data();
        e_.check_rc(nrs_init_stereo(e_.raw(), &cam_.cam, &opt, im_left, im_right, w, h, stride_left, stride_right, (int32_t)n, keypoints_xy.data(), &out));
        selected.resize((size_t)out.n_selected);
        landmarks_position.resize(3 * (size_t)out.n_selected);
        last_ = out;
        last_.selected = nullptr; last_.selected_xyz = nullptr; last_.code = nullptr;
        return out.verdict;
    }
    const nrs_init_stereo_result& last() const { return last_; }   // the counts and the median depth of the last call (no arrays)

private:
    Engine& e_;
    Options options_;
    CameraView cam_;
    nrs_init_stereo_result last_{};
};

// RegularizationGraph (modules/map/regularization_graph.h:34-96) at the reference's all-pairs density, device resident.
// Point "ids" are indices 0 .. capacity-1 (the shim keeps the MapPoint ID <-> index map, as it does for frames).
class RegularizationGraph {
public:
    struct Neighbour { int32_t id; float weight, first_distance; int32_t status; };
    RegularizationGraph(Engine& e, int capacity, float weight_sigma, float streching_th) : e_(e), cap_(capacity) {
        e_.check_rc(nrs_rgraph_create(e_.raw(), capacity, weight_sigma, streching_th, &g_));
    }
    ~RegularizationGraph() { nrs_rgraph_destroy(g_); }
    RegularizationGraph(const RegularizationGraph&) = delete;
    RegularizationGraph& operator=(const RegularizationGraph&) = delete;
    void SetSigma(float sigma) { e_.check_rc(nrs_rgraph_set_sigma(g_, sigma)); }
    float GetMinWeightAllowed() const { return nrs_rgraph_min_weight(g_); }
    // AddEdge(id, other, relative_position) for every (new, other) pair; positions = capacity x 3, by index
    void AddEdges(const std::vector<float>& positions, const std::vector<int32_t>& new_ids, const std::vector<int32_t>& other_ids) {
        e_.check_rc(nrs_rgraph_add_edges(g_, positions.data(), (int32_t)new_ids.size(), new_ids.data(), (int32_t)other_ids.size(), other_ids.data()));
    }
    // int UpdateVertex(ID) for each listed vertex: returns the good-connection counts
    std::vector<int32_t> UpdateVertices(const std::vector<float>& last_world_positions, const std::vector<int32_t>& ids) {
        std::vector<int32_t> good(ids.size());
        e_.check_rc(nrs_rgraph_update(g_, last_world_positions.data(), (int32_t)ids.size(), ids.data(), good.data()));
        return good;
    }
    // std::vector<std::pair<ID, shared_ptr<Edge>>> GetEdges(ID) for each listed vertex
    std::vector<std::vector<Neighbour>> GetEdges(const std::vector<int32_t>& ids, int cap_per_point = 256) {
        const size_t n = ids.size(), no = n * (size_t)cap_per_point;
        std::vector<int32_t> cnt(n), col(no), st(no);
        std::vector<float> w(no), d0(no);
        e_.check_rc(nrs_rgraph_get_edges(g_, (int32_t)n, ids.data(), cap_per_point, cnt.data(), col.data(), w.data(), d0.data(), st.data()));
        std::vector<std::vector<Neighbour>> out(n);
        for (size_t r = 0; r < n; ++r)
            for (int k = 0; k < cnt[r] && k < cap_per_point; ++k) out[r].push_back({col[r * cap_per_point + k], w[r * cap_per_point + k], d0[r * cap_per_point + k], st[r * cap_per_point + k]});
        return out;
    }

    nrs_rgraph* raw() { return g_; }
    int capacity() const { return cap_; }

private:
    Engine& e_;
    int cap_;
    nrs_rgraph* g_ = nullptr;
};

// Masker (modules/masking/masker.{h,cc}) + System::ImageProcessing (SLAM/system.cc:189-201) on the device front end (include/nrs.h f5).
// loadFromTxt reads the reference's filters.txt (masker.cc:32-69): "BorderFilter rb re cb ce th", "BrightFilter th", "Predefined path";
// other lines are skipped, as there.  Decoding the predefined image stays with the caller (cv::imread(path, IMREAD_GRAYSCALE) in a
// drop-in): loadFromTxt hands every path to `decode`, which fills the bytes (rows packed) and the size.
class Masker {
public:
    struct Filter {
        int32_t kind = NRS_FRONT_BRIGHT;
        int32_t p[5] = {0, 0, 0, 0, 0};
        std::string name;                 // Filter::GetFilterName(): the key of the mask in GetAllMasks
        std::string path;                 // Predefined: as written in the file
        std::vector<uint8_t> mask;        // Predefined: w x h bytes
        int32_t w = 0, h = 0;
    };
    using Decoder = std::function<bool(const std::string& path, std::vector<uint8_t>& bytes, int32_t& w, int32_t& h)>;
    using Masks = std::map<std::string, std::vector<uint8_t>>;

    // the three line forms, no device involved
    static std::vector<Filter> ParseFilters(std::istream& in) {
        std::vector<Filter> out;
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ss(line);
            std::string name;
            ss >> name;
            Filter f;
            if (name == "BorderFilter") {
                std::string v[5];
                ss >> v[0] >> v[1] >> v[2] >> v[3] >> v[4];
                f.kind = NRS_FRONT_BORDER; f.name = "BorderFilter";
                for (int i = 0; i < 5; ++i) f.p[i] = std::stoi(v[i]);
            } else if (name == "BrightFilter") {
                std::string th;
                ss >> th;
                f.kind = NRS_FRONT_BRIGHT; f.name = "BrightFilter";
                f.p[0] = std::stoi(th);
            } else if (name == "Predefined") {
                ss >> f.path;
                f.kind = NRS_FRONT_PREDEFINED; f.name = "PredefinedFilter";
            } else {
                continue;
            }
            out.push_back(f);
        }
        return out;
    }

    explicit Masker(Engine& e, float clahe_clip = 3.0f) : e_(e), clip_(clahe_clip) {}

    void loadFromTxt(const std::string& path, const Decoder& decode = nullptr) {
        std::ifstream file(path);
        if (!file.is_open()) return;                                   // (the reference loads nothing, silently)
        for (Filter& f : ParseFilters(file)) {
            if (f.kind == NRS_FRONT_PREDEFINED && (!decode || !decode(f.path, f.mask, f.w, f.h)))
                throw std::runtime_error("Masker: cannot decode the predefined mask " + f.path);
            filters_.push_back(std::move(f));
        }
        configured_ = false;
    }
    void addFilter(Filter f) { filters_.push_back(std::move(f)); configured_ = false; }
    void deleteFilter(size_t idx) { filters_.erase(filters_.begin() + (long)idx); configured_ = false; }
    const std::vector<Filter>& filters() const { return filters_; }

    // System::ImageProcessing + Masker::GetAllMasks of one frame (SLAM/system.cc:113-122) in one upload: the masks by filter name plus
    // "Global"; gray / clahe (nullable) receive im_gray and the processed image.  Afterwards the tracker's *_front calls run on the
    // resident frame.
    Masks ProcessFrame(const uint8_t* im, int32_t w, int32_t h, int32_t stride, int32_t channels, std::vector<uint8_t>* gray = nullptr,
                       std::vector<uint8_t>* clahe = nullptr) {
        configure();
        const size_t n = (size_t)w * h;
        std::vector<std::vector<uint8_t>> m(filters_.size(), std::vector<uint8_t>(n));
        std::vector<uint8_t*> ptr;
        for (auto& v : m) ptr.push_back(v.data());
        std::vector<uint8_t> global(n);
        if (gray) gray->resize(n);
        if (clahe) clahe->resize(n);
        e_.check_rc(nrs_front_process(e_.raw(), im, w, h, stride, channels, gray ? gray->data() : nullptr, clahe ? clahe->data() : nullptr,
                                      global.data(), ptr.empty() ? nullptr : ptr.data()));
        Masks all;
        for (size_t i = 0; i < filters_.size(); ++i) all[filters_[i].name] = std::move(m[i]);   // (a later filter of the same name replaces the earlier one)
        all["Global"] = std::move(global);
        return all;
    }
    // absl::flat_hash_map<std::string, cv::Mat> GetAllMasks(const cv::Mat& im)   masker.cc:94-115 (im: the grey image)
    Masks GetAllMasks(const uint8_t* im_gray, int32_t w, int32_t h, int32_t stride) { return ProcessFrame(im_gray, w, h, stride, 1); }

private:
    void configure() {
        if (configured_) return;
        std::vector<nrs_front_filter> rec(filters_.size());
        for (size_t i = 0; i < filters_.size(); ++i) {
            const Filter& f = filters_[i];
            rec[i].kind = f.kind;
            for (int j = 0; j < 5; ++j) rec[i].p[j] = f.p[j];
            rec[i].mask = f.kind == NRS_FRONT_PREDEFINED ? f.mask.data() : nullptr;
            rec[i].w = f.w; rec[i].h = f.h; rec[i].stride = f.w;
        }
        e_.check_rc(nrs_front_configure(e_.raw(), (int32_t)rec.size(), rec.empty() ? nullptr : rec.data(), clip_, 8, 8));
        configured_ = true;
    }
    Engine& e_;
    float clip_;
    std::vector<Filter> filters_;
    bool configured_ = false;
};

inline std::vector<int32_t> Engine::CameraPoseAndDeformationOptimization(const CameraView& cam, FrameView& f, MapView& m, RegularizationGraph& graph,
                                                                         int cap_per_point) {
    std::vector<int32_t> lost((size_t)graph.capacity());
    int32_t n_lost = 0;
    check(nrs_track_deform_solve_rg(ctx_, &cam.cam, graph.raw(), graph.capacity(), cap_per_point, m.last_world_position.data(), (int32_t)f.status.size(),
                                    f.map_index.data(), f.status.data(), f.uv.data(), f.pos.data(), f.pose_qt, m.scale,
                                    &f.deformation_magnitude, &n_lost, lost.data(), nullptr));
    lost.resize((size_t)n_lost);
    return lost;
}

}  // namespace nrs_host
