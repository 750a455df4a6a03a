// a3: LocalDeformableBundleAdjustment C-ABI entry points (reference
// modules/optimization/g2o_optimization.cc:880-1161) on top of the graph LM engine.
//
// The six "upload + optimise + download" calls are lists of the same stages:
//     validate (nrs_dba_host.hpp) -> build the edge lists -> set up (BaProblem + dba_create / window_pack) -> solve_tail
// When a call drops the window an earlier call left resident (dba_free) relative to its argument checks is part of its behaviour -- after
// a refused call the earlier window either still answers or is gone:
//     nrs_dba_solve                     checks, then dba_free: a refused call leaves the earlier window
//     nrs_dba_solve_embedded            checks, then dba_free: a refused call leaves the earlier window
//     nrs_dba_solve_window              checks, then dba_free: a refused call leaves the earlier window
//     nrs_dba_solve_window_rg           checks, then dba_free: a refused call leaves the earlier window
//     nrs_dba_solve_window_embedded     dba_free, then checks: no earlier window after a refused call
//     nrs_dba_solve_window_rg_embedded  dba_free, then checks: no earlier window after a refused call
#include <algorithm>
#include <chrono>
#include <memory>
#include <vector>
#include "nrs_dba_host.hpp"
#include "nrs_engine.hpp"

namespace nrs {

void dba_free(nrs_ctx* c) {
    if (c->dba) engine_destroy(c, c->dba);
    c->dba = nullptr;
    delete c->dba_embwin;                                            // (the lists of a window nrs_dba_solve_window_embedded made)
    c->dba_embwin = nullptr;
    delete c->dba_rgwin;                                             // (what nrs_dba_solve_window_rg left next to its window)
    c->dba_rgwin = nullptr;
}

// constants of OPT:958-973 (nrs_dba_host.hpp)
void ba_constants(EngineSpec& s, float scale) {
    const nrs_dba::BaConstants k = nrs_dba::ba_constants(scale);
    s.info_reproj = k.info_reproj;
    s.delta_reproj = k.delta_reproj;
    s.info_pos = k.info_pos;
    s.info_spatial = k.info_spatial;
    s.delta_spatial = k.delta_spatial;
    s.k_spring = k.k_spring;
}

}  // namespace nrs

using namespace nrs;

static int refused(nrs_ctx* c, const nrs_dba::Refusal& r) { return r.ok() ? NRS_OK : c->fail(r.code, "%s", r.text.c_str()); }

struct SkinIn {
    int32_t n = 0; const int32_t* kf = nullptr; const float* uv = nullptr; const float* xyz = nullptr; const int32_t* node = nullptr; const double* omega = nullptr;
    int32_t total = 0, base = 0, k0 = 0, k1 = 0;                     // total > 0: a rank's slice of the window's list (EngineSpec sk_total / sk_base / sk_k0 / sk_k1)
};

// ---- the EngineSpec of a BA window, filled in ONE place from the caller's arrays; the structure owns what the spec points into.  Edges
// and skinned observations are attached afterwards
struct BaProblem {
    EngineSpec s;
    std::vector<Pose> poses;
    std::vector<double> x, sk_X0;
    std::vector<uint8_t> rflag;
    BaProblem(const nrs_camera* cam, int32_t n_kf, const double* poses_qt, int32_t n_lm, const float* lm_xyz, const int32_t* lm_kf, const float* lm_uv, float scale)
        : poses(n_kf), x(3 * (size_t)n_lm), rflag(n_lm, RF_OBS | RF_REPROJ_ACTIVE) {
        s.K = n_kf;
        s.M = n_lm;
        nrs_dba::poses_from_qt(n_kf, poses_qt, poses.data(), [](double* q) { quat_normalize(q); });   // SE3Quat ctor (se3quat.h:56-58)
        for (size_t i = 0; i < x.size(); ++i) x[i] = (double)lm_xyz[i];  // OPT:943 cast<double>
        s.poses = poses.data();
        s.x = x.data();
        s.lm_pose = lm_kf;
        s.uv = lm_uv;
        s.rflag = rflag.data();
        s.cam.model = cam->model;
        for (int i = 0; i < 8; ++i) s.cam.p[i] = cam->params[i];
        ba_constants(s, scale);
        s.delta_pos = 0.0;                  // no robust kernel on the BA springs (OPT:1057-1071)
        s.spring_form = 0;                  // PositionRegularizer Jacobian as written (position_regularizer.cc:51-60)
        s.shard = true;                     // with a communicator on the context: one window over its ranks (include/nrs.h)
    }
    BaProblem(const BaProblem&) = delete;
    BaProblem& operator=(const BaProblem&) = delete;
    // host lists, or the lists engine_build_edges_device* left on the device
    void edges(const DevEdges& e, bool on_device) {
        s.n_sp = e.n_sp; s.sp_ij = e.sp_ij; s.sp_d0 = e.sp_d0;
        s.n_dm = e.n_dm; s.dm_idx = e.dm_idx; s.dm_w = e.dm_w;
        s.edges_on_device = on_device;
    }
    void placeholder_edges() { s.n_sp = 1; s.n_dm = 1; }             // for engine_device_pack_ok only: the counts follow
    void skin(const SkinIn& sk) {           // embedded window (N2b): observations of points without a vertex
        if (sk.n <= 0 && sk.total <= 0) return;
        sk_X0.resize(3 * (size_t)sk.n + 3);                          // (+ slack: an empty slice still needs a non-null array)
        for (size_t i = 0; i < 3 * (size_t)sk.n; ++i) sk_X0[i] = (double)sk.xyz[i];
        s.sk_total = sk.total; s.sk_base = sk.base; s.sk_k0 = sk.k0; s.sk_k1 = sk.k1;
        s.n_skin = sk.n; s.sk_uv = sk.uv; s.sk_X0 = sk_X0.data(); s.sk_node = sk.node; s.sk_om = sk.omega; s.sk_pose = sk.kf;
    }
};

// the set-up of the built problem and the ranks' ONE agreement on it
static int dba_create(nrs_ctx* c, const BaProblem& p) {
    // rank-local checks and allocations can fail on one rank only: the ranks agree before the first collective
    int rc = engine_create(c, p.s, &c->arena_dba, &c->dba);
    // Every failure every rank sees alike (argument validation, more ranks than keyframes: all of them checked BEFORE any
    // rank-local work) returns without a collective; from there on a failure may be one rank's alone (err_local) and the ranks
    // agree on the outcome before the first collective of the solve.
    if (rc == NRS_OK || c->err_local) rc = comm_agree(c, rc);
    if (rc == NRS_OK) rc = engine_kft_agree(c, c->dba);           // (every rank got here: the set-up succeeded everywhere)
    if (rc != NRS_OK) dba_free(c);
    return rc;
}

static int dampers_complete(nrs_ctx* c, int32_t n_dm, const int32_t* dm_idx) {
    for (int64_t i = 0; i < 4 * (int64_t)n_dm; ++i)
        if (dm_idx[i] < 0) return c->fail(NRS_ERR_INVALID, "damper index out of range");
    return NRS_OK;
}

static int dba_upload(nrs_ctx* c, const nrs_camera* cam, int32_t n_kf, const double* poses_qt,
                      int32_t n_lm, const float* lm_xyz, const int32_t* lm_kf, const float* lm_uv,
                      int32_t n_sp, const int32_t* sp_ij, const float* sp_d0,
                      int32_t n_dm, const int32_t* dm_idx, const float* dm_w, float scale, const SkinIn& sk) {
    if (!c) return NRS_ERR_INVALID;
    if (!cam || n_kf <= 0 || n_lm <= 0 || !poses_qt || !lm_xyz || !lm_kf || !lm_uv || n_sp < 0 || n_dm < 0 ||
        (n_sp > 0 && (!sp_ij || !sp_d0)) || (n_dm > 0 && (!dm_idx || !dm_w)))
        return c->fail(NRS_ERR_INVALID, "nrs_dba_upload: bad argument");
    if (cam->model != NRS_CAM_PINHOLE && cam->model != NRS_CAM_KB8) return c->fail(NRS_ERR_INVALID, "unknown camera model %d", cam->model);
    NRS_TRY(dampers_complete(c, n_dm, dm_idx));
    dba_free(c);
    BaProblem p(cam, n_kf, poses_qt, n_lm, lm_xyz, lm_kf, lm_uv, scale);
    p.edges(DevEdges{n_sp, n_dm, sp_ij, dm_idx, sp_d0, dm_w}, false);
    p.skin(sk);
    return dba_create(c, p);
}

extern "C" int nrs_dba_upload(nrs_ctx* c, const nrs_camera* cam, int32_t n_kf, const double* poses_qt,
                              int32_t n_lm, const float* lm_xyz, const int32_t* lm_kf, const float* lm_uv,
                              int32_t n_sp, const int32_t* sp_ij, const float* sp_d0,
                              int32_t n_dm, const int32_t* dm_idx, const float* dm_w, float scale) {
    return dba_upload(c, cam, n_kf, poses_qt, n_lm, lm_xyz, lm_kf, lm_uv, n_sp, sp_ij, sp_d0, n_dm, dm_idx, dm_w, scale, SkinIn());
}

// ---- N2b: the embedded form of the window (include/nrs.h) -- vertices = the node copies, every other observation skinned
static int skin_validate(nrs_ctx* c, int32_t n_lm, const SkinIn& sk) {
    if (sk.n < 0 || (sk.n > 0 && (!sk.kf || !sk.uv || !sk.xyz || !sk.node || !sk.omega))) return c->fail(NRS_ERR_INVALID, "nrs_dba_upload_embedded: bad argument");
    for (int64_t i = 0; i < (int64_t)11 * sk.n; ++i)
        if (sk.node[i] < -1 || sk.node[i] >= n_lm) return c->fail(NRS_ERR_INVALID, "skinned observation: node copy out of range");
    return NRS_OK;
}

extern "C" int nrs_dba_upload_embedded(nrs_ctx* c, const nrs_camera* cam, int32_t n_kf, const double* poses_qt,
                                       int32_t n_lm, const float* lm_xyz, const int32_t* lm_kf, const float* lm_uv,
                                       int32_t n_sp, const int32_t* sp_ij, const float* sp_d0,
                                       int32_t n_dm, const int32_t* dm_idx, const float* dm_w,
                                       int32_t n_skin, const int32_t* sk_kf, const float* sk_uv, const float* sk_xyz,
                                       const int32_t* sk_node, const double* sk_omega, float scale) {
    if (!c) return NRS_ERR_INVALID;
    SkinIn sk;
    sk.n = n_skin; sk.kf = sk_kf; sk.uv = sk_uv; sk.xyz = sk_xyz; sk.node = sk_node; sk.omega = sk_omega;
    NRS_TRY(skin_validate(c, n_lm, sk));
    return dba_upload(c, cam, n_kf, poses_qt, n_lm, lm_xyz, lm_kf, lm_uv, n_sp, sp_ij, sp_d0, n_dm, dm_idx, dm_w, scale, sk);
}

extern "C" int nrs_dba_download_skinned(nrs_ctx* c, double* sk_xyz) {
    if (!c) return NRS_ERR_INVALID;
    if (!c->dba) return c->fail(NRS_ERR_STATE, "no BA problem uploaded");
    if (!sk_xyz) return c->fail(NRS_ERR_INVALID, "null output");
    return engine_skin_positions(c, c->dba, sk_xyz);
}

extern "C" int nrs_dba_skin_stats(nrs_ctx* c, int64_t out[3]) {
    if (!c || !out) return NRS_ERR_INVALID;
    if (!c->dba) return c->fail(NRS_ERR_STATE, "no BA problem uploaded");
    if (engine_skin_stats(c->dba, out) != NRS_OK) return c->fail(NRS_ERR_STATE, "no skinned observations on this window");
    return NRS_OK;
}

extern "C" int nrs_dba_stats(nrs_ctx* c, int64_t stats[5]) {
    if (!c || !stats) return NRS_ERR_INVALID;
    if (!c->dba) return c->fail(NRS_ERR_STATE, "no BA problem uploaded");
    engine_stats(c->dba, stats);
    return NRS_OK;
}

extern "C" int nrs_shard_plan(int32_t n_kf, int32_t n_lm, const int32_t* lm_kf, int32_t world, int32_t* kf_begin) {
    if (n_kf <= 0 || n_lm < 0 || (n_lm > 0 && !lm_kf) || world < 1 || world > n_kf || !kf_begin) return NRS_ERR_INVALID;
    std::vector<int> cnt(n_kf, 0), grp(n_kf + 1, 0);
    for (int i = 0; i < n_lm; ++i) {
        if (lm_kf[i] < 0 || lm_kf[i] >= n_kf) return NRS_ERR_INVALID;
        cnt[lm_kf[i]]++;
    }
    for (int k = 0; k < n_kf; ++k) grp[k + 1] = grp[k] + std::max(1, (cnt[k] + 255) / 256);   // rows are padded to 256 per keyframe
    shard_plan(n_kf, grp.data(), world, kf_begin);
    return NRS_OK;
}

extern "C" int nrs_dba_reset(nrs_ctx* c) {
    if (!c) return NRS_ERR_INVALID;
    if (!c->dba) return c->fail(NRS_ERR_STATE, "no BA problem uploaded");
    return engine_reset(c, c->dba);
}

extern "C" int nrs_dba_optimize(nrs_ctx* c, int32_t iters, nrs_lm_trace* trace) {
    if (!c) return NRS_ERR_INVALID;
    if (!c->dba) return c->fail(NRS_ERR_STATE, "no BA problem uploaded");
    if (trace) { trace->count = 0; trace->iterations = 0; }
    return engine_optimize(c, c->dba, iters, 0, trace);
}

static int download(nrs_ctx* c, int n_kf, double* poses_qt, double* xyz) {
    std::vector<Pose> poses(n_kf);
    NRS_TRY(engine_download(c, c->dba, poses.data(), xyz));
    if (poses_qt) nrs_dba::poses_to_qt(n_kf, poses.data(), poses_qt);
    return NRS_OK;
}

extern "C" int nrs_dba_download(nrs_ctx* c, double* poses_qt, double* lm_xyz) {
    if (!c) return NRS_ERR_INVALID;
    if (!c->dba) return c->fail(NRS_ERR_STATE, "no BA problem uploaded");
    return download(c, engine_num_poses(c->dba), poses_qt, lm_xyz);
}

// ---- the tail of every one-call solve: optimize(iters) on the resident window, the poses into poses_qt, the points back as float
// (nrs_dba_host.hpp points_to_float: the OPT:1158 cast) -- dense (idx null), or through the observation lists of an embedded window
struct PointsOut { int32_t n = 0; float* out = nullptr; const int32_t* idx = nullptr; };
static int solve_tail(nrs_ctx* c, int32_t iters, nrs_lm_trace* trace, int32_t n_kf, double* poses_qt, const PointsOut& lm, const PointsOut& skin = PointsOut()) {
    NRS_TRY(nrs_dba_optimize(c, iters, trace));
    std::vector<double> xyz((size_t)lm.n * 3), sk((size_t)skin.n * 3);
    NRS_TRY(download(c, n_kf, poses_qt, xyz.data()));
    if (skin.n > 0) NRS_TRY(engine_skin_positions(c, c->dba, sk.data()));
    nrs_dba::points_to_float(lm.n, lm.idx, xyz.data(), lm.out);
    nrs_dba::points_to_float(skin.n, skin.idx, sk.data(), skin.out);
    return NRS_OK;
}

extern "C" int nrs_dba_solve(nrs_ctx* c, const nrs_camera* cam, int32_t n_kf, double* poses_qt,
                             int32_t n_lm, float* lm_xyz, const int32_t* lm_kf, const float* lm_uv,
                             int32_t n_sp, const int32_t* sp_ij, const float* sp_d0,
                             int32_t n_dm, const int32_t* dm_idx, const float* dm_w,
                             float scale, int32_t iters, nrs_lm_trace* trace) {
    if (!c) return NRS_ERR_INVALID;
    NRS_TRY(nrs_dba_upload(c, cam, n_kf, poses_qt, n_lm, lm_xyz, lm_kf, lm_uv, n_sp, sp_ij, sp_d0, n_dm, dm_idx, dm_w, scale));
    return solve_tail(c, iters, trace, n_kf, poses_qt, PointsOut{n_lm, lm_xyz});
}

extern "C" int nrs_dba_solve_embedded(nrs_ctx* c, const nrs_camera* cam, int32_t n_kf, double* poses_qt,
                                      int32_t n_lm, float* lm_xyz, const int32_t* lm_kf, const float* lm_uv,
                                      int32_t n_sp, const int32_t* sp_ij, const float* sp_d0,
                                      int32_t n_dm, const int32_t* dm_idx, const float* dm_w,
                                      int32_t n_skin, const int32_t* sk_kf, const float* sk_uv, float* sk_xyz,
                                      const int32_t* sk_node, const double* sk_omega, float scale, int32_t iters, nrs_lm_trace* trace) {
    if (!c) return NRS_ERR_INVALID;
    NRS_TRY(nrs_dba_upload_embedded(c, cam, n_kf, poses_qt, n_lm, lm_xyz, lm_kf, lm_uv, n_sp, sp_ij, sp_d0, n_dm, dm_idx, dm_w, n_skin, sk_kf, sk_uv, sk_xyz,
                                    sk_node, sk_omega, scale));
    return solve_tail(c, iters, trace, n_kf, poses_qt, PointsOut{n_lm, lm_xyz}, PointsOut{n_skin, sk_xyz});
}

// ---- "the device packer, else the host packer" for a plain window whose problem is built: leaves c->dba set, or an error and no window.
// de: the edge lists on the device (null: none were built -- the window is not for the device packer); host_lists(DevEdges*): the same
// lists on the host, asked for only when they are needed.
//
// On a communicator every rank builds the window's edge lists on its own device and hands them to the rank-local construction.  Whatever
// happens behind the argument checks may happen on one rank alone, so every rank reaches exactly ONE agreement (comm_agree); a rank that
// reaches none or two hangs a sharded run.  Where it happens (the resident-graph form refuses a communicator: every agreement is a no-op there):
//
//     path of this rank                                                          its one agreement
//     ------------------------------------------------------------------------   ------------------------------------------------------
//     device edge build fails (window_upload, in front of this function)         right behind the failed build
//     device packer builds the window (engine_create NRS_OK)                     behind engine_create, here
//     device packer fails, may be this rank's alone (err_local)                  behind engine_create, here
//     device packer fails as on every rank (no err_local, not NRS_ERR_STATE)     none: every rank returns the same error
//     NRS_ERR_STATE (halos beyond the device path's limits): host packer         none here; in dba_create
//     no device lists, or a list is empty: host packer                           in dba_create
//     host packer, host_lists or the damper check fails                          none: decided from identical inputs, alike on every rank
//
// A rank that takes the host packer does so on its own: the same bits.
template <class HostLists> static int window_pack(nrs_ctx* c, BaProblem& p, const DevEdges* de, HostLists host_lists) {
    if (de && de->n_sp > 0 && de->n_dm > 0) {                        // (the same counts on every rank)
        p.edges(*de, true);
        int rc = engine_create(c, p.s, &c->arena_dba, &c->dba);
        if (rc != NRS_ERR_STATE) {                                   // (NRS_ERR_STATE: the window's halos exceed the device path's limits)
            if (rc == NRS_OK || c->err_local) rc = comm_agree(c, rc);
            if (rc != NRS_OK) dba_free(c);
            return rc;
        }
        dba_free(c);
    }
    DevEdges h;                                                      // host packer: the upload as nrs_dba_upload makes it
    NRS_TRY(host_lists(&h));
    NRS_TRY(dampers_complete(c, h.n_dm, h.dm_idx));
    p.edges(h, false);
    return dba_create(c, p);
}

// LocalDeformableBundleAdjustment in ONE call, as mapping.cc:57 makes it: the edge construction of OPT:927-1137 on the device,
// then the device-side problem construction and the solve.  Windows that do not qualify take nrs_dba_build_edges + nrs_dba_solve.
static int window_upload(nrs_ctx* c, const nrs_camera* cam, int32_t n_kf, const double* poses_qt, const int32_t* kf_rowptr, const int32_t* kf_pt,
                         const float* lm_xyz, const float* lm_uv, int32_t n_points, const int32_t* nbr_rowptr, const int32_t* nbr_col, const float* nbr_w,
                         const float* nbr_d0, const int32_t* nbr_status, float scale, std::vector<int32_t>& lm_kf) {
    NRS_TRY(refused(c, nrs_dba::window_validate("nrs_dba_solve_window", cam, n_kf, poses_qt, kf_rowptr, kf_pt, lm_xyz, lm_uv, n_points, nbr_rowptr, nbr_col, nbr_w,
                                                nbr_d0, nbr_status, lm_kf)));
    dba_free(c);
    BaProblem p(cam, n_kf, poses_qt, kf_rowptr[n_kf], lm_xyz, lm_kf.data(), lm_uv, scale);
    p.placeholder_edges();
    DevEdges de;
    const bool device = engine_device_pack_ok(c, p.s);
    if (device) {
        NRS_HIP(c, hipSetDevice(c->device));
        int rc = engine_build_edges_device(c, n_kf, kf_rowptr, kf_pt, lm_kf.data(), n_points, nbr_rowptr, nbr_col, nbr_w, nbr_d0, nbr_status, &de);
        if (rc != NRS_OK) { (void)comm_agree(c, rc); return rc; }
    }
    std::vector<int32_t> sp, dm;
    std::vector<float> d0, dw;
    return window_pack(c, p, device ? &de : nullptr, [&](DevEdges* h) {      // the two passes of nrs_dba_build_edges
        int32_t ns = 0, nd = 0;
        int rc = nrs_dba_build_edges(n_kf, kf_rowptr, kf_pt, n_points, nbr_rowptr, nbr_col, nbr_w, nbr_d0, nbr_status, &ns, nullptr, nullptr, &nd, nullptr, nullptr);
        if (rc != NRS_OK) return c->fail(rc, "nrs_dba_build_edges failed");
        sp.resize((size_t)2 * ns + 2); dm.resize((size_t)4 * nd + 4);               // (+ slack: empty lists still need non-null arrays)
        d0.resize((size_t)ns + 1); dw.resize((size_t)nd + 1);
        rc = nrs_dba_build_edges(n_kf, kf_rowptr, kf_pt, n_points, nbr_rowptr, nbr_col, nbr_w, nbr_d0, nbr_status, &ns, sp.data(), d0.data(), &nd, dm.data(), dw.data());
        if (rc != NRS_OK) return c->fail(rc, "nrs_dba_build_edges failed");
        *h = DevEdges{ns, nd, sp.data(), dm.data(), d0.data(), dw.data()};
        return (int)NRS_OK;
    });
}

extern "C" int nrs_dba_solve_window(nrs_ctx* c, const nrs_camera* cam, int32_t n_kf, double* poses_qt, const int32_t* kf_rowptr, const int32_t* kf_pt,
                                    float* lm_xyz, const float* lm_uv, int32_t n_points, const int32_t* nbr_rowptr, const int32_t* nbr_col,
                                    const float* nbr_w, const float* nbr_d0, const int32_t* nbr_status, float scale, int32_t iters, nrs_lm_trace* trace) {
    if (!c) return NRS_ERR_INVALID;
    std::vector<int32_t> lm_kf;
    NRS_TRY(window_upload(c, cam, n_kf, poses_qt, kf_rowptr, kf_pt, lm_xyz, lm_uv, n_points, nbr_rowptr, nbr_col, nbr_w, nbr_d0, nbr_status, scale, lm_kf));
    return solve_tail(c, iters, trace, n_kf, poses_qt, PointsOut{(int32_t)lm_kf.size(), lm_xyz});
}

// parity tap of the device edge builder: the edge lists of the resident window (built by nrs_dba_solve_window on the device)
extern "C" int nrs_dba_window_edges(nrs_ctx* c, int32_t* n_spring, int32_t* sp_ij, float* sp_d0, int32_t* n_damper, int32_t* dm_idx, float* dm_w) {
    if (!c) return NRS_ERR_INVALID;
    if (!c->dba) return c->fail(NRS_ERR_STATE, "no BA problem uploaded");
    int ns = 0, nd = 0;
    engine_edge_counts(c->dba, &ns, &nd);
    if (n_spring) *n_spring = ns;
    if (n_damper) *n_damper = nd;
    if (!sp_ij && !sp_d0 && !dm_idx && !dm_w) return NRS_OK;
    if (c->dba_rgwin && c->dba_rgwin->host_lists) {                 // nrs_dba_solve_window_rg below the device packer's threshold: the device-built lists as copied back
        const RgWindow& r = *c->dba_rgwin;
        if (sp_ij) memcpy(sp_ij, r.sp_ij.data(), sizeof(int32_t) * 2 * (size_t)ns);
        if (sp_d0) memcpy(sp_d0, r.sp_d0.data(), sizeof(float) * (size_t)ns);
        if (dm_idx) memcpy(dm_idx, r.dm_idx.data(), sizeof(int32_t) * 4 * (size_t)nd);
        if (dm_w) memcpy(dm_w, r.dm_w.data(), sizeof(float) * (size_t)nd);
        return NRS_OK;
    }
    return engine_edges_to_host(c, c->dba, sp_ij, sp_d0, dm_idx, dm_w);
}

// ---- LocalDeformableBundleAdjustment served by the device-resident all-pairs graph (include/nrs.h nrs_dba_solve_window_rg): the
// window's GetEdges calls (OPT:1029-1030) and its walks (OPT:1033-1074, 1086-1135) run on the device over the graph's own lists
// (nrs_engine_winedges.hpp win_edges_device), then the set-up and the solve of nrs_dba_solve_window.
constexpr int RG_WINDOW_FIRST_CAP = 64;                             // the first prefix length when the caller names none

// the graph-side refusals of the two resident-graph calls
static int rg_validate(nrs_ctx* c, const char* who, const nrs_rgraph* g, const char* sharded_form) {
    if (!g || rg_context(g) != c) return c->fail(NRS_ERR_INVALID, "%s: the graph is null or belongs to another context", who);
    if (c->comm) return c->fail(NRS_ERR_INVALID, "%s: not available with a communicator on the context (sharded windows take %s)", who, sharded_form);
    return NRS_OK;
}

// the device-built lists copied back into rw, for the host packer (windows below the device packer's threshold) and nrs_dba_window_edges
static int rg_lists_to_host(nrs_ctx* c, const DevEdges& de, RgWindow* rw, DevEdges* h) {
    rw->sp_ij.resize(2 * (size_t)de.n_sp + 2); rw->sp_d0.resize((size_t)de.n_sp + 1);
    rw->dm_idx.resize(4 * (size_t)de.n_dm + 4); rw->dm_w.resize((size_t)de.n_dm + 1);
    NRS_HIP(c, hipStreamSynchronize(c->stream));
    if (de.n_sp > 0) {
        NRS_HIP(c, hipMemcpy(rw->sp_ij.data(), de.sp_ij, sizeof(int) * 2 * (size_t)de.n_sp, hipMemcpyDeviceToHost));
        NRS_HIP(c, hipMemcpy(rw->sp_d0.data(), de.sp_d0, sizeof(float) * (size_t)de.n_sp, hipMemcpyDeviceToHost));
    }
    if (de.n_dm > 0) {
        NRS_HIP(c, hipMemcpy(rw->dm_idx.data(), de.dm_idx, sizeof(int) * 4 * (size_t)de.n_dm, hipMemcpyDeviceToHost));
        NRS_HIP(c, hipMemcpy(rw->dm_w.data(), de.dm_w, sizeof(float) * (size_t)de.n_dm, hipMemcpyDeviceToHost));
    }
    rw->host_lists = true;
    *h = DevEdges{de.n_sp, de.n_dm, rw->sp_ij.data(), rw->dm_idx.data(), rw->sp_d0.data(), rw->dm_w.data()};
    return NRS_OK;
}

extern "C" int nrs_dba_solve_window_rg(nrs_ctx* c, const nrs_camera* cam, int32_t n_kf, double* poses_qt, const int32_t* kf_rowptr, const int32_t* kf_pt,
                                       float* lm_xyz, const float* lm_uv, nrs_rgraph* g, int32_t cap_per_point, float scale, int32_t iters, nrs_lm_trace* trace) {
    if (!c) return NRS_ERR_INVALID;
    NRS_TRY(rg_validate(c, "nrs_dba_solve_window_rg", g, "nrs_dba_solve_window"));
    std::vector<int32_t> lm_kf;
    NRS_TRY(refused(c, nrs_dba::window_validate_kf("nrs_dba_solve_window_rg", nrs_dba::GRAPH_CAPACITY, cam, n_kf, poses_qt, kf_rowptr, kf_pt, lm_xyz, lm_uv, rg_capacity(g),
                                                   lm_kf)));
    const int32_t n_lm = kf_rowptr[n_kf];
    dba_free(c);                                                     // whatever happens below, no earlier window stays resident
    NRS_HIP(c, hipSetDevice(c->device));
    std::unique_ptr<RgWindow> rw(new RgWindow());
    DevEdges de;
    NRS_TRY(engine_build_edges_device_rg(c, n_kf, kf_rowptr, kf_pt, lm_kf.data(), g, cap_per_point > 0 ? cap_per_point : RG_WINDOW_FIRST_CAP, &de, rw->stats));
    BaProblem p(cam, n_kf, poses_qt, n_lm, lm_xyz, lm_kf.data(), lm_uv, scale);
    p.placeholder_edges();
    // the host packer gets the same lists, so the same bits as nrs_dba_solve_window on the full lists
    NRS_TRY(window_pack(c, p, engine_device_pack_ok(c, p.s) ? &de : nullptr, [&](DevEdges* h) { return rg_lists_to_host(c, de, rw.get(), h); }));
    c->dba_rgwin = rw.release();
    return solve_tail(c, iters, trace, n_kf, poses_qt, PointsOut{n_lm, lm_xyz});
}

extern "C" int nrs_dba_window_rg_stats(nrs_ctx* c, int64_t out[4]) {
    if (!c || !out) return NRS_ERR_INVALID;
    if (!c->dba || !c->dba_rgwin) return c->fail(NRS_ERR_STATE, "the resident window was not made by nrs_dba_solve_window_rg or nrs_dba_solve_window_rg_embedded");
    for (int i = 0; i < 4; ++i) out[i] = c->dba_rgwin->stats[i];
    return NRS_OK;
}

// ---- the EMBEDDED window in one call (include/nrs.h): the lists of nrs_dba_build_edges_embedded built on the device
// (csrc/nrs_engine_embwin.hpp), handed to the set-up nrs_dba_upload_embedded runs, then optimize(iters) and the download.
// NRS_HOST_PACK=1 or empty neighbour lists take nrs_dba_build_edges_embedded instead: the same lists.  So does a communicator, unless
// NRS_SHARD_EMBWIN_DEVICE=1 is set on the context (the host builder stays the default there: tests/test_gpu_embedded_window.py holds a
// communicator to on_device = 0 and whole lists from the tap; the decision: nrs_dba_host.hpp embwin_builder).  With the switch every rank
// builds on its own device and keeps the skinned observations of its own keyframes only (a sliced list through the set-up); as in
// window_pack, whatever happens after the validation may happen on one rank alone, so every rank reaches exactly ONE agreement: after
// a failed device build, or in the upload (a rank that does not qualify takes the host builder on its own: the same bits).
static int embwin_build_host(nrs_ctx* c, int32_t n_kf, const int32_t* kf_rowptr, const int32_t* kf_pt, const int32_t* obs_kf, const float* obs_xyz, const float* obs_uv,
                             int32_t n_points, const uint8_t* is_node, const int32_t* nbr_rowptr, const int32_t* nbr_col, const float* nbr_w, const float* nbr_d0,
                             const int32_t* nbr_status, EmbWindow* w) {
    {                                                                // a node listed twice in one keyframe: refused here as on the device
        std::vector<int32_t> seen(n_points, -1);
        for (int32_t i = 0; i < kf_rowptr[n_kf]; ++i) {
            if (!is_node[kf_pt[i]]) continue;
            if (seen[kf_pt[i]] == obs_kf[i]) return c->fail(NRS_ERR_INVALID, "nrs_dba_solve_window_embedded: a map point is listed twice in one keyframe");
            seen[kf_pt[i]] = obs_kf[i];
        }
    }
    int32_t nl = 0, ns = 0, nd = 0, nk = 0;
    int rc = nrs_dba_build_edges_embedded(n_kf, kf_rowptr, kf_pt, n_points, is_node, nbr_rowptr, nbr_col, nbr_w, nbr_d0, nbr_status, &nl, nullptr, &ns, nullptr, nullptr,
                                          &nd, nullptr, nullptr, &nk, nullptr, nullptr, nullptr);
    if (rc != NRS_OK) return c->fail(rc, "nrs_dba_build_edges_embedded failed");
    w->on_device = 0; w->n_obs = kf_rowptr[n_kf]; w->n_lm = nl; w->n_sp = ns; w->n_dm = nd; w->n_skin = nk;
    w->sk_base = 0; w->sk_held = nk; w->k0 = 0; w->k1 = n_kf;
    w->host.assign(embwin_bytes(nl, ns, nd, nk, nk), 0);
    embwin_bind(w, w->host.data());
    rc = nrs_dba_build_edges_embedded(n_kf, kf_rowptr, kf_pt, n_points, is_node, nbr_rowptr, nbr_col, nbr_w, nbr_d0, nbr_status, &nl, w->lm_obs, &ns, w->sp_ij, w->sp_d0,
                                      &nd, w->dm_idx, w->dm_w, &nk, w->sk_obs, w->sk_node, w->sk_omega);
    if (rc != NRS_OK) return c->fail(rc, "nrs_dba_build_edges_embedded failed");
    nrs_dba::gather_obs(nl, w->lm_obs, obs_xyz, obs_uv, obs_kf, w->lm_xyz, w->lm_uv, w->lm_kf);
    nrs_dba::gather_obs(nk, w->sk_obs, obs_xyz, obs_uv, obs_kf, w->sk_xyz, w->sk_uv, w->sk_kf);
    return NRS_OK;
}

// what the two embedded window calls share once their lists are built: the set-up nrs_dba_upload_embedded runs (sliced: this rank's
// share of the skinned list, valid by construction), the windows' records for the taps, then the tail with obs_xyz written through
// lm_obs / sk_obs.  rw: what the resident-graph form leaves for nrs_dba_window_rg_stats (null: the CSR form)
static int embwin_finish(nrs_ctx* c, StageTimer& mark, const nrs_camera* cam, int32_t n_kf, double* poses_qt, float* obs_xyz, float scale, int32_t iters,
                         nrs_lm_trace* trace, std::unique_ptr<EmbWindow> w, bool sliced, std::unique_ptr<RgWindow> rw) {
    mark("construction");
    SkinIn sk;
    sk.n = sliced ? w->sk_held : w->n_skin; sk.kf = w->sk_kf; sk.uv = w->sk_uv; sk.xyz = w->sk_xyz; sk.node = w->sk_node; sk.omega = w->sk_omega;
    if (sliced) { sk.total = w->n_skin; sk.base = w->sk_base; sk.k0 = w->k0; sk.k1 = w->k1; }
    else NRS_TRY(skin_validate(c, w->n_lm, sk));
    NRS_TRY(dba_upload(c, cam, n_kf, poses_qt, w->n_lm, w->lm_xyz, w->lm_kf, w->lm_uv, w->n_sp, w->sp_ij, w->sp_d0, w->n_dm, w->dm_idx, w->dm_w, scale, sk));
    const EmbWindow& r = *(c->dba_embwin = w.release());             // both taps answer: nrs_dba_window_edges_embedded and nrs_dba_window_rg_stats
    c->dba_rgwin = rw.release();
    mark.synced("set-up");
    NRS_TRY(solve_tail(c, iters, trace, n_kf, poses_qt, PointsOut{r.n_lm, obs_xyz, r.lm_obs}, PointsOut{r.n_skin, obs_xyz, r.sk_obs}));
    mark("solve + download");
    return NRS_OK;
}

extern "C" int nrs_dba_solve_window_embedded(nrs_ctx* c, const nrs_camera* cam, int32_t n_kf, double* poses_qt, const int32_t* kf_rowptr, const int32_t* kf_pt,
                                             float* obs_xyz, const float* obs_uv, int32_t n_points, const uint8_t* is_node, const int32_t* nbr_rowptr,
                                             const int32_t* nbr_col, const float* nbr_w, const float* nbr_d0, const int32_t* nbr_status, float scale, int32_t iters,
                                             nrs_lm_trace* trace) {
    if (!c) return NRS_ERR_INVALID;
    dba_free(c);                                                     // whatever happens below, no earlier window stays resident
    std::vector<int32_t> obs_kf;
    NRS_TRY(refused(c, nrs_dba::window_validate("nrs_dba_solve_window_embedded", cam, n_kf, poses_qt, kf_rowptr, kf_pt, obs_xyz, obs_uv, n_points, nbr_rowptr, nbr_col,
                                                nbr_w, nbr_d0, nbr_status, obs_kf)));
    if (!is_node) return c->fail(NRS_ERR_INVALID, "nrs_dba_solve_window_embedded: bad argument");
    StageTimer mark{c, "embedded window", false, 14};
    std::unique_ptr<EmbWindow> w(new EmbWindow);
    const nrs_dba::EmbwinBuilder by = nrs_dba::embwin_builder(c->comm != nullptr, c->comm ? c->comm->world : 1, n_kf, c->dbg.is_set(SW_SHARD_EMBWIN_DEVICE),
                                                              c->dbg.is_set(SW_HOST_PACK), nbr_rowptr[n_points] > 0);
    if (by.device) {
        bool duplicate = false;
        int rc = engine_build_embedded_window_device(c, n_kf, kf_rowptr, kf_pt, obs_kf.data(), obs_xyz, obs_uv, n_points, is_node, nbr_rowptr, nbr_col, nbr_w, nbr_d0,
                                                     nbr_status, by.shard, w.get(), &duplicate);
        if (rc != NRS_OK) { (void)comm_agree(c, rc); return rc; }
        // (decided from identical inputs: the same refusal on every rank, before any agreement)
        if (duplicate) return c->fail(NRS_ERR_INVALID, "nrs_dba_solve_window_embedded: a map point is listed twice in one keyframe");
    } else
        NRS_TRY(embwin_build_host(c, n_kf, kf_rowptr, kf_pt, obs_kf.data(), obs_xyz, obs_uv, n_points, is_node, nbr_rowptr, nbr_col, nbr_w, nbr_d0, nbr_status, w.get()));
    const bool sliced = w->on_device && by.shard;
    return embwin_finish(c, mark, cam, n_kf, poses_qt, obs_xyz, scale, iters, trace, std::move(w), sliced, nullptr);
}

// ---- the embedded window served by the device-resident graph (include/nrs.h nrs_dba_solve_window_rg_embedded): the marking, the
// GetEdges rounds and the walks of nrs_dba_solve_window_rg over node copies and skinned observations (csrc/nrs_engine_embwin.hpp
// engine_build_embedded_window_device_rg), then the set-up and the solve of nrs_dba_solve_window_embedded.
extern "C" int nrs_dba_solve_window_rg_embedded(nrs_ctx* c, const nrs_camera* cam, int32_t n_kf, double* poses_qt, const int32_t* kf_rowptr, const int32_t* kf_pt,
                                                float* obs_xyz, const float* obs_uv, nrs_rgraph* g, const uint8_t* is_node, int32_t cap_per_point, float scale,
                                                int32_t iters, nrs_lm_trace* trace) {
    if (!c) return NRS_ERR_INVALID;
    dba_free(c);                                                     // whatever happens below, no earlier window stays resident
    NRS_TRY(rg_validate(c, "nrs_dba_solve_window_rg_embedded", g, "nrs_dba_solve_window_embedded"));
    std::vector<int32_t> obs_kf;
    NRS_TRY(refused(c, nrs_dba::window_validate_kf("nrs_dba_solve_window_rg_embedded", nrs_dba::GRAPH_CAPACITY, cam, n_kf, poses_qt, kf_rowptr, kf_pt, obs_xyz, obs_uv,
                                                   rg_capacity(g), obs_kf)));
    if (!is_node) return c->fail(NRS_ERR_INVALID, "nrs_dba_solve_window_rg_embedded: bad argument");
    StageTimer mark{c, "embedded window (rg)", false, 14};
    std::unique_ptr<EmbWindow> w(new EmbWindow);
    std::unique_ptr<RgWindow> rw(new RgWindow());
    bool duplicate = false;
    NRS_TRY(engine_build_embedded_window_device_rg(c, n_kf, kf_rowptr, kf_pt, obs_kf.data(), obs_xyz, obs_uv, g, is_node,
                                                   cap_per_point > 0 ? cap_per_point : RG_WINDOW_FIRST_CAP, w.get(), &duplicate, rw->stats));
    if (duplicate) return c->fail(NRS_ERR_INVALID, "nrs_dba_solve_window_rg_embedded: a map point is listed twice in one keyframe");
    return embwin_finish(c, mark, cam, n_kf, poses_qt, obs_xyz, scale, iters, trace, std::move(w), false, std::move(rw));
}

// parity tap of the device list builder: the lists of the resident window nrs_dba_solve_window_embedded made
extern "C" int nrs_dba_window_edges_embedded(nrs_ctx* c, int32_t* on_device, int32_t* n_lm, int32_t* lm_obs, int32_t* n_spring, int32_t* sp_ij, float* sp_d0,
                                             int32_t* n_damper, int32_t* dm_idx, float* dm_w, int32_t* n_skin, int32_t* sk_obs, int32_t* sk_node, double* sk_omega) {
    if (!c) return NRS_ERR_INVALID;
    if (!c->dba || !c->dba_embwin) return c->fail(NRS_ERR_STATE, "the resident window was not made by nrs_dba_solve_window_embedded or nrs_dba_solve_window_rg_embedded");
    const EmbWindow& r = *c->dba_embwin;
    if (on_device) *on_device = r.on_device;
    if (n_lm) *n_lm = r.n_lm;
    if (n_spring) *n_spring = r.n_sp;
    if (n_damper) *n_damper = r.n_dm;
    if (n_skin) *n_skin = r.n_skin;
    if (lm_obs) memcpy(lm_obs, r.lm_obs, sizeof(int32_t) * (size_t)r.n_lm);
    if (sp_ij) memcpy(sp_ij, r.sp_ij, sizeof(int32_t) * 2 * (size_t)r.n_sp);
    if (sp_d0) memcpy(sp_d0, r.sp_d0, sizeof(float) * (size_t)r.n_sp);
    if (dm_idx) memcpy(dm_idx, r.dm_idx, sizeof(int32_t) * 4 * (size_t)r.n_dm);
    if (dm_w) memcpy(dm_w, r.dm_w, sizeof(float) * (size_t)r.n_dm);
    if (sk_obs) memcpy(sk_obs, r.sk_obs, sizeof(int32_t) * (size_t)r.n_skin);
    if (sk_node) memcpy(sk_node, r.sk_node, sizeof(int32_t) * 11 * (size_t)r.sk_held);          // (a sliced rank: its rows, nrs_dba_window_slice_embedded)
    if (sk_omega) memcpy(sk_omega, r.sk_omega, sizeof(double) * 11 * (size_t)r.sk_held);
    return NRS_OK;
}

extern "C" int nrs_dba_window_slice_embedded(nrs_ctx* c, int64_t out[6]) {
    if (!c || !out) return NRS_ERR_INVALID;
    if (!c->dba || !c->dba_embwin) return c->fail(NRS_ERR_STATE, "the resident window was not made by nrs_dba_solve_window_embedded or nrs_dba_solve_window_rg_embedded");
    const EmbWindow& r = *c->dba_embwin;
    out[0] = r.sk_base; out[1] = r.sk_held; out[2] = r.k0; out[3] = r.k1; out[4] = (int64_t)r.bytes; out[5] = (int64_t)r.sk_bytes;
    return NRS_OK;
}

extern "C" int nrs_shard_plan_counts(int32_t n_kf, const int32_t* kf_vertices, int32_t world, int32_t* kf_begin) {
    if (n_kf <= 0 || !kf_vertices || world < 1 || world > n_kf || !kf_begin) return NRS_ERR_INVALID;
    for (int k = 0; k < n_kf; ++k) if (kf_vertices[k] < 0) return NRS_ERR_INVALID;
    for (int r = 0; r < world; ++r) { int k0, k1; embwin_own_range(n_kf, kf_vertices, world, r, &k0, &k1); kf_begin[r] = k0; kf_begin[r + 1] = k1; }
    return NRS_OK;
}

extern "C" int nrs_dba_residuals(nrs_ctx* c, double* r_reproj, double* r_spring, double* r_damper) {
    if (!c) return NRS_ERR_INVALID;
    if (!c->dba) return c->fail(NRS_ERR_STATE, "no BA problem uploaded");
    if (!r_reproj || !r_spring || !r_damper) return c->fail(NRS_ERR_INVALID, "null output");
    return engine_residuals(c, c->dba, r_reproj, r_spring, r_damper);
}

extern "C" int nrs_dba_gradient(nrs_ctx* c, double* b, double* diag) {
    if (!c) return NRS_ERR_INVALID;
    if (!c->dba) return c->fail(NRS_ERR_STATE, "no BA problem uploaded");
    if (!b || !diag) return c->fail(NRS_ERR_INVALID, "null output");
    return engine_gradient(c, c->dba, b, diag);
}

extern "C" int nrs_debug_kft(nrs_ctx* c, double lam, int32_t what, int32_t k, const double* in_d, double* out_d, int32_t* out_i) {
    if (!c) return NRS_ERR_INVALID;
    if (!c->dba) return c->fail(NRS_ERR_STATE, "no BA problem uploaded");
    if ((what == 0 || what == 4 || what == 5) ? !out_i : !out_d) return c->fail(NRS_ERR_INVALID, "null output");
    if (what == 3 && !in_d) return c->fail(NRS_ERR_INVALID, "null input");
    return engine_kft_debug(c, c->dba, lam, what, k, in_d, out_d, out_i);
}

extern "C" int nrs_dba_pack_hash(nrs_ctx* c, uint64_t* out) {
    if (!c) return NRS_ERR_INVALID;
    if (!c->dba) return c->fail(NRS_ERR_STATE, "no BA problem uploaded");
    if (!out) return c->fail(NRS_ERR_INVALID, "null output");
    return engine_pack_hash(c, c->dba, out);
}

// parity tap (include/nrs.h): an explicit one-pose / n-row block system through the engine's PCG kernels
extern "C" int nrs_debug_pcg_solve(nrs_ctx* c, int32_t n_rows, const double* Hpp21, const double* bp, const double* D6,
                                   const double* Hpl18, const double* bl, double lambda, double* x, int32_t* iters) {
    if (!c) return NRS_ERR_INVALID;
    if (n_rows <= 0 || !Hpp21 || !bp || !D6 || !Hpl18 || !bl || !x || !(lambda >= 0)) return c->fail(NRS_ERR_INVALID, "nrs_debug_pcg_solve: bad argument");
    EngineSpec s;
    s.K = 1; s.M = n_rows;
    Pose id;
    id.q[0] = id.q[1] = id.q[2] = 0; id.q[3] = 1; id.t[0] = id.t[1] = id.t[2] = 0;
    std::vector<double> xs(3 * (size_t)n_rows);
    for (int i = 0; i < n_rows; ++i) { xs[3 * i] = i; xs[3 * i + 1] = 0; xs[3 * i + 2] = 1; }
    std::vector<int> lm_pose(n_rows, 0);
    std::vector<float> uv(2 * (size_t)n_rows, 0.f);
    std::vector<uint8_t> rflag(n_rows, 0);
    s.poses = &id; s.x = xs.data(); s.lm_pose = lm_pose.data(); s.uv = uv.data(); s.rflag = rflag.data();
    s.cam.model = NRS_CAM_PINHOLE;
    for (int i = 0; i < 8; ++i) s.cam.p[i] = 1.f;
    ba_constants(s, 1.f);
    s.force_gather = true;
    Engine* e = nullptr;
    Arena arena;
    nrs::Comm* keep = c->comm;
    c->comm = nullptr;                                               // never sharded
    int rc = engine_create(c, s, &arena, &e);
    int it = 0, ok = 0;
    if (rc == NRS_OK) rc = engine_debug_solve(c, e, Hpp21, bp, D6, Hpl18, bl, lambda, x, x + 6, &it, &ok);
    if (e) engine_destroy(c, e);
    arena.mem.reset();
    c->comm = keep;
    if (iters) *iters = it;
    if (rc == NRS_OK && !ok) return c->fail(NRS_ERR_NUMERIC, "debug solve: not positive definite or not converged after %d iterations", it);
    return rc;
}

extern "C" int nrs_debug_nd_solve(nrs_ctx* c, int32_t n_nodes, const double* pos, const uint8_t* last, int32_t n_pairs, const int32_t* pairs,
                                  const double* Dn, const double* Vp, const double* bn, double lambda, int32_t repeats, double* x, int64_t* stats,
                                  double* ms_per_solve) {
    if (!c) return NRS_ERR_INVALID;
    if (n_nodes <= 0 || n_pairs < 0 || !pos || (n_pairs > 0 && (!pairs || !Vp)) || !Dn || !bn || !x || repeats < 0)
        return c->fail(NRS_ERR_INVALID, "nrs_debug_nd_solve: bad argument");
    return engine_nd_debug_solve(c, n_nodes, pos, last, n_pairs, pairs, Dn, Vp, bn, lambda, repeats, x, stats, ms_per_solve);
}

extern "C" int nrs_debug_nd_cache_stats(nrs_ctx* c, int64_t out[2]) {
    if (!c || !out) return NRS_ERR_INVALID;
    nd_cache_stats(c, out);
    return NRS_OK;
}
