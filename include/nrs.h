/* nrs.h -- C ABI of the MI355X-native NR-SLAM hot path (libnrs_hip.so).
 *
 * The reference (endomapper/NR-SLAM) has no FFI; its seam is a handful of C++ free functions and
 * two classes.  Each entry point below replaces the *body* of one of them; the C++
 * shim in nr-slam_amd/host/ keeps the reference signatures, flattens Frame/Map/KeyFrame into the
 * plain arrays declared here and calls through.
 *
 * Conventions
 *   - all functions return 0 on success or a negative nrs_status; nothing throws across the ABI;
 *     nrs_last_error(ctx) gives a human-readable message for the last failure on that context.
 *   - host pointers are caller-owned and only read/written during the call; the context owns all
 *     device memory and one HIP stream; a context is NOT thread-safe (the reference calls these
 *     functions from its single main thread, modules/SLAM/system.cc:113-132).
 *   - poses are double[7] = {qx,qy,qz,qw,tx,ty,tz} of T_camera_world, i.e. what the reference
 *     hands to g2o::SE3Quat (modules/optimization/g2o_optimization.cc:68-71,165-168,907-910).
 *   - camera model: 0 = PinHole (fx fy cx cy), 1 = KannalaBrandt8 (fx fy cx cy k0 k1 k2 k3)
 *     (modules/calibration/pin_hole.cc:22-25, kannala_brandt_8.cc:25-32).
 *   - LandmarkStatus values are the reference's (modules/utilities/landmark_status.h:23-30).
 *   - there is no CPU fallback: every compute entry point fails with NRS_ERR_NO_DEVICE when no
 *     HIP device is usable.
 */
#ifndef NRS_H
#define NRS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRS_VERSION 100

typedef enum {
    NRS_OK = 0,
    NRS_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, index out of range) */
    NRS_ERR_NO_DEVICE = -2,   /* no usable HIP device / HIP runtime error at context creation    */
    NRS_ERR_HIP = -3,         /* HIP runtime error during the call (message in nrs_last_error)    */
    NRS_ERR_ALLOC = -4,       /* host or device allocation failed                                 */
    NRS_ERR_STATE = -5,       /* call sequence error (e.g. optimize before upload)                */
    NRS_ERR_NUMERIC = -6,     /* non-finite values reached the solver                             */
    NRS_ERR_COMM = -7         /* RCCL not loadable / a collective failed (message in nrs_last_error) */
} nrs_status;

typedef enum { NRS_CAM_PINHOLE = 0, NRS_CAM_KB8 = 1 } nrs_camera_model;

/* LandmarkStatus (modules/utilities/landmark_status.h:23-30) */
enum { NRS_TRACKED_WITH_3D = 0, NRS_TRACKED = 1, NRS_JUST_TRIANGULATED = 2, NRS_BAD = 3,
       NRS_OUT_IMAGE_BOUNDARIES = 4, NRS_BAD_FEATURE = 5 };

/* RegularizationGraph::Status (modules/map/regularization_graph.h:42-47) */
enum { NRS_GRAPH_VERIFIED = 0, NRS_GRAPH_NEIGHBOR = 1, NRS_GRAPH_NEUTRAL = 2, NRS_GRAPH_BAD = 3 };

typedef struct nrs_ctx nrs_ctx;

typedef struct {
    int32_t model;            /* nrs_camera_model */
    float params[8];
} nrs_camera;

 /* nrs_options grows at its END only and says how long the caller's version of it is: nrs_create reads struct_size bytes and takes
 * the defaults for everything behind them, so a binding compiled against an older header keeps working.  Fill it with
 * nrs_options_init() (device = -1, everything else 0 = default, struct_size = sizeof) or set struct_size = sizeof(nrs_options) by
 * hand; struct_size = 0 is read as the first published layout (fields up to exact_trials, 32 bytes) -- a caller that does not use
 * nrs_options_init MUST set struct_size or zero the whole struct: a value larger than 4096 is rejected as garbage (NRS_ERR_INVALID). */
typedef struct {
    int32_t device;           /* HIP device ordinal; -1 = current device                         */
    uint32_t struct_size;     /* sizeof(nrs_options) as the CALLER was compiled (sits where the layout had padding) */
    double pcg_rtol;          /* relative residual ||b-Ax||/||b|| at which the inner solve stops;
                                 0 = default 1e-10 (SURVEY.md 7.2 hard part 1)                    */
    int32_t pcg_max_iters;    /* 0 = default 2000                                                */
    int32_t pcg_batch;        /* PCG iterations enqueued between host checks; 0 = default 8       */
    int32_t profile;          /* 1 = time the linearise and SpMV kernels with HIP events on the
                                 context stream (serialises launches; for bench roofline only)    */
    int32_t exact_trials;     /* 0 (default): an LM trial whose gain ratio is already < -1 / -0.25 / -0.1 /
                                 -0.03 when the inner solve has reached 1e-1 / 1e-2 / 1e-3 / 1e-4 (and whose
                                 chi2 increase exceeds 1e-5 chi2) is rejected there.  This is a HEURISTIC with
                                 measured margins (the gain ratio of a partially converged step is
                                 within 0.15 / 0.017 / 0.004 / 0.002 of its final value at those milestones;
                                 0 decision changes in 200-problem sweeps): the step of a rejected trial is
                                 discarded and accepted steps are always solved to pcg_rtol, so the iterates
                                 are the reference's as long as no rejection is mispredicted.
                                 1: every trial is solved to pcg_rtol (g2o's behaviour; use it to verify). */
    int32_t direct_solve;     /* linear solver of the single-frame problems (nrs_track_deform_solve[_rg]):
                                 0 (default): a sparse direct solve (nested dissection, multifrontal Cholesky on the
                                 matrix cores: what LinearSolverEigen does, linear_solver_eigen.h:92-173) for frames of
                                 up to 8000 free rows (1.1 .. 4.4 x faster than the PCG at every measured size, 129 ..
                                 4525 points: DESIGN.md section 1), PCG beyond; 1: direct whenever the problem has the
                                 single-frame structure; 2: always
                                 PCG.  Same LM iterates either way (both are held to the oracle).  BA windows always
                                 use PCG.  Values outside 0..2 are read as 0. */
    int32_t embedded_solver;  /* linear solver of the EMBEDDED BA windows (nrs_dba_*_embedded):
                                 the system of an embedded window is block tridiagonal over the keyframes -- dense keyframe
                                 blocks (node copies + pose, coupled through the skinned observations), sparse damper
                                 couplings -- and can be factorised EXACTLY per LM trial (what LinearSolverEigen does for the
                                 reference, linear_solver_eigen.h:92-173): the keyframe blocks are inverted on the matrix
                                 cores along two elimination chains, and the factorisation preconditions the PCG, which then
                                 converges to pcg_rtol in one or two iterations (csrc/nrs_engine_kft.hpp).
                                 0 (default): that solver where a cost model of the two says it is the faster one (measured:
                                 5 x at 100 nodes x 20 keyframes, 2.3 x at 300, 1.24 x at 440, break-even at the literal C2 --
                                 458 node copies x 20 keyframes; the PCG wins beyond), block-Jacobi PCG else;
                                 1: always the factorisation (if its K x (3 nodes + 6)^2 x 8 bytes fit 6 GB);
                                 2: always block-Jacobi PCG (hundreds of iterations per trial).  Same LM iterates either
                                 way.  Plain windows (every point a node) use the block-Jacobi PCG.  On a context with a
                                 communicator an embedded window solves by block-Jacobi PCG whatever this says, unless
                                 sharded_kft = 1.
                                 (Sits where the 40-byte layout had padding: values outside 0..2 are read as 0.) */
    int32_t sharded_kft;      /* embedded BA windows on a context with a communicator:
                                 0 (default): block-Jacobi PCG, whatever embedded_solver says;
                                 1: embedded_solver decides as on one GPU.  The keyframe-block factorisation is then sharded:
                                 a rank holds and inverts the blocks of its own keyframes, and the elimination chains are
                                 handed from rank to rank (one Schur-update operand per crossing in the factorisation, one
                                 vector per crossing in the solve).  The factor and M^-1 x are bit-identical to one GPU's.
                                 If any rank cannot hold its share, every rank falls back to the PCG.  Values other than
                                 0 / 1 are read as 0. */
} nrs_options;
void nrs_options_init(nrs_options* opt);

/* One Levenberg-Marquardt trial as executed by g2o
 * (third_party/g2o/g2o/core/optimization_algorithm_levenberg.cpp:94-145). */
typedef struct {
    int32_t round;            /* outer round of the entry point (inlier rounds), 0 for BA         */
    int32_t iter;             /* LM iteration inside optimize()                                  */
    int32_t trial;            /* qmax at the time of the trial                                   */
    int32_t accepted;
    int32_t solver_ok;        /* 0 = linear solve reported "not positive definite"               */
    int32_t inner_iters;      /* PCG iterations of this trial (0 for dense 6x6 solves)           */
    int32_t early_rejected;   /* 1 = rejected at a peek (chi2_new / rho are the peek values) */
    int32_t reserved;
    double lambda;
    double chi2;              /* currentChi                                                      */
    double chi2_new;          /* tempChi                                                         */
    double rho;
} nrs_lm_trial;

typedef struct {
    nrs_lm_trial* trials;     /* caller-allocated, may be NULL                                   */
    int32_t capacity;
    int32_t count;            /* out: trials executed (may exceed capacity; extra are dropped)   */
    int32_t iterations;       /* out: LM iterations executed (cjIterations)                      */
} nrs_lm_trace;

/* Kernel timing accumulated while nrs_options.profile = 1 */
typedef struct {
    double linearize_ms;  int64_t linearize_launches;
    double spmv_ms;       int64_t spmv_launches;
    double vec_ms;        int64_t vec_launches;
    double update_ms;     int64_t update_launches;
} nrs_profile;

int nrs_create(nrs_ctx** out, const nrs_options* opt);

/* ---- Debug switches -----------------------------------------------------------------------------------------------------
 * None is needed in normal use.  A context reads the NRS_* variables of the environment ONCE, in nrs_create (also
 * NRS_DEBUG="NAME=VALUE,NAME2=VALUE2", names without the prefix); afterwards the library never looks at the environment again --
 * a host application may call setenv at any time -- and a switch is changed through nrs_debug_set only (value NULL: unset;
 * takes effect at the next problem upload / solve of that context).  The host edge builders, which take no context, read
 * NRS_HOST_THREADS from a process-wide snapshot taken at their first call.
 * Every switch is a row of ONE table (nr-slam_amd/csrc/nrs_switches.hpp: kind, default, group, one line on what it does); a name that is
 * not in it is accepted and does nothing.  A switch written without a value below goes by presence: it is on when set to anything, "0"
 * included (NRS_NO_LDS=0 turns the LDS path off); one written with a value is read with atoi / atof (garbage reads as 0).
 *   measurement   NRS_TIMING (stage marks of engine_create, the a2 driver and the frame-mapping entry points on stderr), NRS_ND_DBG / NRS_ND_DBG2 (phase clocks of one
 *                 direct solve through nrs_debug_nd_solve), NRS_PEEK_DEBUG (gain ratios at the early-rejection looks)
 *   checks        NRS_POISON (fresh device allocations filled with NaN patterns), NRS_CHECK_EVAL / NRS_CHECK_FUSED / NRS_CHECK_CHI (an
 *                 evaluation / a single-launch PCG iteration / the carried chi2 computed twice and compared)
 *   direct solver NRS_ND=0|1, NRS_ND_MAX_ROWS, NRS_ND_NO_CACHE, NRS_ND_NO_COVER, NRS_ND_CHAIN, NRS_ND_LEVELS, NRS_ND_THREADS=256,
 *                 NRS_ND_STEP32=0, NRS_ND_BACK_FLAGS, NRS_ND_LEAF=<n>, NRS_ND_NO_SPLIT, NRS_ND_PLAN_PAR=<n>
 *   LM trials     NRS_SPEC_TRIALS=<0..3> (shadow sets for the speculative trials of a run of rejections; 0: one at a time; read when an
 *                 engine is created), NRS_SPEC_FIXED=<n>, NRS_SPEC_FIRST=<n>, NRS_SPEC_NO_ABORT, NRS_SPEC_DBG, NRS_SPEC_MAX_ROWS=<n> (rows up
 *                 to which a BA window on the two-kernel PCG carves shadow sets; default 2^18), NRS_NO_REARM (plain windows: the PCG's
 *                 status words cleared by a fill per trial, not re-armed by k_finalize)
 *   PCG / packing NRS_NO_LDS, NRS_NO_FUSED, NRS_FUSED_MAX_ROWS=<n>, NRS_NO_COARSE, NRS_COARSE_MIN_TILES=<n>, NRS_NO_ONE_XCD, NRS_NO_ECD, NRS_HIER,
 *                 NRS_NO_PLAIN, NRS_NO_H4, NRS_RC=<0..3>, NRS_NT=0|1, NRS_DFORM, NRS_NO_EDGE_CHI, NRS_SELL_T=<lanes>, NRS_NO_MORTON,
 *                 NRS_NO_TILE_SORT, NRS_ONE_CLASS, NRS_TILE_CUT_PCT=<p>, NRS_HOST_PACK, NRS_HOST_THREADS=<n>, NRS_HOST_THREADS_SMALL=<n>,
 *                 NRS_SKIN_OP_OWN_LAUNCH, NRS_SKIN_ROWS_OWN_LAUNCH, NRS_PCG_RTOL=<r> (experiments), NRS_SHARD_EMBWIN_DEVICE (a rank of a
 *                 communicator builds its share of nrs_dba_solve_window_embedded's lists on its device; off: the host builder)
 *   embedded BA   NRS_KFT_TWO_LAUNCHES (a sweep step of the keyframe-block factorisation as two launches), NRS_KFT_SCALAR_SWEEP (the pivot
 *                 block's sweep in the 4-pivot register form), NRS_KFT_FOUR_WAVES (panel workgroups without the four helper waves), NRS_KFT_NO_RESIDUAL_TEST (M^-1 applied again after the first PCG step
 *                 instead of the step's residual tested on its own)
 *   sharding      NRS_SHARD_PACK_ALL, NRS_SHARD_FULL_VECTORS
 *   a1 / graph    NRS_PO_MULTI_MIN=<n>, NRS_PO_NO_CACHE, NRS_PO_MULTI_GROUPS=<g>, NRS_HOST_WALK, NRS_WALK_MAX_PASSES=<n>, NRS_RG_NO_MIRROR, NRS_RG_MAX_CAP=<n> (a lower limit on the GetEdges
 *                 prefix a call may ask for: the "ran off at the limit" refusals)
 *   evaluation    NRS_STEREO_NO_MFMA (nrs_stereo_match_pattern: plain integer correlation instead of the int8 matrix-core form)
 *   front end     NRS_FRONT_PER_EYE (nrs_front_process_stereo: grey and CLAHE issued per eye with the single-frame kernels instead of the
 *                 pair launches; the same bytes), NRS_RECT_OWN_LAUNCH (nrs_front_process_stereo_raw: the remap into a rectified colour
 *                 buffer and the pair's grey kernel after it, two launches instead of the fused one; the same bytes), NRS_RESIZE_OWN_LAUNCH
 *                 (nrs_front_process_raw: the resize into a colour buffer and the ordinary grey kernel after it, two launches instead of
 *                 the fused one; the same bytes)
 *   initialisation NRS_DBND_NO_TILE (nrs_dbscan_nd and nrs_flow_tracks_cluster: the neighbour stage as a wave per point with candidates
 *                 from global memory instead of the LDS tiles; the same bits)
 *   probes      (read by a `make PROBES=1` build only) NRS_LIN_DBG / NRS_SPMV_DBG / NRS_PCG_DBG (phase clocks of one lineariser /
 *                 operator / single-launch PCG iteration launch), NRS_LIN_EXP=<n> (lineariser removal experiments: wrong results on purpose)
 * (what each selects: README.md "Debug switches"; the A/B tests drive every launch form through nrs_debug_set). */
int nrs_debug_set(nrs_ctx* ctx, const char* name /* "NRS_..." */, const char* value /* NULL: unset */);
void nrs_destroy(nrs_ctx* ctx);
const char* nrs_last_error(const nrs_ctx* ctx);
int nrs_device_name(const nrs_ctx* ctx, char* buf, int32_t buf_len);
int nrs_get_profile(const nrs_ctx* ctx, nrs_profile* out);
int nrs_reset_profile(nrs_ctx* ctx);
void* nrs_stream(nrs_ctx* ctx);                 /* hipStream_t the context launches on */

/* ---- a1: CameraPoseOptimization (modules/optimization/g2o_optimization.cc:50-146) ------------
 * 3 rounds x optimize(10), restart from the seed each round, chi2 > 5.99 edges to level 1 between
 * rounds; all three rounds use the Huber kernel (the reference's setRobustKernel(0) at OPT:134-137 runs
 * after the last optimize() and has no effect on the solve).  uv: n x 2 keypoints, X: n x 3 landmark positions of
 * the TRACKED_WITH_3D observations in frame index order.  pose_qt in: frame pose, out: refined.
 * inlier (may be NULL): final classification of every edge. */
int nrs_pose_only_solve(nrs_ctx* ctx, const nrs_camera* cam, int32_t n, const float* uv,
                        const float* X, double pose_qt[7], uint8_t* inlier, nrs_lm_trace* trace);

/* ---- a3: LocalDeformableBundleAdjustment (g2o_optimization.cc:880-1161) ----------------------
 * Host-side edge construction of OPT:927-1137 from flattened keyframes and the ordered
 * neighbour lists that RegularizationGraph::GetEdges returns (a19).  kf_rowptr[n_kf+1] delimits,
 * oldest keyframe first, the map-point index of every TRACKED_WITH_3D observation in keyframe
 * index order (kf_pt).  Landmark l = position in that concatenation.  Two-call pattern: pass
 * sp_ij = NULL to obtain the counts, then call again with buffers of that size. */
int nrs_dba_build_edges(int32_t n_kf, const int32_t* kf_rowptr, const int32_t* kf_pt,
                        int32_t n_points, const int32_t* nbr_rowptr, const int32_t* nbr_col,
                        const float* nbr_w, const float* nbr_d0, const int32_t* nbr_status,
                        int32_t* n_spring, int32_t* sp_ij, float* sp_d0,
                        int32_t* n_damper, int32_t* dm_idx, float* dm_w);

/* One-shot: upload, optimize(iters), download.  lm_kf[l] = keyframe (pose index) of landmark l,
 * must be non-decreasing.  sp_ij: n_spring x 2 landmark indices; dm_idx: n_damper x 4
 * (1c,2c,1n,2n).  scale = Map::GetMapScale().  The reference calls optimize(5). */
int nrs_dba_solve(nrs_ctx* ctx, const nrs_camera* cam, int32_t n_kf, double* poses_qt,
                  int32_t n_lm, float* lm_xyz, const int32_t* lm_kf, const float* lm_uv,
                  int32_t n_spring, const int32_t* sp_ij, const float* sp_d0,
                  int32_t n_damper, const int32_t* dm_idx, const float* dm_w,
                  float scale, int32_t iters, nrs_lm_trace* trace);

/* ---- N2b: the EMBEDDED form of the window -- BASELINE configs[1] as written, "5k map points x 500 deformation-graph nodes x 20
 * keyframes".  The reference has no such estimator (its graph has a vertex per map point); this is
 * LocalDeformableBundleAdjustment (g2o_optimization.cc:880-1161) with the vertices restricted to the keyframe copies of a NODE set:
 * springs (OPT:1031-1072) and dampers (OPT:1076-1132) by the reference's walks between node copies only, and every other observed
 * point SKINNED in its keyframe to the <= 11 node copies its walk accepts, x = X0 + sum_k omega_k (x_{n_k} - x_start_{n_k}) with the
 * connection weights normalised; its ReprojectionError edge (reprojection_error.cc:32-64) keeps residual, information and Huber
 * kernel and constrains those node copies and the keyframe pose (Jacobian omega_k x the reference's block).  With every point a
 * node all of it IS the plain window (same lists, same bits); beyond that it is held to oracle/embedded_oracle.py
 * (dba_build_embedded / dba_solve_embedded), "parity unpinned".  Observation o = position in the concatenation kf_pt.
 *   nrs_dba_build_edges_embedded  host: node copies (lm_obs[n_lm]: their observation, keyframe-major), springs / dampers over
 *                                 node-copy indices, skinned observations (sk_obs, sk_node [n x 11, -1 pads], sk_omega [n x 11]);
 *                                 two-call pattern: lm_obs = NULL returns the four counts
 *   nrs_dba_upload_embedded       the window resident: lm_* of the node copies, sk_kf / sk_uv / sk_xyz of the skinned observations
 *                                 (sk_xyz = X0, their positions at the start); then nrs_dba_reset / optimize / download as before
 *   nrs_dba_download_skinned      the skinned points at the current estimate (n_skin x 3, fp64)
 *   nrs_dba_solve_embedded        one shot: upload, optimize(iters), download (poses_qt, lm_xyz, sk_xyz in/out)
 *   nrs_dba_skin_stats            out[0] skinned observations held on this context (sharded: those of its own keyframes), [1] their
 *                                 padded slots, [2] device bytes of the skin buffer they occupy (not part of nrs_dba_stats' [4]);
 *                                 NRS_ERR_STATE when no skinned observations are resident
 * The linear solve is the PCG with the observations' blocks applied as hyper-edges (csrc/nrs_engine_skin.hpp), or the keyframe-block
 * factorisation as its preconditioner (nrs_options.embedded_solver).  With a communicator the window is sharded like a plain one (the
 * multi-GPU block below). */
int nrs_dba_build_edges_embedded(int32_t n_kf, const int32_t* kf_rowptr, const int32_t* kf_pt, int32_t n_points, const uint8_t* is_node,
                                 const int32_t* nbr_rowptr, const int32_t* nbr_col, const float* nbr_w, const float* nbr_d0, const int32_t* nbr_status,
                                 int32_t* n_lm, int32_t* lm_obs, int32_t* n_spring, int32_t* sp_ij, float* sp_d0,
                                 int32_t* n_damper, int32_t* dm_idx, float* dm_w,
                                 int32_t* n_skin, int32_t* sk_obs, int32_t* sk_node, double* sk_omega);
int nrs_dba_upload_embedded(nrs_ctx* ctx, const nrs_camera* cam, int32_t n_kf, const double* poses_qt,
                            int32_t n_lm, const float* lm_xyz, const int32_t* lm_kf, const float* lm_uv,
                            int32_t n_spring, const int32_t* sp_ij, const float* sp_d0,
                            int32_t n_damper, const int32_t* dm_idx, const float* dm_w,
                            int32_t n_skin, const int32_t* sk_kf, const float* sk_uv, const float* sk_xyz,
                            const int32_t* sk_node, const double* sk_omega, float scale);
int nrs_dba_download_skinned(nrs_ctx* ctx, double* sk_xyz /* n_skin x 3, fp64 */);
int nrs_dba_skin_stats(nrs_ctx* ctx, int64_t out[3]);
int nrs_dba_solve_embedded(nrs_ctx* ctx, const nrs_camera* cam, int32_t n_kf, double* poses_qt,
                           int32_t n_lm, float* lm_xyz, const int32_t* lm_kf, const float* lm_uv,
                           int32_t n_spring, const int32_t* sp_ij, const float* sp_d0,
                           int32_t n_damper, const int32_t* dm_idx, const float* dm_w,
                           int32_t n_skin, const int32_t* sk_kf, const float* sk_uv, float* sk_xyz,
                           const int32_t* sk_node, const double* sk_omega, float scale, int32_t iters, nrs_lm_trace* trace);

/* The whole of LocalDeformableBundleAdjustment in one call, as mapping.cc:57 makes it: flattened keyframes (kf_rowptr / kf_pt as in
 * nrs_dba_build_edges; lm_xyz / lm_uv per landmark = position in that concatenation, lm_xyz in/out) + the ordered neighbour lists
 * RegularizationGraph::GetEdges returns (a19).  The edge construction of OPT:927-1137 runs on the device as well (index for index
 * the lists nrs_dba_build_edges returns), followed by the device-side problem construction and optimize(iters).  Windows that do
 * not qualify for the device path (a single keyframe, tiny windows, a communicator on the context) take nrs_dba_build_edges +
 * nrs_dba_solve internally: the result is the same.  nrs_dba_window_edges (parity tap): the edge lists of the resident window
 * when they were built on the device (two-call pattern: null arrays return the counts). */
int nrs_dba_solve_window(nrs_ctx* ctx, const nrs_camera* cam, int32_t n_kf, double* poses_qt, const int32_t* kf_rowptr,
                         const int32_t* kf_pt, float* lm_xyz, const float* lm_uv, int32_t n_points, const int32_t* nbr_rowptr,
                         const int32_t* nbr_col, const float* nbr_w, const float* nbr_d0, const int32_t* nbr_status, float scale,
                         int32_t iters, nrs_lm_trace* trace);
int nrs_dba_window_edges(nrs_ctx* ctx, int32_t* n_spring, int32_t* sp_ij, float* sp_d0, int32_t* n_damper, int32_t* dm_idx, float* dm_w);

/* The EMBEDDED window (N2b above) in one call: flattened keyframes as for nrs_dba_solve_window, obs_xyz / obs_uv per OBSERVATION
 * (position in the concatenation kf_pt), the node flags and the ordered neighbour lists.  The lists nrs_dba_build_edges_embedded
 * returns are built on the device (csrc/nrs_engine_embwin.hpp: index for index, the fp64 weights to the last bit), copied to the
 * host and handed to the set-up nrs_dba_upload_embedded runs; then optimize(iters) and the download.  There is no size threshold.
 * The host construction (nrs_dba_build_edges_embedded, the same lists) is taken with a communicator on the context, under
 * NRS_HOST_PACK=1 and for a window whose neighbour lists are empty.  A communicator takes the host builder BY DEFAULT; with
 * NRS_SHARD_EMBWIN_DEVICE=1 on the context (nrs_debug_set; collective; at most 8 ranks, no more ranks than keyframes) every rank
 * builds the lists on its own device over the same inputs and keeps the skinned observations of ITS keyframes only: node copies,
 * springs, dampers and sk_obs whole, sk_node / sk_omega and the gathered per-observation data for the slice
 * [sk_base, sk_base + sk_held) of the skinned list -- staging, host memory and set-up work of a rank follow its share (unmeasured on
 * hardware).  The set-up adds no collective; a rank that does not qualify takes the host construction on its own, with the same
 * bits in the solve.  Arguments are checked as for nrs_dba_solve_window, and is_node
 * must not be null; a NODE listed twice in one keyframe (which the reference cannot produce, frame.h:108-123, and on which a
 * sequential and a parallel walk would differ) is NRS_ERR_INVALID as well.  After an error nothing is resident.
 * On return the window is resident as after nrs_dba_upload_embedded (reset / optimize / download / download_skinned /
 * nrs_debug_kft), and obs_xyz holds, cast to float: the optimised position of every node copy, the skinned position of every
 * skinned observation; observations that reach no node copy are unchanged.
 *   nrs_dba_window_edges_embedded  parity tap: the lists of the resident window (null arrays: the four counts only); *on_device = 1
 *                                  when the device built them; NRS_ERR_STATE when the resident window was not made by this call.
 *                                  On a rank of a communicator that built its share on the device the counts are the window's, sk_obs is
 *                                  whole, and sk_node / sk_omega hold the rank's sk_held rows (the window's rows from sk_base on)
 *   nrs_dba_window_slice_embedded  of the resident window: out[0] sk_base, [1] sk_held, [2] / [3] the rank's keyframes [k0, k1),
 *                                  [4] bytes of the lists' staging, [5] bytes the five sliced skinned arrays take of it (padding
 *                                  included); a whole window: 0, n_skin, 0, n_kf */
int nrs_dba_solve_window_embedded(nrs_ctx* ctx, const nrs_camera* cam, int32_t n_kf, double* poses_qt /* in/out */,
                                  const int32_t* kf_rowptr, const int32_t* kf_pt, float* obs_xyz /* n_obs x 3, in/out */, const float* obs_uv,
                                  int32_t n_points, const uint8_t* is_node, const int32_t* nbr_rowptr, const int32_t* nbr_col, const float* nbr_w,
                                  const float* nbr_d0, const int32_t* nbr_status, float scale, int32_t iters, nrs_lm_trace* trace);
int nrs_dba_window_edges_embedded(nrs_ctx* ctx, int32_t* on_device, int32_t* n_lm, int32_t* lm_obs, int32_t* n_spring, int32_t* sp_ij,
                                  float* sp_d0, int32_t* n_damper, int32_t* dm_idx, float* dm_w, int32_t* n_skin, int32_t* sk_obs,
                                  int32_t* sk_node, double* sk_omega);
int nrs_dba_window_slice_embedded(nrs_ctx* ctx, int64_t out[6]);

/* Device-resident form of the same solve (used by bench.py so that the timed region starts with
 * the inputs already in HBM): upload once, then any number of {reset, optimize}. */
int nrs_dba_upload(nrs_ctx* ctx, const nrs_camera* cam, int32_t n_kf, const double* poses_qt,
                   int32_t n_lm, const float* lm_xyz, const int32_t* lm_kf, const float* lm_uv,
                   int32_t n_spring, const int32_t* sp_ij, const float* sp_d0,
                   int32_t n_damper, const int32_t* dm_idx, const float* dm_w, float scale);
int nrs_dba_reset(nrs_ctx* ctx);                                  /* estimates <- uploaded values */
int nrs_dba_optimize(nrs_ctx* ctx, int32_t iters, nrs_lm_trace* trace);
int nrs_dba_download(nrs_ctx* ctx, double* poses_qt, double* lm_xyz /* n_lm x 3, fp64 */);
/* Debug/parity taps on the resident problem (host buffers, fp64): per-edge residuals at the
 * current estimate and the assembled gradient b = -J^T W r in solver order (poses then landmarks). */
int nrs_dba_residuals(nrs_ctx* ctx, double* r_reproj /* n_lm x 2 */, double* r_spring /* n_spring */,
                      double* r_damper /* n_damper x 3 */);
int nrs_dba_gradient(nrs_ctx* ctx, double* b /* 6 n_kf + 3 n_lm */, double* diag /* same size */);
/* Parity tap of the embedded window's keyframe-block factorisation (nrs_options.embedded_solver = 0; csrc/nrs_engine_kft.hpp) on the resident
 * window, linearised at the current estimate with damping lam:
 *   what 0  out_i[0..6) = {in use, keyframes K, block dimension ld, ld / 64, middle keyframe, factor MiB}, then K free-node counts, K pose sizes (6 / 0)
 *   what 1  out_d = the assembled diagonal block of keyframe k (ld x ld: its free node copies in row order, then its pose)
 *   what 2  out_d = the coupling of keyframes k and k + 1 as a dense ld x ld matrix (rows: k)
 *   what 3  out_d = M^-1 in_d, both in solver order (6 per pose, then 3 per node copy): the factorisation applied as the PCG applies it
 *   what 4  out_i = per node copy its (keyframe, compact index) pair, -1: fixed
 *   what 5  out_i[0..6) = this rank's share: {first own keyframe, own keyframes, middle keyframe, rank that holds it,
 *           factor bytes held >> 10 (KiB), hand-overs per factorisation}; one GPU: {0, K, m, 0, bytes >> 10, 0}
 * On a communicator (nrs_options.sharded_kft = 1) what 0 reports as on one GPU, what 1 / 2 answer for the rank's own keyframes only
 * (NRS_ERR_INVALID on the other ranks); what 1 / 2 / 3 linearise and assemble, so every rank calls them together (the same lam and
 * k); what 3 returns the complete M^-1 in_d on every rank, the same bits everywhere. */
int nrs_debug_kft(nrs_ctx* ctx, double lam, int32_t what, int32_t k, const double* in_d, double* out_d, int32_t* out_i);

/* Parity tap of the problem construction (edge lists -> row layout, sliced-ELL incidence streams, halo lists, chi2 edge lists;
 * g2o_optimization.cc:927-1137 ends where this starts): FNV-1a checksums of every packed array of the resident problem,
 * out[0..24).  A plain BA window (>= 2 keyframes, >= 2048 padded rows, nothing fixed, no masks / offsets / unary or incomplete
 * dampers: both the two-kernel path, T = 2, and the fused one, T = 8) is packed on the device (csrc/nrs_engine_devpack.hpp) --
 * on a communicator too, where every rank builds its own share there (a sharded window is always two-kernel: T = 8 below 32768
 * rows) -- everything else on the host, as is everything under NRS_HOST_PACK=1 or any of the A/B switches the host path honours
 * (NRS_SELL_T, NRS_NO_FUSED, NRS_FUSED_MAX_ROWS, NRS_NO_PLAIN, NRS_NO_LDS, NRS_DFORM, NRS_NO_EDGE_CHI, NRS_TILE_CUT_PCT, NRS_HIER,
 * NRS_NO_ECD, NRS_SHARD_PACK_ALL); the two constructions produce the same bits (out[21] says which one ran: 1 = device; it is not
 * part of the comparison).  A rank of a sharded window that holds its own rows of the per-row arrays only hashes those rows. */
int nrs_dba_pack_hash(nrs_ctx* ctx, uint64_t* out /* 24 */);

/* Parity tap for a18 (the linear solve): solves (H + lambda I) x = b for an explicitly given block system with
 * the engine's own PCG kernels (block-Jacobi preconditioner, operator on stored blocks, single-reduction CG),
 * as g2o's linear solvers are handed an explicit SparseBlockMatrix in the reference's known-answer test
 * (third_party/g2o/unit_test/solver/linear_solver_test.cpp:72-85).  Shape: one 6x6 block H_pp (21 packed upper
 * entries, row-major), n_rows 3x3 diagonal blocks D6 (xx xy xz yy yz zz), and one 6x3 coupling block per row
 * (Hpl18: entry p*3 + c = H[pose p][row component c]); no row-row coupling.  x = [x_pose(6), x_rows(3 n_rows)].
 * Not used by any solve entry point. */
int nrs_debug_pcg_solve(nrs_ctx* ctx, int32_t n_rows, const double* Hpp21, const double* bp /*6*/, const double* D6,
                        const double* Hpl18, const double* bl /*3 n_rows*/, double lambda, double* x, int32_t* iters);

/* ---- N1 parity tap: the direct (nested-dissection, multifrontal Cholesky) solve of a2's system on an explicitly given
 * block system -- what replaces LinearSolverEigen::solve (third_party/g2o/g2o/solvers/eigen/linear_solver_eigen.h:92-173:
 * ordering + symbolic step once, numeric sparse Cholesky per LM trial) when nrs_track_deform_solve[_rg] runs a frame on the
 * direct path.  n_nodes unknown blocks of 3 scalars at positions pos (n x 3, used for the
 * dissection only), `last` (n, may be null) marks blocks that are eliminated at the root whatever their position (the two
 * halves of a pose block), n_pairs unique couplings (a, b) with their 3x3 blocks Vp (row-major, rows = a's components),
 * diagonal blocks Dn (9 per node), right-hand side bn (3 per node): solves (A + lambda I) x = b.  Returns
 * NRS_ERR_NUMERIC when a pivot is not positive (linear_solver_eigen.h:124-136: the LM trial then counts as failed).
 * stats (8, may be null): fronts, levels, largest own / boundary size, L and U doubles, factorisation flops, workgroups.
 * Runs the device kernels (k_nd_level / k_nd_back) `repeats` times (timing: ms_per_solve, may be null).  Not used by any solve
 * entry point; the host reference it is held to lives in oracle/nd_host.cpp. */
int nrs_debug_nd_solve(nrs_ctx* ctx, int32_t n_nodes, const double* pos, const uint8_t* last, int32_t n_pairs, const int32_t* pairs,
                       const double* Dn, const double* Vp, const double* bn, double lambda, int32_t repeats, double* x, int64_t* stats,
                       double* ms_per_solve);
/* The context keeps the symbolic factorisation (ordering, fronts, device arrays) of the last few single-frame problems and reuses
 * it when a later problem has the same structure -- as a caller of linear_solver_eigen.h:144-169 does who does not request a new
 * ordering (the symbolic step runs once, then only numeric factorisations).  out[0] = problems that reused a plan, out[1] = plans
 * built, since the context was created. */
int nrs_debug_nd_cache_stats(nrs_ctx* ctx, int64_t out[2]);

/* ---- f3: ShiTomasi (modules/features/shi_tomasi.{h,cc}) + Tracking::ExtractFeatures (tracking.cc:118-134) --
 * nrs_shi_configure = ShiTomasi::ShiTomasi(Options) (shi_tomasi.cc:29-31): a fresh extractor (zeroed
 * buffers on first use, feature ids from 0).  nrs_shi_extract = ShiTomasi::Extract (shi_tomasi.cc:38-54)
 * followed by the caller's mask filter: prev_xy are the keypoints the frame already holds (their score
 * cells are set to -1, shi_tomasi.cc:93-96; they are not returned), out = the NEW keypoints in the
 * reference's row-major order with their class ids (ids are consumed before the mask drops points).
 * The extractor is stateful exactly like the reference object: gradient and score buffers persist
 * between calls (reallocated, zeroed, only when the image size changes) and the reference's single pass
 * leaves some cells to the next call.  width >= height >= 5 is required: the reference's
 * first / last row loops run their column index to rows-1 (shi_tomasi.cc:187,336).
 * *n_out = number of keypoints found; if it exceeds capacity only the first `capacity` were written. */
int nrs_shi_configure(nrs_ctx* ctx, int32_t nms_window /* Options::non_max_suprresion_window_size, default 5 */);
int nrs_shi_extract(nrs_ctx* ctx, const uint8_t* img, int32_t w, int32_t h, int32_t stride,
                    const uint8_t* mask /* nullable: keep points where mask != 0 */, int32_t mask_stride,
                    int32_t n_prev, const float* prev_xy /* n_prev x 2 */,
                    int32_t capacity, float* out_xy /* capacity x 2 */, int32_t* out_id /* capacity */, int32_t* n_out);
/* parity tap: the extractor's buffers after the last call (h x w each, any pointer may be null) */
int nrs_shi_buffers(nrs_ctx* ctx, float* scores, int16_t* xgrad, int16_t* ygrad);

/* ---- multi-GPU: one deformable-BA window sharded over the GPUs of a node ---------
 * The reference solves LocalDeformableBundleAdjustment (g2o_optimization.cc:880-1161) as one g2o graph
 * in one thread; there is no reference interface for this -- it is the build's own extension of a3.
 * One process (or thread) per GPU, one context each.  After nrs_comm_init_* every rank calls
 * nrs_dba_upload with the SAME complete problem; each rank then runs the row kernels for its own
 * contiguous range of keyframes (nrs_shard_plan) and the ranks exchange, on the context's stream,
 *   - per linearisation / trial evaluation: one all-reduce (sum) of the pose blocks of the normal
 *     equations (H_pp 21 + b_p 6 doubles per keyframe) together with chi2, the LM scale and the
 *     max-diagonal slots, and the landmark rows of the boundary keyframes with the two neighbour ranks;
 *   - per PCG iteration: the boundary rows of the search direction and one all-reduce of 3 + 6 n_kf
 *     doubles (dot products, pose rows of the operator).
 * nrs_dba_reset / optimize / download / residuals are collective: every rank calls them in the same
 * order; they return the same trace and, after download, the same complete result on every rank.
 * Embedded windows (nrs_dba_upload_embedded) shard the same way and exchange nothing new: the keyframe ranges are those of
 * nrs_shard_plan on the node copies' lm_kf, a rank holds the skinned observations of its own keyframes only (they reach node copies
 * of their own keyframe, so no halo row), and their pose blocks, chi2, max diagonal and PCG shares travel in the packets above.
 * The solve is the block-Jacobi PCG (nrs_options.embedded_solver).  nrs_dba_download_skinned and nrs_dba_solve_embedded are
 * collective as well: every rank returns the same bits (the skinned points are evaluated on the device, each rank its own, into a
 * vector of the window's observations that is summed over the ranks where it stands).  nrs_dba_solve_window_embedded on a
 * communicator builds each rank's share of the lists on its device under NRS_SHARD_EMBWIN_DEVICE=1 (above).
 * RCCL is bound at run time (dlopen): librccl must be loadable only if nrs_comm_init_rccl is used.   */
#define NRS_COMM_ID_BYTES 128
int nrs_comm_unique_id(uint8_t* id, int32_t capacity /* >= NRS_COMM_ID_BYTES */);      /* rank 0; broadcast by the caller */
int nrs_comm_init_rccl(nrs_ctx* ctx, int32_t world, int32_t rank, const uint8_t* id, int32_t id_bytes);
int nrs_comm_rank(const nrs_ctx* ctx, int32_t* rank, int32_t* world);
/* Sizes of the BA problem resident on THIS rank: stats[0] padded landmark rows of the window, [1] rows whose incidence
 * records this rank packed and holds (sharded: the rows of its keyframe range), [2] / [3] spring / damper incidence
 * slots held, [4] device bytes of the problem.  (A rank also holds the per-row arrays -- state, PCG vectors, diagonal blocks --
 * of its own keyframes and one ghost keyframe either side only; they are addressed by the window's row index all the same.
 * nrs_dba_download and the residual taps gather through transient full-length scratch that is released when they return.) */
int nrs_dba_stats(nrs_ctx* ctx, int64_t stats[5]);
/* keyframe ranges: rank r owns keyframes kf_begin[r] .. kf_begin[r+1]-1 (balanced by padded landmark
 * rows, every rank at least one keyframe).  Host only, needs no device. */
int nrs_shard_plan(int32_t n_kf, int32_t n_lm, const int32_t* lm_kf, int32_t world, int32_t* kf_begin /* world+1 */);
/* the same ranges from the number of vertices of every keyframe (what a rank of nrs_dba_solve_window_embedded derives on its device) */
int nrs_shard_plan_counts(int32_t n_kf, const int32_t* kf_vertices, int32_t world, int32_t* kf_begin /* world+1 */);
/* Test harness: ranks are threads of one process, their contexts on the same GPU; rendezvous on the
 * host.  Runs the sharded arithmetic on a 1-GPU box. */
int nrs_local_group_create(int32_t world /* <= 8 */, void** group);
void nrs_local_group_destroy(void* group);
int nrs_comm_init_local(nrs_ctx* ctx, void* group, int32_t rank);

/* ---- a19 / a20: RegularizationGraph (modules/map/regularization_graph.{h,cc}) ------------------
 * Flat form of the graph: undirected edges carry the fields of RegularizationGraph::Edge
 * (regularization_graph.h:49-59); the raw CSR lists, per map point, its neighbours in ascending
 * index order (= the btree_map ID order GetEdges starts from) together with the undirected edge id.
 * Weights are (float)exp((double)arg) of the float argument -(d*d)/(2*sigma*sigma)
 * (utilities/geometry_toolbox.cc:26-28; see DESIGN.md "weights"). */
typedef struct {
    int32_t n_points;
    const int32_t* rowptr;    /* n_points+1 */
    const int32_t* col;       /* nnz = 2 * n_edges, ascending inside a row */
    const int32_t* eid;       /* nnz -> undirected edge */
    int32_t n_edges;
    float* e_w;               /* in/out: weight                */
    const float* e_d0;        /*         first_distance        */
    float* e_max;             /* in/out: max_distance          */
    float* e_min;             /* in/out: min_distance          */
    int32_t* e_status;        /* in/out: NRS_GRAPH_*           */
    float sigma;              /* options_.weight_sigma         */
    float stretch_th;         /* options_.streching_th (1.1)   */
} nrs_graph;

/* RegularizationGraph::GetEdges for every point (regularization_graph.cc:61-87): neighbours sorted
 * by (status asc, weight desc, index asc) and cut at the first weight below min_weight =
 * InterpolationWeight(1.5 sigma, sigma).  o_col / o_eid need room for nnz entries. */
int nrs_graph_select_neighbours(nrs_ctx* ctx, const nrs_graph* g, int32_t* o_rowptr, int32_t* o_col,
                                int32_t* o_eid);

/* RegularizationGraph::UpdateVertex for the listed points (regularization_graph.cc:89-146): every
 * edge of such a point is refreshed from pos (n_points x 3 last world positions); good_count[i] =
 * connections of ids[i] that pass the stretch test. */
int nrs_graph_update(nrs_ctx* ctx, nrs_graph* g, const float* pos, int32_t n_ids, const int32_t* ids,
                     int32_t* good_count);

/* ---- a19 / a20 at the reference's density: RegularizationGraph as a device-resident object ----------------------
 * The reference graph is all-pairs (Map::InitializeRegularizationGraph, modules/map/map.cc:148-166; graph growth
 * modules/mapping/mapping.cc:240-256): every vertex has N - 1 connections, UpdateVertex counts ALL of them (its
 * return value feeds the caller's "fewer than 5 good connections -> BAD", g2o_optimization.cc:468-473), so a radius
 * cut-off is not equivalent.  nrs_rgraph keeps the dense edge state in HBM (capacity^2 x 13 bytes: 5k points =
 * 325 MB) and replaces the bodies of the class' methods (modules/map/regularization_graph.cc):
 *   nrs_rgraph_create     RegularizationGraph(Options&, Map*) :27-31       point indices are 0 .. capacity-1
 *   nrs_rgraph_set_sigma  SetSigma :33-36
 *   nrs_rgraph_add_edges  AddEdge :38-55 for every (new, other) pair, new != other, relative position pos[other] -
 *                         pos[new]; all-pairs initialisation: new = other = every initial point
 *   nrs_rgraph_update     UpdateVertex :130-146 for the listed points; good_count[i] = its return value
 *   nrs_rgraph_get_edges  GetEdges :71-87 for the listed points: (status asc, weight desc, index asc), cut at the first
 *                         weight below min_weight; fixed-stride outputs [n_ids][cap_per_point] + count[n_ids] = the
 *                         FULL length of the list, of which the first min(count, cap_per_point) entries are written
 *                         (the reference's callers walk a prefix: 11 accepted neighbours or the first BAD edge)
 *   nrs_rgraph_edge       GetEdge :57-59 (out = weight, first, max, min distance; status -1 = no such edge)
 * pos is capacity x 3 floats (positions by point index; rows of unlisted points are not read). */
typedef struct nrs_rgraph nrs_rgraph;
int nrs_rgraph_create(nrs_ctx* ctx, int32_t capacity, float sigma, float stretch_th, nrs_rgraph** out);
void nrs_rgraph_destroy(nrs_rgraph* g);
int nrs_rgraph_set_sigma(nrs_rgraph* g, float sigma);
float nrs_rgraph_min_weight(const nrs_rgraph* g);
int nrs_rgraph_add_edges(nrs_rgraph* g, const float* pos, int32_t n_new, const int32_t* new_ids, int32_t n_other,
                         const int32_t* other_ids);
int nrs_rgraph_update(nrs_rgraph* g, const float* pos, int32_t n_ids, const int32_t* ids, int32_t* good_count);
int nrs_rgraph_get_edges(nrs_rgraph* g, int32_t n_ids, const int32_t* ids, int32_t cap_per_point, int32_t* count,
                         int32_t* col, float* w, float* d0, int32_t* status);
int nrs_rgraph_edge(nrs_rgraph* g, int32_t i, int32_t j, float out[4], int32_t* status);
/* parity tap: rows of the dense state, n_ids x capacity each (status 255 = no edge; any pointer may be null) */
int nrs_rgraph_rows(nrs_rgraph* g, int32_t n_ids, const int32_t* ids, float* maxd, float* mind, float* d0, uint8_t* status);
/* Grows the graph to new_capacity >= the current one (the limits of nrs_rgraph_create; its error texts with the call's own name in front): the dense state is
 * re-laid at the new stride on the device, every new cell is "no edge", every edge between old indices keeps its values, and
 * the lists a GetEdges left on the device are dropped.  On failure the graph is unchanged.  Callers of nrs_track_deform_solve_rg
 * pad map_pos to the new capacity (n_points = capacity = rows of map_pos still holds). */
int nrs_rgraph_resize(nrs_rgraph* g, int32_t new_capacity);

/* ---- f2: DeformableTriangulation, batched (modules/optimization/g2o_optimization.cc:559-814) --------------------
 * One call triangulates every candidate feature of a frame (the reference calls the function once per candidate from
 * Mapping::LandmarkTriangulation, modules/mapping/mapping.cc:65-116).  Input = the TemporalBuffer flattened
 * (modules/map/temporal_buffer.h:43-63): n_frames <= 21 snapshots, oldest first; per snapshot its
 * camera_transform_world (Sophus::SE3f as qx qy qz qw tx ty tz) and, per keypoint id 0 .. n_ids-1, whether the id has
 * a keypoint there (keypoint_tracks) and a landmark position (mapppoint_tracks_); last_status = keypoint_tracks_status
 * of the LAST snapshot (GetClosestMapPointsToFeature looks for TRACKED_WITH_3D neighbours there).
 * out_status: 0 ok, else the InternalError the reference returns: 1 "Feature too close to other ones." 2 / 3 "High
 * reprojection error at first / second camera." 4 "Low parallax." 5 "Found no neighbours in a temporal point."
 * 6 "Negative initial depth." 7 "Optimization is empty." 8 "Triangulation has to many bad neighbors." 9 "Triangulation
 * has to much error." 10 the caller's "Short track" (track shorter than min_track; mapping.cc:88 uses 5).
 * out_xyz: the triangulated world position (zeros unless status 0).  out_debug (nullable, n_cand x 4): final chi2,
 * LM iterations, LM trials, regulariser edges.  The reprojection edge has no analytic Jacobian in the reference: it is
 * g2o's numeric one (delta 1e-9, central) through the fp32 projection, reproduced as such. */
int nrs_triangulate_batch(nrs_ctx* ctx, const nrs_camera* cam, int32_t n_frames, const float* poses /* n_frames x 7 */,
                          int32_t n_ids, const uint8_t* has_kp /* n_frames x n_ids */, const float* kp_xy /* .. x 2 */,
                          const uint8_t* has_lm, const float* lm_xyz /* .. x 3 */, const int32_t* last_status /* n_ids */,
                          int32_t n_cand, const int32_t* cand_ids, int32_t min_track, int32_t* out_status,
                          float* out_xyz /* n_cand x 3 */, double* out_debug);

/* ---- Frame mapping: Mapping::LandmarkTriangulation (modules/mapping/mapping.cc:65-236) in one call ---------------
 * Input: the flat TemporalBuffer of nrs_triangulate_batch (same layout, same checks, oldest snapshot first, n_frames <= 21:
 * InsertSnapshotFromFrame pops when size() > 20 and then inserts, temporal_buffer.cc:49-55) plus deform_mag[n_frames] =
 * Snapshot::deformation_magnitud (what nrs_track_deform_solve* return in deform_median), Mapping::Options::rad_per_pixel,
 * CheckRigidity's threshold (the reference passes 0.004) and the shortest track the deformable leg takes (5).
 * The candidates are found on the device: GetTriangulationCandidatesIds (temporal_buffer.cc:62-74) = the ids whose last_status
 * is TRACKED (1), ascending.  Per candidate the call returns both legs:
 *   rigid_status (mapping.cc:117-190; the track's endpoints are the OLDEST and the NEWEST snapshot holding the id, which the
 *   reference names current_ / previous_ in that order):
 *     0 NRS_MAP_OK
 *     1 NRS_MAP_CLOSE            "Close features" (GetClosestMapPointsToFeature(id, 10, 20, 500) empty; both legs get this code)
 *     2 NRS_MAP_NOT_RIGID        "Rigidity not detected"
 *     3 NRS_MAP_MIDPOINT         TriangulateMidPoint's own error (geometry_toolbox.cc:45-79 returns none: never produced)
 *     4 NRS_MAP_PARALLAX         "Parallax error." -- parallax outside [10, 20] x rad_per_pixel
 *     5 NRS_MAP_DEPTH_PREVIOUS   "Parallax error." -- negative depth in the previous (newest) camera
 *     6 NRS_MAP_REPROJ_PREVIOUS  "Parallax error." -- squared reprojection error > 5.991 there
 *     7 NRS_MAP_DEPTH_CURRENT    "Parallax error." -- negative depth in the current (oldest) camera
 *     8 NRS_MAP_REPROJ_CURRENT   "Parallax error." -- squared reprojection error > 5.991 there
 *   deform_status (:97-115): the codes of nrs_triangulate_batch (10 = "Short track") and 11 = "NaN." (a result with a NaN).
 * counts = n_rigid_triangulations, n_deformable_triangulations and the mode of the vote (:192-209): 1 rigid (n_rigid > 1.5
 * n_deformable), else 2 deformable (n_deformable >= 1.5 n_rigid; also 0 / 0), else 0 none.  The accepted list (:211-236) is, in
 * candidate order, every success of the voted leg without a NaN that has a keypoint in snapshot index_snapshot (-1 = the last
 * one, which is what current_frame->GetId() - 1 names when DoMapping runs: DESIGN.md 4 "Frame mapping").
 * Every output array needs room for as many entries as there are TRACKED ids (x 3 for positions).  A frame without
 * candidates returns 0 with *n_cand = *n_accepted = 0, mode 2, and launches nothing. */
enum { NRS_MAP_OK = 0, NRS_MAP_CLOSE = 1, NRS_MAP_NOT_RIGID = 2, NRS_MAP_MIDPOINT = 3, NRS_MAP_PARALLAX = 4, NRS_MAP_DEPTH_PREVIOUS = 5,
       NRS_MAP_REPROJ_PREVIOUS = 6, NRS_MAP_DEPTH_CURRENT = 7, NRS_MAP_REPROJ_CURRENT = 8 };
int nrs_map_frame(nrs_ctx* ctx, const nrs_camera* cam, int32_t n_frames, const float* poses /* n_frames x 7 */, int32_t n_ids,
                  const uint8_t* has_kp, const float* kp_xy, const uint8_t* has_lm, const float* lm_xyz, const int32_t* last_status,
                  const float* deform_mag /* n_frames */, float rad_per_pixel, float rigidity_th, int32_t min_track,
                  int32_t index_snapshot, int32_t* n_cand, int32_t* cand_ids, int32_t* rigid_status, float* rigid_xyz,
                  int32_t* deform_status, float* deform_xyz, int32_t counts[3], int32_t* n_accepted, int32_t* accepted_ids,
                  float* accepted_xyz);

/* Graph growth of the same function (mapping.cc:238-256): AddEdge(new, other, pos[other] - pos[new]) for every new landmark
 * against every map point the frame holds as TRACKED_WITH_3D or JUST_TRIANGULATED -- the new ones included, so a pair of two
 * new points is added from both sides and the second AddEdge writes the same edge (regularization_graph.cc:38-55).  These are
 * exactly the semantics of nrs_rgraph_add_edges, which this call forwards to (tests/test_gpu_map.py holds it to
 * RegularizationGraph.AddEdge of the restatement); the graph must have been resized to hold the new indices. */
int nrs_map_grow_graph(nrs_ctx* ctx, nrs_rgraph* g, const float* pos, int32_t n_new, const int32_t* new_ids, int32_t n_other,
                       const int32_t* other_ids);

/* ---- The resident TemporalBuffer (reference modules/map/temporal_buffer.cc:28-74) ----------------------------------------------
 * The buffer nrs_map_frame takes flattened from the host, held on the device by an object a context owns (as nrs_rgraph): a frame
 * enters with ONE upload and frame mapping reads the buffer where it lies.
 *   nrs_tbuf_create   TemporalBuffer(Options&): max_buffer_size in [1, 20] (the reference's 20, SLAM/system.cc:42)
 *   nrs_tbuf_insert   InsertSnapshotFromFrame (:28-56).  The caller passes the frame's n slots UNFILTERED: keypoint id (class_id),
 *                     keypoint, landmark position and LandmarkStatus per slot; only the slots whose status is TRACKED_WITH_3D (0) or
 *                     TRACKED (1) enter the snapshot (:31-34).  has_lm: null = every kept slot has a landmark entry, as in the
 *                     reference (:41, zeros for TRACKED); else one byte per slot (the synthetic buffers of the tests have keypoints
 *                     without one).  pose_qt = camera_transform_world (qx qy qz qw tx ty tz), deform_mag = deformation_magnitud.
 *                     The pop rule is the reference's (:49-55): the oldest snapshot leaves when size() > max_buffer_size BEFORE the
 *                     insert, so the buffer fills to max + 1, then goes max + 1 -> max -> max + 1 inside every call: never more than max + 1 <= 21.
 *                     Refused with NRS_ERR_INVALID, the buffer unchanged: a null array with n > 0; a negative id among the kept
 *                     slots; two kept slots with one id (the reference's map would silently overwrite the first: this build refuses
 *                     and says so; ids of slots that are not kept are not looked at); held ids that would span more than 4 194 304
 *                     (2^22: the device addresses a row through tables over [lowest, highest] held id).
 *                     The snapshot is staged in pinned memory and copied in one asynchronous transfer; the slots grow by doubling,
 *                     so a steady state allocates nothing.
 *   nrs_tbuf_clear    forgets every snapshot (the slots stay allocated)
 *   nrs_tbuf_info     snapshots held, distinct keypoint ids over them, GetTriangulationCandidatesIds().size() (:62-74) -- known on
 *                     the host (per-id reference counts), nothing is read back
 *   nrs_tbuf_flat     debug download of the dense form the device builds for a mapping call: the distinct ids ascending (row j =
 *                     ids[j]), has_kp / has_lm [n_frames x n_ids], kp_xy [.. x 2], lm_xyz [.. x 3], last_status [n_ids] (BAD (3) for
 *                     an id the last snapshot does not hold), poses [n_frames x 7], deform_mag [n_frames], oldest snapshot first;
 *                     values under a clear flag are zero.  Sizes from nrs_tbuf_info.
 *   nrs_map_frame_tbuf  nrs_map_frame (above: same arguments, same outputs, same bits) on the resident buffer, except that cand_ids
 *                     and accepted_ids are KEYPOINT IDS (ascending, as the rows are), translated on the device.  The outputs need
 *                     room for as many entries as nrs_tbuf_info's candidates.  No candidates: 0 / 0, mode 2, nothing launched.
 *                     An empty buffer is NRS_ERR_STATE; a buffer of another context, index_snapshot outside [-1, snapshots held)
 *                     or a non-finite threshold NRS_ERR_INVALID. */
typedef struct nrs_tbuf nrs_tbuf;
int nrs_tbuf_create(nrs_ctx* ctx, int32_t max_buffer_size, nrs_tbuf** out);
void nrs_tbuf_destroy(nrs_tbuf* tb);
int nrs_tbuf_clear(nrs_tbuf* tb);
int nrs_tbuf_insert(nrs_tbuf* tb, int32_t n, const int32_t* kp_id, const float* kp_xy /* n x 2 */, const float* lm_xyz /* n x 3 */,
                    const int32_t* status, const uint8_t* has_lm /* n or null */, const float pose_qt[7], float deform_mag);
int nrs_tbuf_info(const nrs_tbuf* tb, int32_t* n_frames, int32_t* n_ids, int32_t* n_candidates);
int nrs_tbuf_flat(nrs_tbuf* tb, int32_t* ids, uint8_t* has_kp, float* kp_xy, uint8_t* has_lm, float* lm_xyz, int32_t* last_status,
                  float* poses, float* deform_mag);
int nrs_map_frame_tbuf(nrs_ctx* ctx, const nrs_camera* cam, nrs_tbuf* tb, float rad_per_pixel, float rigidity_th, int32_t min_track,
                       int32_t index_snapshot, int32_t* n_cand, int32_t* cand_ids, int32_t* rigid_status, float* rigid_xyz,
                       int32_t* deform_status, float* deform_xyz, int32_t counts[3], int32_t* n_accepted, int32_t* accepted_ids,
                       float* accepted_xyz);

/* ---- a2: CameraPoseAndDeformationOptimization (g2o_optimization.cc:148-557) ------------------
 * Frame side: n_f landmarks in frame index order with their map-point index (f_map, -1 = none),
 * LandmarkStatus (in/out), keypoint (f_uv) and position (f_pos, in/out).  Map side: the graph
 * (updated in place, OPT:458-474) and MapPoint::GetLastWorldPosition of every map point (map_pos,
 * in/out).  pose_qt in: frame pose; out: refined pose.  Outputs: Frame::SetDeformationMaginitud
 * value, and the re-located lost map points (lost needs room for n_points entries). */
int nrs_track_deform_solve(nrs_ctx* ctx, const nrs_camera* cam, nrs_graph* g, float* map_pos,
                           int32_t n_f, const int32_t* f_map, int32_t* f_status, const float* f_uv,
                           float* f_pos, double pose_qt[7], float scale, float* deform_median,
                           int32_t* n_lost, int32_t* lost, nrs_lm_trace* trace);

/* The same function with the RegularizationGraph held on the device at the reference's all-pairs density (nrs_rgraph,
 * above): GetEdges (OPT:252, 496) and UpdateVertex (OPT:468) are served from it, so a point's good-connection count is
 * taken over all of its N - 1 connections as in the reference (the "fewer than 5 -> BAD" rule, OPT:470-473).
 * n_points = the graph's capacity = rows of map_pos; cap_per_point = how much of each point's GetEdges list is fetched at
 * first (if a walk of OPT:255-279 reaches the end of a truncated list, four times as much is fetched and the walks start
 * over: the result does not depend on cap_per_point, the time does).  Connections a walk passes over without any effect
 * are left out of the fetched lists on the device: in the lost-point stage (OPT:483-520) those to points that were not
 * optimised, in the embedded mode below those to optimised points that carry no vertex (BAD ones stay: they end a walk). */
int nrs_track_deform_solve_rg(nrs_ctx* ctx, const nrs_camera* cam, nrs_rgraph* g, int32_t n_points, int32_t cap_per_point,
                              float* map_pos, int32_t n_f, const int32_t* f_map, int32_t* f_status, const float* f_uv,
                              float* f_pos, double pose_qt[7], float scale, float* deform_median, int32_t* n_lost,
                              int32_t* lost, nrs_lm_trace* trace);

/* LocalDeformableBundleAdjustment (g2o_optimization.cc:880-1161) served by the same device-resident graph: nrs_dba_solve_window
 * without the neighbour lists.  kf_pt are map-point indices = the graph's indices (the graph's capacity stands for n_points; an index
 * beyond it is NRS_ERR_INVALID), everything else as for nrs_dba_solve_window.  On the device: the window's distinct map points are
 * listed in ascending order, GetEdges (OPT:1029-1030) runs for them at cap_per_point entries per point (<= 0: 64) and the lists stay
 * where it leaves them; the walks of OPT:1033-1074 (springs) and OPT:1086-1135 (dampers) read them there, a wave per landmark.  Those
 * walks are not a2's: a neighbour the keyframe does not observe is passed over WITHOUT counting (OPT:1041-1043, 1094-1097), so no fixed
 * prefix of a list is enough.  A walk RAN OFF when it comes to the end of a truncated prefix without having met a BAD connection and
 * with no more than 10 regularisers counted; if any walk of the window ran off, GetEdges and the walks are redone for the whole window
 * at twice the prefix length, up to the LIMIT: min(capacity, the candidates k_rg_get_edges can sort in one workgroup's LDS - 1024) --
 * 3072 entries per point with 64 KB of LDS per workgroup, 7168 with 160 KB; a graph of no more points than that is served whole,
 * whatever its lists look like.  A walk that still runs off at the
 * limit is NRS_ERR_INVALID (the message names the map point and the limit), never a shorter window.  The result does not depend on
 * cap_per_point: the edge lists are index for index those of nrs_dba_build_edges on the full lists, poses, points and trace are
 * bit for bit those of nrs_dba_solve_window on them (windows below the device packer's threshold copy the device-built lists back
 * and take the host packer).  nrs_dba_window_edges returns the resident window's lists in both cases.  A context with a communicator
 * is refused (NRS_ERR_INVALID): a sharded form of this call does not exist; the embedded form is nrs_dba_solve_window_rg_embedded.
 * nrs_dba_window_rg_stats: out = {distinct map points, final prefix length, GetEdges rounds, walks that ran off in round 1} of the
 * resident window this call made (NRS_ERR_STATE otherwise).  Debug switch: NRS_RG_MAX_CAP=<n> lowers the limit. */
int nrs_dba_solve_window_rg(nrs_ctx* ctx, const nrs_camera* cam, int32_t n_kf, double* poses_qt /* in/out */, const int32_t* kf_rowptr,
                            const int32_t* kf_pt, float* lm_xyz /* in/out */, const float* lm_uv, nrs_rgraph* g, int32_t cap_per_point,
                            float scale, int32_t iters, nrs_lm_trace* trace);
int nrs_dba_window_rg_stats(nrs_ctx* ctx, int64_t out[4]);

/* The EMBEDDED window (nrs_dba_solve_window_embedded) served by the device-resident graph: nrs_dba_solve_window_rg with a node set.
 * kf_pt are the graph's indices, obs_xyz / obs_uv are per observation, is_node is indexed by graph index and holds as many entries as
 * the graph has capacity.  No neighbour array crosses the host.  On the device: the distinct map points of ALL observations, nodes or
 * not, are listed; GetEdges runs for them at cap_per_point entries per point (<= 0: 64); a wave per observation walks its list there
 * (csrc/nrs_engine_embwin.hpp k_ew_walk_wave): a node copy its springs and dampers between node copies, any other observation the walk
 * that accepts its <= 11 node copies.  All three walks pass over a neighbour that is not a node copy of the keyframe without counting,
 * so each of them can RUN OFF a truncated prefix under the rule above; rounds, limit, NRS_RG_MAX_CAP and the refusal at the limit
 * (NRS_ERR_INVALID; the message names this call, the map point and the limit) are those of nrs_dba_solve_window_rg.  Then the shared
 * construction of nrs_dba_solve_window_embedded (one copy back, the set-up of nrs_dba_upload_embedded), optimize(iters) and the download.
 * Arguments are checked as for nrs_dba_solve_window_rg, and is_node must not be null; a NODE listed twice in one keyframe is
 * NRS_ERR_INVALID; a context with a communicator is refused.  The result does not depend on cap_per_point: the lists are index for index
 * and bit for bit those of nrs_dba_build_edges_embedded on the graph's full lists, poses, obs_xyz and trace those of
 * nrs_dba_solve_window_embedded on them.  On return the window is resident as after nrs_dba_upload_embedded and obs_xyz is written as
 * nrs_dba_solve_window_embedded writes it; nrs_dba_window_edges_embedded returns the lists (*on_device = 1) and nrs_dba_window_rg_stats
 * the four statistics.  After an error nothing is resident and neither tap answers (NRS_ERR_STATE). */
int nrs_dba_solve_window_rg_embedded(nrs_ctx* ctx, const nrs_camera* cam, int32_t n_kf, double* poses_qt /* in/out */, const int32_t* kf_rowptr,
                                     const int32_t* kf_pt, float* obs_xyz /* n_obs x 3, in/out */, const float* obs_uv, nrs_rgraph* g,
                                     const uint8_t* is_node /* by graph index, capacity entries */, int32_t cap_per_point, float scale, int32_t iters,
                                     nrs_lm_trace* trace);

/* ---- N2: embedded deformation -- "points x graph nodes" as SURVEY.md 8(d) words it ------------------------------------
 * nrs_track_deform_solve_rg with a node set: f_node[i] != 0 marks the frame landmarks (among the TRACKED_WITH_3D ones) that carry
 * a free deformation; the regularisers of g2o_optimization.cc:255-335 are built between nodes only.  Every other TRACKED_WITH_3D
 * landmark is SKINNED: its deformation is sum_k omega_k delta_{n_k} over the <= 11 nodes its own GetEdges walk accepts (the walk of
 * OPT:255-279: stop after more than 10 accepted or at the first BAD connection; omega = connection weight / their sum), and its
 * reprojection edge (reprojection_error_with_deformation.cc:37-68: same residual, information, Huber kernel) constrains those nodes
 * and the pose with the Jacobian omega_k x the reference's block.  Rounds, inlier levels, IQR rejection, write-back and graph
 * update treat all optimised landmarks alike; the lost-point stage (OPT:476-553) follows nodes and skinned landmarks (the latter as
 * constants).  The reference has no such estimator -- its only skinning is that second stage -- so this mode is this build's,
 * stated in oracle/embedded_oracle.py; with every landmark a node it IS nrs_track_deform_solve_rg, bit for bit (tests).  Runs on
 * the direct solver (nrs_options.direct_solve != 2). */
int nrs_track_deform_solve_embedded(nrs_ctx* ctx, const nrs_camera* cam, nrs_rgraph* graph, int32_t n_points, int32_t cap_per_point,
                                    float* map_pos, int32_t n_f, const int32_t* f_map, int32_t* f_status, const float* f_uv,
                                    float* f_pos, const uint8_t* f_node, double pose_qt[7], float scale, float* deform_median,
                                    int32_t* n_lost, int32_t* lost, nrs_lm_trace* trace);


/* ---- a21-a23: LucasKanadeTracker (modules/matching/lucas_kanade_tracker.{h,cc}) ----------------
 * The context holds what the reference's tracker object holds: the reference points and, per point
 * and pyramid level, the cached 21x21 template (intensity x32 as int16, Scharr derivative as
 * 2 x int16, the two window means, a "filled" flag) -- members Iref_/Idref_/vMeanI_/vMeanI2_/prevPts_
 * (lucas_kanade_tracker.h:76-91).  Images are 8-bit single channel, row stride in bytes.
 * The pyramid is built on the device the way cv::buildOpticalFlowPyramid(img, pyr, Size(21,21),
 * maxLevel) builds it (LK:50,184; DESIGN.md "pyramid"). */
typedef struct {
    int32_t win_size;            /* 21 (the only size the reference uses, SLAM/system.cc:78)        */
    int32_t max_level;           /* 4                                                              */
    int32_t max_iters;           /* 10                                                             */
    float epsilon;               /* 1e-4, on |delta|^2                                             */
    float min_eig_threshold;     /* 1e-4                                                           */
} nrs_klt_config;

int nrs_klt_configure(nrs_ctx* ctx, const nrs_klt_config* cfg);     /* defaults = the values above */
int nrs_klt_clear(nrs_ctx* ctx);                                    /* LucasKanadeTracker::clear   */
int nrs_klt_num_points(nrs_ctx* ctx);

/* LucasKanadeTracker::SetReferenceImage (LK:47-168).  mask: NULL or w x h bytes, 0 = masked. */
int nrs_klt_set_reference(nrs_ctx* ctx, const uint8_t* img, int32_t w, int32_t h, int32_t stride,
                          const uint8_t* mask, int32_t n, const float* xy);

/* LucasKanadeTracker::Track (LK:170-596).  xy in: initial guess (used when use_initial_flow),
 * out: tracked positions; status in/out: LandmarkStatus, only usable points are tracked and they
 * may become OUT_IMAGE_BOUNDARIES / BAD_FEATURE / BAD; n_good = points that pass the SSIM gate;
 * ssim (may be NULL): SSIM of every point that reached the gate.
 * Two rules are this project's definitions (the reference is undefined there; DESIGN.md 4 "Lucas-Kanade tracker"):
 *  - top level: the iteration starts at min(max_level, n_levels - 1) of the TRACKED image's pyramid, which is shorter than
 *    max_level + 1 levels when min(w, h) <= 21 * 2^max_level, and the initial guess (or the previous point) is scaled to that level.
 *    A tracker configured with max_level >= n_levels returns bit for bit what one configured with n_levels - 1 returns; template
 *    slots of levels that were not built stay invalid with means of -1.
 *  - positions: a window origin whose coordinate is not finite, or whose floor does not fit an int, is outside the image.  The test
 *    comes before every float -> int conversion: the reference point in nrs_klt_set_reference (no template at that level), the
 *    previous point, every iterate and the SSIM position here (the level ends; OUT_IMAGE_BOUNDARIES at level 0).  A window that is
 *    all zero in the tracked image (meanJ2 = 0: the step is NaN) ends this way, as does a NaN / inf / 1e30 guess. */
int nrs_klt_track(nrs_ctx* ctx, const uint8_t* img, int32_t w, int32_t h, int32_t stride, int32_t n,
                  float* xy, int32_t* status, int32_t use_initial_flow, float min_ssim, int32_t* n_good,
                  float* ssim);

/* GetPhotometricInformationOfPoint / InsertPhotometricInformation (LK:598-620).  Buffers hold
 * (max_level+1) levels: gray (levels x 441), grad (levels x 441 x 2), mean (levels x 2: meanI,
 * meanI2), valid (levels). */
int nrs_klt_get_template(nrs_ctx* ctx, int32_t idx, float xy[2], int16_t* gray, int16_t* grad,
                         float* mean, uint8_t* valid);
int nrs_klt_insert_template(nrs_ctx* ctx, const float xy[2], const int16_t* gray, const int16_t* grad,
                            const float* mean, const uint8_t* valid);

/* The same two calls for `count` consecutive points at once (no reference counterpart: the caller
 * loops, tracking.cc:203-209,383-391,457-460): buffers are point-major, i.e. the single-point layout
 * repeated; get reads points [first, first+count), insert appends. */
int nrs_klt_get_templates(nrs_ctx* ctx, int32_t first, int32_t count, float* xy, int16_t* gray, int16_t* grad,
                          float* mean, uint8_t* valid);
int nrs_klt_insert_templates(nrs_ctx* ctx, int32_t count, const float* xy, const int16_t* gray,
                             const int16_t* grad, const float* mean, const uint8_t* valid);

/* The same hand-over without the host in between.  The reference keeps a map point's photometric information in its Map
 * (GetPhotometricInformation at keyframes, tracking.cc:383-391) and inserts it into a tracker when the point is reused
 * (InsertPhotometricInformation, tracking.cc:457-460; PointReuse's own tracker, :422-448).  Here the context keeps an ARCHIVE in
 * device memory: nrs_klt_archive_templates copies the templates of tracker slots `slots[i]` into the archive entries `keys[i]`
 * (the caller's ids, e.g. map point ids; an entry is overwritten when archived again), nrs_klt_insert_archived appends the entries
 * `keys[i]` of context `src`'s archive to THIS context's tracker with the positions xy (n x 2).  Both contexts on one device; a
 * tracker with fewer pyramid levels than the archive takes the levels it has (PointReuse's tracker: maxLevel 1).  Byte for
 * byte what nrs_klt_get_templates + nrs_klt_insert_templates hand over (tests/test_gpu_klt.py).  The archive is DENSE by key (the key
 * indexes its entry: no lookup on the device), window^2 x levels x 6 bytes per key up to the largest key seen: keys must be
 * below 2^20 (NRS_ERR_INVALID otherwise); an archive that was built with another pyramid level count is dropped and starts over. */
int nrs_klt_archive_templates(nrs_ctx* ctx, int32_t n, const int32_t* slots, const int32_t* keys);
int nrs_klt_insert_archived(nrs_ctx* ctx, nrs_ctx* src, int32_t n, const int32_t* keys, const float* xy);

/* Tracking::PointReuse (tracking.cc:394-506) in ONE call on the context that tracks the frame: nothing but the frame's bookkeeping is
 * uploaded, the image is the pyramid this context's last nrs_klt_track[_front] / nrs_klt_set_reference[_front] built (levels 0 and 1
 * of it are what PointReuse's own LucasKanadeTracker(21x21, maxLevel 1) would build), the templates are the archive entries whose key
 * is the MAP INDEX, read in place.  Every fp32 expression below runs without contraction, in the stated order (DESIGN.md 4
 * "PointReuse (one call)").
 *   1 project    R from pose_qt (qx qy qz qw tx ty tz) entry by entry as 1 - 2(yy + zz), 2(xy - zw), ...;
 *                pc_r = ((R_r0 X0 + R_r1 X1) + R_r2 X2) + t_r;  uv = the camera model's fp32 projection of pc
 *   2 candidates ascending map index: (lost or (not present and pc.z >= 0)) and inside, where inside = 0 <= u < w and 0 <= v < h
 *                (a NaN coordinate is outside), present = frame_slot[i] >= 0 and slot_status[frame_slot[i]] is TRACKED_WITH_3D or
 *                JUST_TRIANGULATED, lost = i is listed in lost_ids.  Lost points are not tested for z (the reference does not either)
 *   3 track      every candidate from status TRACKED_WITH_3D: reference point and initial guess = its uv (the seed), top level
 *                min(1, pyramid levels - 1), this context's max_iters / epsilon / min_eig_threshold, then the SSIM gate with
 *                min_ssim -- nrs_klt_track's arithmetic.  A key nothing was archived under is a template that was never filled:
 *                OUT_IMAGE_BOUNDARIES, no error (an empty archive: every candidate ends so)
 *   4 gate       accepted = status still TRACKED_WITH_3D and not (ex ex + ey ey > 5.99f), ex = u - x, ey = v - y
 *   5 outputs    caller buffers of n_map entries (x 2 for seed_xy / xy), the first n_cand of them written: cand_id (map index),
 *                seed_xy, xy, status, accepted (0 / 1); n_reused = number accepted
 *   6 insert_new != 0: the accepted candidates with frame_slot < 0 are appended to this context's tracker in candidate order, each with
 *                its xy as reference point -- the state nrs_klt_insert_archived(ctx, ctx, those ids, those xy) leaves; n_new = their
 *                number (0 with insert_new = 0).  With no candidate the tracker is untouched.
 * One host wait for n_cand, one at the end (the tracker's buffers growing aside).
 * NRS_ERR_STATE: no pyramid has been built, or w x h is not its level 0.  NRS_ERR_INVALID: a null pointer, a negative count, a
 * frame_slot at or above n_slots, a lost id outside the map, n_map at or above 2^20 (the archive's key bound), an archive of fewer
 * than 2 levels (or, with insert_new, of fewer levels than this tracker has). */
int nrs_point_reuse(nrs_ctx* ctx, const nrs_camera* cam, const float pose_qt[7], int32_t w, int32_t h, int32_t n_map,
                    const float* map_pos /* n_map x 3 */, const int32_t* frame_slot /* n_map */, int32_t n_slots,
                    const int32_t* slot_status /* n_slots */, int32_t n_lost, const int32_t* lost_ids, float min_ssim, int32_t insert_new,
                    int32_t* n_cand, int32_t* cand_id, float* seed_xy, float* xy, int32_t* status, int32_t* accepted, int32_t* n_reused,
                    int32_t* n_new);

/* ---- f5: the image front end -- System::ImageProcessing + Masker::GetAllMasks (modules/SLAM/system.cc:113-201) ------------
 * What the reference does to every frame before the tracker is entered, on the device, with ONE upload of the frame:
 *   grey    cv::cvtColor(RGB2GRAY) (system.cc:193): 8-bit fixed point (R*9798 + G*19235 + B*3735 + 2^14) >> 15, channel 0 = R
 *   CLAHE   createCLAHE(3.0, Size(8,8))->apply (system.cc:198)
 *   masks   one per configured filter (bright_filter.cc:24-39, border_filter.cc:24-39, predefined_filter.cc:27-39) and "Global":
 *           their AND from 255, eroded by the 10x10 rectangle (masker.cc:94-115)
 * The arithmetic is written down in DESIGN.md "f5"; the Gaussian of BrightFilter is this project's own definition (parity with
 * OpenCV unpinned: no OpenCV in the build, none of its source in the reference tree).  The filters take the grey image only (the
 * reference never hands them anything else, system.cc:122).
 *
 * A filter record mirrors one line of the reference's filters.txt (masker.cc:32-69):
 *   NRS_FRONT_BRIGHT      p[0] = threshold                      ("BrightFilter th")
 *   NRS_FRONT_BORDER      p[0..4] = rb, re, cb, ce, th          ("BorderFilter rb re cb ce th"; th is unused, as in the reference)
 *   NRS_FRONT_PREDEFINED  mask / w / h / stride: the decoded mask image ("Predefined path": decoding stays with the caller); it is
 *                         eroded once, here, by the 20x20 ellipse (PredefinedFilter's constructor) and kept on the device
 * At most NRS_FRONT_MAX_FILTERS filters.  tiles_x x tiles_y: only the reference's 8 x 8 grid is built -- any other value is refused
 * with NRS_ERR_INVALID.  Configuring drops the resident frame.  A context that was never configured processes with no filters,
 * clip 3.0 and 8 x 8 tiles (the Global mask is then 255 everywhere). */
#define NRS_FRONT_MAX_FILTERS 8
enum { NRS_FRONT_BRIGHT = 0, NRS_FRONT_BORDER = 1, NRS_FRONT_PREDEFINED = 2 };
enum { NRS_FRONT_IMAGE_GRAY = 0, NRS_FRONT_IMAGE_CLAHE = 1 };
typedef struct {
    int32_t kind;                /* NRS_FRONT_BRIGHT / BORDER / PREDEFINED                                              */
    int32_t p[5];
    const uint8_t* mask;         /* PREDEFINED only: w x h bytes on the host, row stride in bytes; read during the call  */
    int32_t w, h, stride;
} nrs_front_filter;
int nrs_front_configure(nrs_ctx* ctx, int32_t n_filters, const nrs_front_filter* filters, float clahe_clip, int32_t tiles_x,
                        int32_t tiles_y);
/* System::ImageProcessing (system.cc:189-201) + Masker::GetAllMasks (masker.cc:94-115) of one frame.  img: 8 bit, 1, 3 or 4
 * interleaved channels, row stride in bytes.  Every output pointer may be NULL; outputs are w x h bytes, rows packed.
 * filter_masks_out (NULL, or one pointer per configured filter, each of them nullable) receives the filters' masks in
 * configuration order: with global_out this is the GetAllMasks map.  Grey, CLAHE and Global stay resident in the context until
 * the next call or configuration.  NRS_ERR_INVALID: empty image, channels not 1 / 3 / 4, a PREDEFINED mask of another size, a
 * BorderFilter ROI (cb, rb, w-ce-cb, h-re-rb) that is empty or leaves the image. */
int nrs_front_process(nrs_ctx* ctx, const uint8_t* img, int32_t w, int32_t h, int32_t stride, int32_t channels, uint8_t* gray_out,
                      uint8_t* clahe_out, uint8_t* global_out, uint8_t* const* filter_masks_out);
/* Resident hand-over: nrs_klt_set_reference (LK:47-168), nrs_klt_track (LK:170-596) and nrs_shi_extract (shi_tomasi.cc:38-54 +
 * tracking.cc:118-134) on the frame the context already holds, so that a frame crosses the bus once.  The arguments are those of
 * the host-pointer forms without the image / mask pointers and their strides; `image` selects NRS_FRONT_IMAGE_GRAY or
 * NRS_FRONT_IMAGE_CLAHE; use_global_mask != 0 passes the resident Global mask where the host form takes a mask (the tracker's
 * Track takes none).  The same internals run on the resident buffers: results are bit for bit those of the host-pointer forms
 * fed the downloaded bytes (tests/test_gpu_front_resident.py).  NRS_ERR_STATE when no frame has been processed since the
 * context was created or configured, or when w x h is not the resident frame's size. */
int nrs_klt_set_reference_front(nrs_ctx* ctx, int32_t w, int32_t h, int32_t image, int32_t use_global_mask, int32_t n, const float* xy);
int nrs_klt_track_front(nrs_ctx* ctx, int32_t w, int32_t h, int32_t image, int32_t n, float* xy, int32_t* status,
                        int32_t use_initial_flow, float min_ssim, int32_t* n_good, float* ssim);
int nrs_shi_extract_front(nrs_ctx* ctx, int32_t w, int32_t h, int32_t image, int32_t use_global_mask, int32_t n_prev,
                          const float* prev_xy, int32_t capacity, float* out_xy, int32_t* out_id, int32_t* n_out);
/* The front end of System::TrackImageWithStereo (system.cc:134-160): ImageProcessing on BOTH images (:137-138), the masks from the
 * left one only (:144).  left / right: two images of the same size and channel count, each with its own row stride in bytes, each
 * uploaded once.  The left eye gets everything nrs_front_process does; the right eye gets the grey conversion and CLAHE and no mask.
 * The stages both eyes share -- grey, the CLAHE tile LUTs, the CLAHE blend -- run as ONE launch each over both eyes (the eye is the
 * grid's third dimension: 128 LUT workgroups where a frame gives 64); each eye's bytes are, byte for byte, what nrs_front_process
 * gives for that image alone (tests/test_gpu_front_stereo.py).  Outputs: those of nrs_front_process for the left eye, and
 * gray_right_out / clahe_right_out; every one may be NULL.
 * State: afterwards the left slot is exactly what nrs_front_process(left) leaves -- every nrs_*_front call above works on it
 * unchanged -- and the right eye's grey and CLAHE images are resident next to it for the nrs_*_front calls of the stereo section
 * below.  nrs_front_process (one image) invalidates the right slot; nrs_front_configure drops both.  The call synchronises the
 * context's stream before it returns: this is what makes the resident pair safe to read from ANOTHER context of the same device
 * (nrs_stereo_match_lk_front).  NRS_ERR_INVALID: the refusals of nrs_front_process, for either image. */
int nrs_front_process_stereo(nrs_ctx* ctx, const uint8_t* left, const uint8_t* right, int32_t w, int32_t h, int32_t stride_l, int32_t stride_r,
                             int32_t channels, uint8_t* gray_out, uint8_t* clahe_out, uint8_t* global_out, uint8_t* const* filter_masks_out,
                             uint8_t* gray_right_out, uint8_t* clahe_right_out);
/* Stereo rectification: what the reference's Hamlyn loader does to every pair before System::TrackImageWithStereo sees it
 * (modules/datasets/hamlyn.cc:194-198: stereoRectify + one initUndistortRectifyMap per eye, once; :226-229: cv::remap(INTER_LINEAR) of
 * both eyes, every frame), on the device, so that the RAW pair crosses the bus and the rectified one never does.  cv::stereoRectify
 * stays with the caller (a one-off on 3 x 3 matrices): an eye record takes its outputs.  The arithmetic is this project's definition
 * (DESIGN.md 4 "Stereo rectification"; parity with OpenCV unpinned: no OpenCV in the build, none of its source in the reference tree),
 * restated in tests/rect_oracle.py, to which the device is held bit for bit (maps) and byte for byte (images):
 *   map     per destination pixel, fp64: (X, Y, W) = (P R)^-1 (u, v, 1), the rational distortion model on (X/W, Y/W), K's focal lengths and
 *           centre; stored as fp32.  dist = k1 k2 p1 p2 k3 k4 k5 k6, unused entries 0 (the reference passes four, hamlyn.cc:194-198)
 *   remap   OpenCV's 8-bit INTER_LINEAR convention: the map times 32 rounded half to even, integer part saturated to int16, 5-bit fractions,
 *           integer tap weights that sum to 2^15, (sum + 2^14) >> 15; a tap outside the source is 0 (BORDER_CONSTANT 0, the default
 *           hamlyn.cc:226-229 takes); a non-finite map entry gives 0
 * row-major 3 x 3 matrices; of K only K[0], K[4], K[2], K[5] are used; P: the left 3 x 3 of stereoRectify's P1 / P2. */
typedef struct { double K[9], dist[8], R[9], P[9]; } nrs_rect_eye;
/* hamlyn.cc:194-198: builds both eyes' maps on the device (src_w x src_h raw eyes, dst_w x dst_h rectified ones) and drops the
 * resident frame.  nrs_front_configure keeps the maps (filters and rectification are independent); nrs_destroy frees them.
 * NRS_ERR_INVALID: a null eye, a size that is not in 1 .. 16384, a non-finite parameter, det(P R) == 0. */
int nrs_front_rectify_configure(nrs_ctx* ctx, int32_t src_w, int32_t src_h, int32_t dst_w, int32_t dst_h, const nrs_rect_eye* left,
                                const nrs_rect_eye* right);
/* The fp32 maps of eye 0 (left) or 1 (right), as initUndistortRectifyMap(CV_32FC1) would hand them over (hamlyn.cc:194-198):
 * dst_w x dst_h floats each, rows packed; either pointer may be NULL.  NRS_ERR_STATE before any nrs_front_rectify_configure. */
int nrs_front_rectify_maps(nrs_ctx* ctx, int32_t eye, float* map_x, float* map_y);
/* hamlyn.cc:226-229 followed by nrs_front_process_stereo: the raw eyes (src_w x src_h, 1 / 3 / 4 interleaved channels, a row stride in
 * bytes each) are uploaded once, remapped channel by channel and converted to grey in one launch over both eyes; from the CLAHE LUTs on
 * everything is nrs_front_process_stereo.  Outputs: exactly those of nrs_front_process_stereo, all dst_w x dst_h, and the rectified
 * images themselves, dst_w x dst_h x channels, rows packed (the colour pixel is written only when one of the two is asked for).  Every
 * output may be NULL.
 * State: afterwards the context is exactly what nrs_front_process_stereo leaves when fed the two rectified images: w x h is
 * dst_w x dst_h, every nrs_*_front call works on it unchanged, a PREDEFINED mask must have the rectified size.
 * NRS_ERR_STATE before any nrs_front_rectify_configure; NRS_ERR_INVALID: a raw size other than the configured src_w x src_h, and the
 * refusals of nrs_front_process_stereo. */
int nrs_front_process_stereo_raw(nrs_ctx* ctx, const uint8_t* left, const uint8_t* right, int32_t src_w, int32_t src_h, int32_t stride_l,
                                 int32_t stride_r, int32_t channels, uint8_t* gray_out, uint8_t* clahe_out, uint8_t* global_out,
                                 uint8_t* const* filter_masks_out, uint8_t* gray_right_out, uint8_t* clahe_right_out, uint8_t* rect_left_out,
                                 uint8_t* rect_right_out);
/* Frame resize: what the reference's Endomapper app does to every frame before System::TrackImage sees it (apps/endomapper.cc:65-69:
 * cv::resize(image, image, Size(cols / 2.0f, rows / 2.0f)), INTER_LINEAR), on the device, so that the frame crosses the bus as the video
 * decoder hands it over.  The arithmetic is this project's definition (DESIGN.md 4 "Frame resize"; parity with OpenCV unpinned: no OpenCV
 * in the build, none of its source in the reference tree), restated in tests/resize_oracle.py, to which the device is held byte for byte.
 * It follows OpenCV's 8-bit INTER_LINEAR conventions:
 *   box      iff src_w == 2 dst_w and src_h == 2 dst_h: per channel (s00 + s01 + s10 + s11 + 2) >> 2 over the 2 x 2 block
 *   general  every other size, up-scaling included.  scale = 1.0 / ((double)dst / src); f = (float)((d + 0.5) * scale - 0.5), s = floor(f),
 *            f -= s in fp32; weights sat_i16(rne((1.f - f) * 2048.f)), sat_i16(rne(f * 2048.f)), rne = round half to even.
 *            Columns: s < 0 -> s = 0, f = 0; s >= src_w - 1 -> s = src_w - 1, f = 0 (the second tap is not read).  Rows: the fraction
 *            stays, rows s and s + 1 are each clamped to [0, src_h - 1].  Per channel D_r = S[r][sx] a0 + S[r][sx + 1] a1 (int32),
 *            dst = sat_u8((((b0 (D_0 >> 4)) >> 16) + ((b1 (D_1 >> 4)) >> 16) + 2) >> 2)
 * The resize comes first, channel by channel; the grey conversion of nrs_front_process reads the resized pixel (the reference's order).
 *
 * nrs_front_resize_configure builds the tap tables (on the host, uploaded) and drops the resident frame.  nrs_front_configure and
 * nrs_front_rectify_configure leave the tables alone, and this call leaves the filters and the maps alone; nrs_destroy frees them.
 * NRS_ERR_INVALID: a size that is not in 1 .. 16384. */
int nrs_front_resize_configure(nrs_ctx* ctx, int32_t src_w, int32_t src_h, int32_t dst_w, int32_t dst_h);
/* The tables: sx [dst_w], ax [dst_w][2], sy [dst_h][2] (clamped), by [dst_h][2]; *box = 1 when the box branch applies (the tables are built
 * all the same), else 0.  Every pointer may be NULL.  NRS_ERR_STATE before any nrs_front_resize_configure. */
int nrs_front_resize_taps(nrs_ctx* ctx, int32_t* sx, int16_t* ax, int32_t* sy, int16_t* by, int32_t* box);
/* endomapper.cc:65-69 followed by nrs_front_process: the raw frame (src_w x src_h, 1 / 3 / 4 interleaved channels, a row stride in bytes)
 * is uploaded once, resized and converted to grey in one launch; from the CLAHE LUTs on everything is nrs_front_process.  Outputs: those
 * of nrs_front_process, all dst_w x dst_h, and the resized frame itself, dst_w x dst_h x channels, rows packed (the colour pixel is written
 * only when it is asked for).  Every output may be NULL.
 * State: afterwards the context is exactly what nrs_front_process leaves when fed the resized image: w x h is dst_w x dst_h, every
 * nrs_*_front call works on it unchanged, a PREDEFINED mask must have the resized size, no right eye is resident.
 * NRS_ERR_STATE before any nrs_front_resize_configure; NRS_ERR_INVALID: a raw size other than the configured src_w x src_h, and the
 * refusals of nrs_front_process. */
int nrs_front_process_raw(nrs_ctx* ctx, const uint8_t* img, int32_t src_w, int32_t src_h, int32_t stride, int32_t channels, uint8_t* gray_out,
                          uint8_t* clahe_out, uint8_t* global_out, uint8_t* const* filter_masks_out, uint8_t* resized_out);

/* ---- N2: the skinned mode ("5k points x 500 graph nodes") --------------------------------------------------------
 * The reference has no separate node set; its skinning is stage 2 of CameraPoseAndDeformationOptimization
 * (modules/optimization/g2o_optimization.cc:476-553, spatial_regularizer_fixed.cc:32-43): points of the frame that are not
 * optimised follow <= 11 optimised graph neighbours.  Skinned mode = that algorithm with a chosen node set: the nodes
 * keep NRS_TRACKED_WITH_3D, every other point of the frame is handed over as NRS_TRACKED (in the frame, no 3D), and
 * nrs_track_deform_solve / nrs_track_deform_solve_rg run unchanged.  Coverage is the reference's, not "every point": stage 2
 * carries the points of the lost set, i.e. the non-node points met during some node's GetEdges walk before that walk stops
 * (11 accepted node neighbours or the first BAD edge, OPT:255-279).  A non-node point outside every node's walked prefix is
 * not in `lost`, keeps its old position and its NRS_TRACKED status: callers find them as "status NRS_TRACKED and not listed
 * in lost" (farthest point sampling with n_nodes >= n_points / 10 leaves < 10 % of them on the synthetic frames).  This call chooses the nodes: farthest point
 * sampling over the eligible points (eligible == NULL: all), first pick = lowest eligible index, fp32 squared distances,
 * ties to the lowest index.  node_ids[n_nodes] in pick order.  NRS_ERR_INVALID if fewer points are eligible.
 * An eligible point with a NaN or +-inf coordinate is refused (NRS_ERR_INVALID, the message names the first one; host scan, nothing is
 * uploaded); a point that is not eligible may hold anything and cannot influence a pick. */
int nrs_skin_select_nodes(nrs_ctx* ctx, int32_t n_points, const float* pos /* n_points x 3 */, const uint8_t* eligible /* nullable */,
                          int32_t n_nodes, int32_t* node_ids);

/* ---- f6: monocular map initialisation -- EssentialMatrixInitialization::Initialize (modules/tracking/essential_matrix_initialization.cc:47-410),
 * the solve behind Tracking::MonocularMapInitialization (tracking.cc:136-214), in one call: the inputs are uploaded once, every stage runs
 * on the device, the outputs come back in one download.  The arithmetic is written down in DESIGN.md "f6".
 *   1 UnprojectTrackedFeatures (:83-103)   keypoints with status NRS_TRACKED become COMPACT indices in ascending order; rays are
 *                                          Unproject(...).normalized() in fp32, pinhole and KB8
 *   2 the sampler (:112-147)               8 clusters over the compact reference keypoints, one pick per cluster and hypothesis.  THIS PROJECT'S
 *                                          DEFINITION (the reference: cv::kmeans + srand(4) / random_shuffle; parity unpinned): farthest-point seeds
 *                                          (first = compact index 0, fp32 squared distances, ties to the lowest index), <= 10 Lloyd iterations
 *                                          that stop when no centre moved more than 1 px, labels by fp32 squared distance (ties to the lowest
 *                                          cluster), centres = fp64 sums rounded to fp32 (an empty cluster keeps its centre); hypothesis h takes
 *                                          from cluster c the member of rank splitmix64(seed + (8 h + c + 1) * 0x9E3779B97F4A7C15) mod |c| in
 *                                          ascending compact index (an empty cluster: that value mod the compact count, as a compact index)
 *   3 ComputeE (:180-206)                  A (8 x 9) in fp32 as written; its right null vector and the 3 x 3 SVD in fp64 (Jacobi), each rounded
 *                                          to fp32; Ef = -U diag(1,1,0) V^T.  The sign of E is free
 *   4 ComputeScoreAndInliers (:236-256)    every hypothesis over the first n_matches compact rays, fp32 in a fixed order; acos is the fp64
 *                                          function rounded to fp32.  Best = highest score, lowest h on ties (:154)
 *   5 ReconstructCameras (:284-318)        DecomposeEssentialMatrix in fp64, rounded; the smaller rotation by trace; t = U.col(2) with its
 *                                          component of the largest magnitude made positive (the reference: whatever sign Eigen's SVD returns),
 *                                          then the `away` test over the inlier rays
 *   6 ReconstructPoints (:320-410)         TriangulateMidPoint(ref, cur, I, T), parallax < 5 radians_per_pixel, depth and reprojection (5.991)
 *                                          gates in the reference's order, the counters and the two verdict tests
 * THE INDEXING QUIRK.  FindEssentialWithRANSAC fills the inlier flags by COMPACT index; ReconstructEnvironment / ReconstructPoints read
 * inliers[idx], reference_keypoints_[idx] and current_keypoints_[idx] by KEYPOINT index over idx < n_matches (:266-267, :331-338).
 * compact_indexing = 0 restates exactly that (with every keypoint TRACKED the two coincide); 1 reads keypoint compact_map[idx] instead.
 * Not built: RefineSolution (never called in the reference).  The DBSCAN labels of FeatureTracksClustering are nrs_flow_tracks_cluster,
 * below the solve. */
typedef struct {
    uint32_t struct_size;
    int32_t  n_hypotheses;        /* 0 = the reference's count, ComputeMaxTries(0.8, 0.95) = 16 (:78-81,130-132); 1..4096              */
    float    epipolar_threshold;  /* 0.005 rad (tracking.cc:66)                                                                       */
    float    radians_per_pixel;   /* the caller's (tracking.cc:65); nrs_init_options_init sets 0.0025                                  */
    int32_t  min_triangulated;    /* 100  (essential_matrix_initialization.cc:401)                                                    */
    float    max_low_parallax;    /* 0.25 (:405)                                                                                      */
    int32_t  compact_indexing;    /* 0 = index the inlier flags as the reference writes it (see above); 1 = through the compact map    */
    uint64_t seed;                /* the sampler's; nrs_init_options_init sets 4 (srand(4), :112)                                      */
} nrs_init_options;
/* Caller-owned; struct_size must be set; every pointer may be NULL. */
typedef struct {
    uint32_t struct_size;
    int32_t  verdict;             /* 0 ok; 1 fewer than 8 matches (:51); 2 fewer than min_triangulated landmarks (:401); 3 low-parallax share
                                     above max_low_parallax (:405)                                                                     */
    int32_t  best_hypothesis, score;
    int32_t  n_compact, n_hypotheses;   /* TRACKED keypoints; hypotheses run                                                           */
    int32_t  counters[8];         /* ReconstructPoints: N (inliers visited), n_triangulated, n_parallax, n_depth_1, n_reprojection_error_1,
                                     n_depth_2, n_reprojection_error_2, n_triangulation_error (always 0: TriangulateMidPoint never fails) */
    float    E[9];                /* the best hypothesis, row-major                                                                     */
    float    pose_qt[7];          /* camera_transform_world: qx qy qz qw tx ty tz, qw >= 0, |t| = 1                                     */
    uint8_t* inlier;              /* n_matches, by compact index                                                                        */
    float*   xyz;                 /* n x 3, by keypoint index; 0 where code != 0                                                        */
    int32_t* code;                /* n: 0 triangulated; 1 not an inlier or not visited; 2 low parallax; 3 negative depth in camera 1;
                                     4 reprojection in camera 1; 5 negative depth in camera 2; 6 reprojection in camera 2               */
    float*   hyp_E;               /* parity taps: n_hypotheses x 9                                                                      */
    int32_t* hyp_score;           /*              n_hypotheses                                                                          */
    int32_t* samples_out;         /*              n_hypotheses x 8 compact indices                                                      */
    int32_t* labels;              /*              n_compact (written by the library's sampler only)                                     */
    float*   centres;             /*              8 x 2     (likewise)                                                                  */
} nrs_init_result;
void nrs_init_options_init(nrs_init_options* opt);
/* ref_xy / cur_xy: n x 2 keypoints of the reference and the current image; status: n LandmarkStatus; n_matches: the tracker's count
 * (<= the number of TRACKED keypoints); samples: NULL = the library's sampler, else n_hypotheses x 8 compact indices.  Returns an NRS_*
 * code: a failed initialisation is a verdict, not an error.  NRS_ERR_INVALID: a wrong struct_size, n_hypotheses outside 0..4096,
 * n_matches above the TRACKED count, a sample index outside the compact range. */
int nrs_init_essential(nrs_ctx* ctx, const nrs_camera* cam, const nrs_init_options* opt, int32_t n, const float* ref_xy,
                       const float* cur_xy, const int32_t* status, int32_t n_matches, const int32_t* samples, nrs_init_result* out);

/* Flow-track clustering -- MonocularMapInitializer::FeatureTracksClustering (modules/tracking/monocular_map_initializer.cc:185-219) with
 * DbscanND (modules/utilities/dbscan.cc:106-131), which ProcessNewImage runs on every image between a reset and a start (:62-63) and whose
 * labels InitializationRefinement receives as track_labels (:238,260).  Arithmetic of record: DESIGN.md 4 "Flow-track clustering".
 *
 * The clustering over dim coordinates.  mlpack is not in the tree, so the rule is THIS PROJECT'S DEFINITION (parity unpinned), the one of
 * Dbscan3D (f8) at any dimension:
 *   data        n points of dim fp32 coordinates, point-major; 0 <= n <= NRS_DBSCAN_MAX_POINTS, 1 <= dim <= NRS_DBSCAN_MAX_DIM
 *   neighbour   j != i and d2(i, j) <= eps * eps; d2 = the fp64 sum over k = 0 .. dim-1, in ascending k, of (double(a_k) - double(b_k))^2:
 *               one product and one add per coordinate, the first product starts the sum, no contraction; eps * eps one double product;
 *               the boundary is inclusive; a pair with a non-finite d2 is no neighbour pair.  At dim = 3 this is, bit for bit, Dbscan3D's
 *               (dx*dx + dy*dy) + dz*dz
 *   core        at least min_points neighbours (the point itself is not counted)
 *   clusters    the connected components of the core points under the neighbour relation; raw labels 0, 1, ... in ascending order of a
 *               component's lowest-index core point; a non-core point with a core neighbour takes the lowest raw label among its core
 *               neighbours; every other point is noise, -1
 *   no ranking  DbscanND has none: the raw label is the label
 * label: n; counts: clusters, noise points.  NRS_ERR_INVALID: n outside 0..16384, dim outside 1..64, eps not finite or <= 0,
 * min_points < 1, a null pointer.  n = 0 succeeds with counts (0, 0).
 *
 * The flow tracks (:191-211).  A track is `length` keypoints (2 <= length <= 33), its point has dim = 2 (length - 1) coordinates:
 * coordinate 2(t-1) is x_t - x_(t-1) and coordinate 2(t-1)+1 is y_t - y_(t-1), each ONE fp32 subtraction (cv::Point2f::operator-).
 * eps = double(float(0.1 * double(dim))) -- the reference stores the product in a float -- and min_points = 10 (:212-213).  Only tracks of the
 * maximal length take part (:194); the caller passes them in ascending feature index (the reference iterates a hash map whose order nothing
 * fixes).  DEPARTURE: InitializationRefinement reads feature_labels[idx] by KEYPOINT index although the vector is in full-length-track
 * order (:260); that misindexing is not reproduced, a track's label is its own.
 * flows_out (nullable): n_tracks x dim, the points that were clustered.  NRS_ERR_INVALID: n_tracks outside 0..16384, length outside 2..33, a
 * null pointer.
 *
 * Each call: one upload, every stage on the context's stream and scratch, one packed download.  The neighbour stage streams the candidates
 * through LDS tiles of 64 points; NRS_DBND_NO_TILE (nrs_debug_set) selects its plain form, the same bits. */
#define NRS_DBSCAN_MAX_DIM 64
int nrs_dbscan_nd(nrs_ctx* ctx, int32_t n, int32_t dim, const float* data /* n x dim */, double eps, int32_t min_points,
                  int32_t* label /* n */, int32_t counts[2] /* clusters, noise points */);
int nrs_flow_tracks_cluster(nrs_ctx* ctx, int32_t n_tracks, int32_t length, const float* tracks_xy /* n x length x 2 */,
                            float* flows_out /* nullable: n x 2(length-1) */, int32_t* label, int32_t counts[2]);

/* ---- f7: evaluation -- FrameEvaluator (modules/utilities/frame_evaluator.cc) and its two sources of ground truth, the stereo matchers
 * (modules/stereo/) and a depth image.  Arithmetic and the stated departures: DESIGN.md 4 "Evaluation (f7)".  Per-point status: */
typedef enum {
    NRS_EVAL_OK = 0,
    NRS_EVAL_OUT_OF_BOUNDS = 1,      /* either boundary test of the pattern matcher; the last column / row of a depth image             */
    NRS_EVAL_SATURATED = 2,          /* template maximum above 250                                                                    */
    NRS_EVAL_LOW_CORRELATION = 3,    /* best CCORR_NORMED below 0.99                                                                  */
    NRS_EVAL_ZERO_DISPARITY = 4,     /* departure: the reference returns +-inf here and aborts later in the evaluator's CHECK          */
    NRS_EVAL_BAD_DEPTH = 5,          /* interpolated depth not finite                                                                 */
    NRS_EVAL_NOT_TRACKED = 6,        /* LK stereo: the tracker's status is not NRS_TRACKED                                            */
    NRS_EVAL_ROW_DIFFERENCE = 7      /* LK stereo: |dy| > 2                                                                           */
} nrs_eval_status;

/* StereoPatternMatching::computeStereo3D for n keypoints (stereo_pattern_matching.cc:33-94): 15 x 15 template of the left image around
 * (int)(x-7), (int)(y-7), TM_CCORR_NORMED against the search region (0, 0, w-3, 2*(int)((h-1)/2.f-2)) of the right image, first
 * row-major maximum, rejected below 0.99.  Sums are exact integers, the score is fp64 (0 where a norm is 0).  cam supplies fx fy cx cy;
 * bf is the matcher's baseline_.  xyz of a rejected point is NaN; score / match_xy (top-left corner of the best window) are NaN / -1
 * for status 1 and 2.  Strides in bytes.  NRS_STEREO_NO_MFMA=1 (nrs_debug_set) selects the plain integer form of the correlation.
 * NRS_ERR_INVALID: an image smaller than 32 x 32 (no search position left). */
int nrs_stereo_match_pattern(nrs_ctx* ctx, const nrs_camera* cam, float bf, const uint8_t* left, const uint8_t* right, int32_t w, int32_t h,
                             int32_t stride_l, int32_t stride_r, int32_t n, const float* xy, float* xyz, int32_t* status, double* score,
                             int32_t* match_xy);

/* The precomputed_depth_ branch of FrameEvaluator::ComputeGroundTruth (frame_evaluator.cc:265-278): Interpolate (geometry_toolbox.h:47-60)
 * of an fp32 depth image (stride in floats) at the keypoint, times Unproject(keypoint) / its z.  Status 1 for x < 0, y < 0, x >= w-1 or
 * y >= h-1 (departure: the reference reads past the image), 5 for a depth that is not finite; gt_xyz is NaN for both. */
int nrs_eval_depth_ground_truth(nrs_ctx* ctx, const nrs_camera* cam, const float* depth, int32_t w, int32_t h, int32_t stride, int32_t n,
                                const float* xy, float* gt_xyz, int32_t* gt_status);

/* The loop of StereoLucasKanade::ComputeStereo3D (stereo_lucas_kanade.cc:50-72) on the tracker's output; the matcher itself is
 * nrs_klt_set_reference(left) + nrs_klt_track(right, use_initial_flow = 1, min_ssim = 0.5) on a context kept for stereo.
 * Host code, no context. */
int nrs_stereo_from_tracks(const nrs_camera* cam, float bf, int32_t n, const float* left_xy, const float* right_xy,
                           const int32_t* track_status, float* xyz, int32_t* status);

/* ComputeReconstructionRMSE / ComputeRMSEWithScaleAlignment / ComputeRMSEWithoutScaleAlignment (frame_evaluator.cc:54-226) on the depths
 * of the points with gt_ok != 0.  counts: valid, kept by the IQR gate, n_inliers.  inlier (nullable): n flags of the last iteration.
 * Host code, no context.  NRS_ERR_INVALID with rmse = scale = NaN when n_inliers < 1 or no point is valid. */
int nrs_eval_rmse(int32_t n, const float* est_z, const float* gt_z, const uint8_t* gt_ok, int32_t align_scales, int32_t precomputed_depth,
                  float* rmse, float* scale, int32_t counts[3], uint8_t* inlier);

/* EvaluateFrameReconstruction + SaveGroundTruthToFrame (frame_evaluator.cc:35-52, 291-305) for the n TRACKED_WITH_3D points of a frame:
 * pose_qt = T_camera_world (xyzw, t) in float, world_xyz their positions, xy their keypoints.  Ground truth: a depth image (depth != NULL:
 * nrs_eval_depth_ground_truth on ctx, precomputed_depth semantics) or gt_xyz / gt_status of a stereo matcher (ctx may be NULL then).
 * The camera-frame depth is the z row of the SE3f action (host function se3f_act_z of csrc/nrs_eval_host.hpp, the arithmetic of se3f_act
 * in py/nrs_frame_loop.py).  Outputs: nrs_eval_rmse's rmse / scale / counts, gt_world = T^-1 * (gt / scale) (n x 3, NaN without ground
 * truth; nullable) and gt_status_out (n; nullable).  An nrs_eval_rmse failure is returned as is, with gt_status_out filled. */
int nrs_eval_frame(nrs_ctx* ctx, const nrs_camera* cam, const float pose_qt[7], int32_t n, const float* world_xyz, const float* xy,
                   const float* depth, int32_t w, int32_t h, int32_t stride, const float* gt_xyz, const int32_t* gt_status,
                   float* rmse, float* scale, int32_t counts[3], float* gt_world, int32_t* gt_status_out);

/* ---- f8: stereo map initialisation -- Tracking::StereoMapInitialization (modules/tracking/tracking.cc:216-289) with Dbscan3D
 * (modules/utilities/dbscan.cc:61-104).  Arithmetic of record: DESIGN.md 4 "Stereo map initialisation".
 *
 * nrs_dbscan3d.  mlpack is not in the tree, so the clustering rule is THIS PROJECT'S DEFINITION (parity unpinned):
 *   neighbour   j != i and d2(i, j) <= eps * eps; d2 = (dx*dx + dy*dy) + dz*dz in fp64 on the fp32 coordinates converted to double, no
 *               contraction; eps * eps one double product; the boundary is inclusive; a pair with a non-finite d2 is no neighbour pair
 *   core        at least min_points neighbours (the point itself is not counted)
 *   clusters    the connected components of the core points under the neighbour relation; raw labels 0, 1, ... in ascending order of a
 *               component's lowest-index core point; a non-core point with a core neighbour takes the lowest raw label among its core
 *               neighbours; every other point is noise, -1
 *   ranking     (dbscan.cc:80-101) classes by raw label, size descending, ties by ascending raw key; with noise_competes = 1 noise is a
 *               class with key -1 (as in the reference's std::map), with 0 noise keeps -1 and is never rank 0.  The reference's tie
 *               comparator compares a label with a size (p1.first < p2.second): it is no ordering and is not reproduced
 * raw_label (nullable) / label: n each; counts: clusters, noise points, size of label 0.  n up to 16384.  NRS_ERR_INVALID: n outside
 * 0..16384, eps not finite or <= 0, min_points < 1, a null pointer. */
#define NRS_DBSCAN_MAX_POINTS 16384
int nrs_dbscan3d(nrs_ctx* ctx, int32_t n, const float* xyz /* n x 3 */, double eps, int32_t min_points, int32_t noise_competes,
                 int32_t* raw_label /* n, nullable */, int32_t* label /* n */, int32_t counts[3]);

typedef struct {
    uint32_t struct_size;
    float    bf;                  /* 3886.37: the matcher's baseline_ (baseline times focal length)                                     */
    float    z_min, z_max;        /* 35.5, 70.5: the depth gate, both ends excluded (tracking.cc:229-233)                               */
    double   eps;                 /* 2.5                                                                                                */
    int32_t  min_points;          /* 5                                                                                                  */
    int32_t  noise_competes;      /* 1: the reference's behaviour, noise can be the winning class                                       */
} nrs_init_stereo_options;
/* Caller-owned; struct_size must be set; every pointer may be NULL. */
typedef struct {
    uint32_t struct_size;
    int32_t  verdict;             /* 0 ok; 1 no keypoint passed the gate (the reference would read an empty vector)                     */
    int32_t  n_matched, n_gated, n_clusters, n_noise, n_selected;
    float    median_depth;        /* nth_element at n_selected / 2 of the selected z (:239-248); NaN when nothing is selected           */
    float*   xyz;                 /* n x 3: the matcher's, NaN where match_status != 0                                                  */
    int32_t* match_status;        /* n, nrs_eval_status                                                                                 */
    int32_t* code;                /* n: 0 selected; 1 matcher rejected; 2 depth outside the gate; 3 clustered but not rank 0            */
    int32_t* raw_label;           /* n: nrs_dbscan3d's raw label of the gated points, -2 for codes 1 and 2                              */
    int32_t* label;               /* n: the rank, likewise                                                                              */
    int32_t* selected;            /* n (n_selected written): keypoint indices of the rank-0 points in keypoint order                    */
    float*   selected_xyz;        /* n x 3 (n_selected rows written)                                                                    */
} nrs_init_stereo_result;
void nrs_init_stereo_options_init(nrs_init_stereo_options* opt);
/* One upload of the two images and the keypoints, every stage on the device, one packed download:
 *   1 the kernels of nrs_stereo_match_pattern (:226-228)     2 gate: status OK and z_min < z < z_max, float against float, a NaN
 *   fails; survivors compacted stably in keypoint order (:229-233)     3 nrs_dbscan3d's kernels on them     4 the rank-0 points in
 *   keypoint order (:254-263)     5 median_depth.  scale is the reference's constant 1.
 * A verdict is not an error.  NRS_ERR_INVALID: a wrong struct_size, the matcher's own refusals, n > 16384, eps not finite or <= 0,
 * min_points < 1, z_min >= z_max (or either NaN). */
int nrs_init_stereo(nrs_ctx* ctx, const nrs_camera* cam, const nrs_init_stereo_options* opt, const uint8_t* left, const uint8_t* right,
                    int32_t w, int32_t h, int32_t stride_l, int32_t stride_r, int32_t n, const float* xy, nrs_init_stereo_result* out);

/* ---- the resident stereo pair: the stages of System::TrackImageWithStereo (system.cc:134-160) joined on the device.  After
 * nrs_front_process_stereo both eyes lie in the context; the calls below read them where they lie, so each image crosses the bus
 * once.  Each takes the arguments of its host-pointer form without the image pointers and strides, plus w, h and `image`
 * (NRS_FRONT_IMAGE_GRAY or NRS_FRONT_IMAGE_CLAHE, applied to both eyes), runs the same internals and gives bit for bit what the
 * host-pointer form gives on the downloaded bytes (tests/test_gpu_front_stereo.py).  NRS_ERR_STATE when no pair is resident (none
 * processed, a one-image nrs_front_process or nrs_front_configure since) or when w x h is not the resident pair's size.
 *
 * nrs_stereo_match_pattern_front: StereoPatternMatching::computeStereo3D (stereo_pattern_matching.cc:33-94), the launches of
 *   nrs_stereo_match_pattern; NRS_STEREO_NO_MFMA selects the plain correlation here too.
 * nrs_init_stereo_front: Tracking::StereoMapInitialization (tracking.cc:216-263), the stages and the packed download of
 *   nrs_init_stereo; only the keypoints go up.
 * nrs_stereo_match_lk_front: StereoLucasKanade::ComputeStereo3D (stereo_lucas_kanade.cc:38-75): SetReferenceImage (no mask) on the
 *   resident left eye of ctx_front, Track (initial flow, min_ssim) on its resident right eye -- both in the tracker state of
 *   ctx_tracker -- and the loop of nrs_stereo_from_tracks on the tracks.  right_xy (n x 2) / track_status (n): the tracker's output.
 *   The two contexts may be the same one: the call then REPLACES its tracking templates (the reference's matcher owns a tracker of
 *   its own, SLAM/system.cc:45-54: keep a context for stereo, as for nrs_klt_set_reference + nrs_klt_track).  Two different contexts
 *   must be on the same device (NRS_ERR_INVALID otherwise; the precedent is nrs_klt_insert_archived); the read of ctx_front's
 *   buffers is ordered by the stream synchronisation at the end of nrs_front_process_stereo, and ctx_front must not process another
 *   frame while the call runs.  Errors are reported on ctx_tracker. */
int nrs_stereo_match_pattern_front(nrs_ctx* ctx, const nrs_camera* cam, float bf, int32_t w, int32_t h, int32_t image, int32_t n,
                                   const float* xy, float* xyz, int32_t* status, double* score, int32_t* match_xy);
int nrs_init_stereo_front(nrs_ctx* ctx, const nrs_camera* cam, const nrs_init_stereo_options* opt, int32_t w, int32_t h, int32_t image,
                          int32_t n, const float* xy, nrs_init_stereo_result* out);
int nrs_stereo_match_lk_front(nrs_ctx* ctx_tracker, nrs_ctx* ctx_front, const nrs_camera* cam, float bf, int32_t w, int32_t h, int32_t image,
                              int32_t n, const float* xy, float min_ssim, float* xyz, int32_t* status, float* right_xy,
                              int32_t* track_status);

#ifdef __cplusplus
}
#endif
#endif /* NRS_H */
