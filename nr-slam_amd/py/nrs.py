"""ctypes binding of libnrs_hip.so (include/nrs.h) for the tests and bench.py.

Thin by design: every function maps 1:1 onto a C-ABI entry point, takes/returns NumPy arrays and
raises NrsError (with nrs_last_error) on a non-zero status.  There is no fallback: if the
shared library is missing the import fails; if no HIP device is usable nrs_create fails.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NRS_LIB") or os.path.join(os.path.dirname(_HERE), "libnrs_hip.so")

OK = 0
STATUS_NAMES = {0: "NRS_OK", -1: "NRS_ERR_INVALID", -2: "NRS_ERR_NO_DEVICE", -3: "NRS_ERR_HIP",
                -4: "NRS_ERR_ALLOC", -5: "NRS_ERR_STATE", -6: "NRS_ERR_NUMERIC", -7: "NRS_ERR_COMM"}
COMM_ID_BYTES = 128

# every symbol include/nrs.h declares (tests check that the library exports all of them)
SYMBOLS = ["nrs_create", "nrs_options_init", "nrs_destroy", "nrs_last_error", "nrs_device_name", "nrs_get_profile",
           "nrs_reset_profile", "nrs_stream", "nrs_pose_only_solve", "nrs_dba_build_edges",
           "nrs_dba_solve", "nrs_dba_upload", "nrs_dba_build_edges_embedded", "nrs_dba_upload_embedded", "nrs_dba_download_skinned", "nrs_dba_solve_embedded", "nrs_dba_reset", "nrs_dba_optimize",
           "nrs_dba_download", "nrs_dba_residuals", "nrs_dba_gradient", "nrs_dba_pack_hash", "nrs_dba_solve_window", "nrs_dba_window_edges", "nrs_dba_solve_window_embedded", "nrs_dba_window_edges_embedded", "nrs_dba_window_slice_embedded", "nrs_shard_plan_counts", "nrs_debug_pcg_solve", "nrs_debug_kft", "nrs_debug_set", "nrs_debug_nd_solve", "nrs_debug_nd_cache_stats", "nrs_track_deform_solve_embedded",
           "nrs_graph_select_neighbours", "nrs_graph_update", "nrs_track_deform_solve",
           "nrs_klt_configure", "nrs_klt_clear", "nrs_klt_num_points", "nrs_klt_set_reference",
           "nrs_klt_track", "nrs_klt_get_template", "nrs_klt_insert_template", "nrs_klt_get_templates",
           "nrs_klt_insert_templates", "nrs_klt_archive_templates", "nrs_klt_insert_archived", "nrs_point_reuse",
           "nrs_shi_configure", "nrs_shi_extract", "nrs_shi_buffers",
           "nrs_front_configure", "nrs_front_process", "nrs_klt_set_reference_front", "nrs_klt_track_front", "nrs_shi_extract_front",
           "nrs_comm_unique_id", "nrs_comm_init_rccl", "nrs_comm_rank", "nrs_shard_plan",
           "nrs_local_group_create", "nrs_local_group_destroy", "nrs_comm_init_local",
           "nrs_rgraph_create", "nrs_rgraph_destroy", "nrs_rgraph_set_sigma", "nrs_rgraph_min_weight", "nrs_rgraph_add_edges",
           "nrs_rgraph_update", "nrs_rgraph_get_edges", "nrs_rgraph_edge", "nrs_rgraph_rows", "nrs_rgraph_resize", "nrs_triangulate_batch", "nrs_map_frame", "nrs_map_grow_graph", "nrs_track_deform_solve_rg", "nrs_dba_solve_window_rg", "nrs_dba_window_rg_stats", "nrs_dba_solve_window_rg_embedded",
           "nrs_skin_select_nodes", "nrs_dba_stats", "nrs_dba_skin_stats",
           "nrs_init_options_init", "nrs_init_essential", "nrs_dbscan_nd", "nrs_flow_tracks_cluster",
           "nrs_stereo_match_pattern", "nrs_eval_depth_ground_truth", "nrs_stereo_from_tracks", "nrs_eval_rmse", "nrs_eval_frame",
           "nrs_dbscan3d", "nrs_init_stereo_options_init", "nrs_init_stereo",
           "nrs_front_process_stereo", "nrs_stereo_match_pattern_front", "nrs_init_stereo_front", "nrs_stereo_match_lk_front",
           "nrs_front_rectify_configure", "nrs_front_rectify_maps", "nrs_front_process_stereo_raw",
           "nrs_front_resize_configure", "nrs_front_resize_taps", "nrs_front_process_raw",
           "nrs_tbuf_create", "nrs_tbuf_destroy", "nrs_tbuf_clear", "nrs_tbuf_insert", "nrs_tbuf_info", "nrs_tbuf_flat", "nrs_map_frame_tbuf"]


class NrsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (STATUS_NAMES.get(code, "?"), code, msg))
        self.code = code


class Camera(C.Structure):
    _fields_ = [("model", C.c_int32), ("params", C.c_float * 8)]


# ---- debug / A-B switches (include/nrs.h "Debug switches"): a context reads the NRS_* environment ONCE when it is created; afterwards they are
# changed through nrs_debug_set only.  debug_set() here applies a switch to every live Context of this process and to the ones created later.
import weakref
_DEBUG = {}
_LIVE = weakref.WeakSet()


def debug_set(name, value):
    """value None: unset.  (tests / probes: the replacement of os.environ[name] = value for a library that no longer reads the environment per call)"""
    if value is None:
        _DEBUG.pop(name, None)
    else:
        _DEBUG[name] = str(value)
    for c in list(_LIVE):
        c.debug_set(name, value)


def debug_clear():
    for k in list(_DEBUG):
        debug_set(k, None)


class Options(C.Structure):
    _fields_ = [("device", C.c_int32), ("struct_size", C.c_uint32), ("pcg_rtol", C.c_double), ("pcg_max_iters", C.c_int32),
                ("pcg_batch", C.c_int32), ("profile", C.c_int32), ("exact_trials", C.c_int32), ("direct_solve", C.c_int32),
                ("embedded_solver", C.c_int32), ("sharded_kft", C.c_int32)]


class LmTrial(C.Structure):
    _fields_ = [("round", C.c_int32), ("iter", C.c_int32), ("trial", C.c_int32),
                ("accepted", C.c_int32), ("solver_ok", C.c_int32), ("inner_iters", C.c_int32),
                ("early_rejected", C.c_int32), ("reserved", C.c_int32),
                ("lam", C.c_double), ("chi2", C.c_double), ("chi2_new", C.c_double),
                ("rho", C.c_double)]


class LmTrace(C.Structure):
    _fields_ = [("trials", C.POINTER(LmTrial)), ("capacity", C.c_int32), ("count", C.c_int32),
                ("iterations", C.c_int32)]


class Graph(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("rowptr", C.POINTER(C.c_int32)), ("col", C.POINTER(C.c_int32)),
                ("eid", C.POINTER(C.c_int32)), ("n_edges", C.c_int32), ("e_w", C.POINTER(C.c_float)),
                ("e_d0", C.POINTER(C.c_float)), ("e_max", C.POINTER(C.c_float)), ("e_min", C.POINTER(C.c_float)),
                ("e_status", C.POINTER(C.c_int32)), ("sigma", C.c_float), ("stretch_th", C.c_float)]


class KltConfig(C.Structure):
    _fields_ = [("win_size", C.c_int32), ("max_level", C.c_int32), ("max_iters", C.c_int32),
                ("epsilon", C.c_float), ("min_eig_threshold", C.c_float)]


class FrontFilter(C.Structure):
    """nrs_front_filter: kind, five ints, and for PREDEFINED a host mask with w, h, stride"""
    _fields_ = [("kind", C.c_int32), ("p", C.c_int32 * 5), ("mask", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32),
                ("stride", C.c_int32)]


FRONT_BRIGHT, FRONT_BORDER, FRONT_PREDEFINED = 0, 1, 2
FRONT_GRAY, FRONT_CLAHE = 0, 1


class RectEye(C.Structure):
    """nrs_rect_eye: K, dist (k1 k2 p1 p2 k3 k4 k5 k6), R, P -- doubles, the matrices row-major"""
    _fields_ = [("K", C.c_double * 9), ("dist", C.c_double * 8), ("R", C.c_double * 9), ("P", C.c_double * 9)]


def make_rect_eye(eye):
    """a RectEye, or a dict(K=3x3, dist=up to 8 numbers, R=3x3, P=3x3) (the form of tests/rect_oracle.py) -> RectEye; None stays None"""
    if eye is None or isinstance(eye, RectEye):
        return eye
    r = RectEye()
    for name in ("K", "R", "P"):
        getattr(r, name)[:] = [float(v) for v in np.asarray(eye[name], np.float64).reshape(9)]
    dist = [float(v) for v in np.asarray(eye.get("dist", ()), np.float64).ravel()]
    if len(dist) > 8:
        raise ValueError("at most 8 distortion coefficients (k1 k2 p1 p2 k3 k4 k5 k6)")
    r.dist[:] = dist + [0.0] * (8 - len(dist))
    return r


def half_size(w, h):
    """the newSize of the reference's Endomapper app (apps/endomapper.cc:65-69: cv::Size(cols / 2.0f, rows / 2.0f), truncated) -> (w, h)"""
    return int(np.float32(w) / np.float32(2)), int(np.float32(h) / np.float32(2))


class InitOptions(C.Structure):
    """nrs_init_options (f6)"""
    _fields_ = [("struct_size", C.c_uint32), ("n_hypotheses", C.c_int32), ("epipolar_threshold", C.c_float), ("radians_per_pixel", C.c_float),
                ("min_triangulated", C.c_int32), ("max_low_parallax", C.c_float), ("compact_indexing", C.c_int32), ("seed", C.c_uint64)]


class InitResult(C.Structure):
    """nrs_init_result (f6): scalars in the record, arrays through caller-owned pointers (each nullable)"""
    _fields_ = [("struct_size", C.c_uint32), ("verdict", C.c_int32), ("best_hypothesis", C.c_int32), ("score", C.c_int32),
                ("n_compact", C.c_int32), ("n_hypotheses", C.c_int32), ("counters", C.c_int32 * 8), ("E", C.c_float * 9),
                ("pose_qt", C.c_float * 7), ("inlier", C.c_void_p), ("xyz", C.c_void_p), ("code", C.c_void_p), ("hyp_E", C.c_void_p),
                ("hyp_score", C.c_void_p), ("samples_out", C.c_void_p), ("labels", C.c_void_p), ("centres", C.c_void_p)]


class InitStereoOptions(C.Structure):
    """nrs_init_stereo_options (f8)"""
    _fields_ = [("struct_size", C.c_uint32), ("bf", C.c_float), ("z_min", C.c_float), ("z_max", C.c_float), ("eps", C.c_double),
                ("min_points", C.c_int32), ("noise_competes", C.c_int32)]


class InitStereoResult(C.Structure):
    """nrs_init_stereo_result (f8): scalars in the record, arrays through caller-owned pointers (each nullable)"""
    _fields_ = [("struct_size", C.c_uint32), ("verdict", C.c_int32), ("n_matched", C.c_int32), ("n_gated", C.c_int32), ("n_clusters", C.c_int32),
                ("n_noise", C.c_int32), ("n_selected", C.c_int32), ("median_depth", C.c_float), ("xyz", C.c_void_p), ("match_status", C.c_void_p),
                ("code", C.c_void_p), ("raw_label", C.c_void_p), ("label", C.c_void_p), ("selected", C.c_void_p), ("selected_xyz", C.c_void_p)]


SINIT_OK, SINIT_NOTHING_GATED = 0, 1
SINIT_SELECTED, SINIT_MATCHER_REJECTED, SINIT_OUTSIDE_GATE, SINIT_OTHER_CLUSTER = 0, 1, 2, 3
DBSCAN_MAX_POINTS = 16384
DBSCAN_MAX_DIM = 64
FLOW_MIN_LENGTH, FLOW_MAX_LENGTH, FLOW_MIN_POINTS = 2, 33, 10

INIT_OK, INIT_FEW_MATCHES, INIT_FEW_LANDMARKS, INIT_LOW_PARALLAX = 0, 1, 2, 3
INIT_COUNTERS = ("N", "n_triangulated", "n_parallax", "n_depth_1", "n_reprojection_error_1", "n_depth_2", "n_reprojection_error_2",
                 "n_triangulation_error")


class Profile(C.Structure):
    _fields_ = [("linearize_ms", C.c_double), ("linearize_launches", C.c_int64),
                ("spmv_ms", C.c_double), ("spmv_launches", C.c_int64),
                ("vec_ms", C.c_double), ("vec_launches", C.c_int64),
                ("update_ms", C.c_double), ("update_launches", C.c_int64)]


def load_library(path=LIB_PATH):
    if not os.path.exists(path):
        raise ImportError("libnrs_hip.so not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C nr-slam_amd`): %s" % path)
    lib = C.CDLL(path)
    lib.nrs_last_error.restype = C.c_char_p
    lib.nrs_stream.restype = C.c_void_p
    lib.nrs_destroy.restype = None
    lib.nrs_local_group_destroy.restype = None
    lib.nrs_rgraph_destroy.restype = None
    lib.nrs_rgraph_destroy.argtypes = [C.c_void_p]
    lib.nrs_rgraph_min_weight.restype = C.c_float
    lib.nrs_rgraph_min_weight.argtypes = [C.c_void_p]
    lib.nrs_local_group_destroy.argtypes = [C.c_void_p]
    lib.nrs_comm_init_local.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    # the resident stereo pair (include/nrs.h "the resident stereo pair")
    i32, f32, ptr = C.c_int32, C.c_float, C.c_void_p
    lib.nrs_front_process_stereo.argtypes = [ptr, ptr, ptr, i32, i32, i32, i32, i32, ptr, ptr, ptr, ptr, ptr, ptr]
    lib.nrs_stereo_match_pattern_front.argtypes = [ptr, ptr, f32, i32, i32, i32, i32, ptr, ptr, ptr, ptr, ptr]
    lib.nrs_init_stereo_front.argtypes = [ptr, ptr, ptr, i32, i32, i32, i32, ptr, ptr]
    lib.nrs_stereo_match_lk_front.argtypes = [ptr, ptr, ptr, f32, i32, i32, i32, i32, ptr, f32, ptr, ptr, ptr, ptr]
    # stereo rectification (include/nrs.h "Stereo rectification")
    lib.nrs_front_rectify_configure.argtypes = [ptr, i32, i32, i32, i32, ptr, ptr]
    lib.nrs_front_rectify_maps.argtypes = [ptr, i32, ptr, ptr]
    lib.nrs_front_process_stereo_raw.argtypes = [ptr, ptr, ptr, i32, i32, i32, i32, i32, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]
    # frame resize (include/nrs.h "Frame resize")
    lib.nrs_front_resize_configure.argtypes = [ptr, i32, i32, i32, i32]
    lib.nrs_front_resize_taps.argtypes = [ptr, ptr, ptr, ptr, ptr, ptr]
    lib.nrs_front_process_raw.argtypes = [ptr, ptr, i32, i32, i32, i32, ptr, ptr, ptr, ptr, ptr]
    # flow-track clustering (include/nrs.h "f6")
    lib.nrs_dbscan_nd.argtypes = [ptr, i32, i32, ptr, C.c_double, i32, ptr, ptr]
    lib.nrs_flow_tracks_cluster.argtypes = [ptr, i32, i32, ptr, ptr, ptr, ptr]
    # the resident temporal buffer (include/nrs.h "The resident TemporalBuffer")
    lib.nrs_tbuf_create.argtypes = [ptr, i32, ptr]
    lib.nrs_tbuf_destroy.restype = None
    lib.nrs_tbuf_destroy.argtypes = [ptr]
    lib.nrs_tbuf_clear.argtypes = [ptr]
    lib.nrs_tbuf_insert.argtypes = [ptr, i32, ptr, ptr, ptr, ptr, ptr, ptr, f32]
    lib.nrs_tbuf_info.argtypes = [ptr, ptr, ptr, ptr]
    lib.nrs_tbuf_flat.argtypes = [ptr] + [ptr] * 8
    lib.nrs_map_frame_tbuf.argtypes = [ptr, ptr, ptr, f32, f32, i32, i32] + [ptr] * 10
    return lib


def comm_unique_id(lib=None):
    """RCCL unique id (bytes) made on rank 0; the caller broadcasts it (torch.distributed, MPI, a file ...)."""
    lib = lib or load_library()
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    rc = lib.nrs_comm_unique_id(buf, C.c_int32(COMM_ID_BYTES))
    if rc != OK:
        raise NrsError(rc, "nrs_comm_unique_id (is librccl loadable?)")
    return bytes(buf)


def shard_plan(n_kf, lm_kf, world, lib=None):
    """Keyframe ranges of a sharded BA window (host only)."""
    lib = lib or load_library()
    lm_kf = _i32(lm_kf)
    kb = np.zeros(world + 1, np.int32)
    rc = lib.nrs_shard_plan(C.c_int32(n_kf), C.c_int32(len(lm_kf)), _p(lm_kf, C.c_int32), C.c_int32(world), _p(kb, C.c_int32))
    if rc != OK:
        raise NrsError(rc, "nrs_shard_plan")
    return kb


def shard_plan_counts(kf_vertices, world, lib=None):
    """The same ranges from the number of vertices of every keyframe (include/nrs.h nrs_shard_plan_counts; host only)."""
    lib = lib or load_library()
    cnt = _i32(kf_vertices)
    kb = np.zeros(world + 1, np.int32)
    rc = lib.nrs_shard_plan_counts(C.c_int32(len(cnt)), _p(cnt, C.c_int32), C.c_int32(world), _p(kb, C.c_int32))
    if rc != OK:
        raise NrsError(rc, "nrs_shard_plan_counts")
    return kb


# ---- f7: evaluation (include/nrs.h "f7: evaluation").  nrs_eval_status:
EVAL_OK, EVAL_OUT_OF_BOUNDS, EVAL_SATURATED, EVAL_LOW_CORRELATION, EVAL_ZERO_DISPARITY, EVAL_BAD_DEPTH, EVAL_NOT_TRACKED, EVAL_ROW_DIFFERENCE = range(8)


def eval_rmse(est_z, gt_z, gt_ok, align_scales=True, precomputed_depth=False, lib=None):
    """nrs_eval_rmse (host only).  -> (rmse, scale, (valid, kept, n_inliers), inlier mask, rc); rc = -1 (NRS_ERR_INVALID) where no RMSE
    exists (rmse and scale are NaN then)"""
    lib = lib or load_library()
    est, gt, ok = _f32(est_z), _f32(gt_z), np.ascontiguousarray(gt_ok, np.uint8)
    n = len(est)
    assert len(gt) == n and len(ok) == n
    rmse, scale = C.c_float(0), C.c_float(0)
    counts = (C.c_int32 * 3)()
    inl = np.zeros(n, np.uint8)
    rc = lib.nrs_eval_rmse(C.c_int32(n), _p(est, C.c_float), _p(gt, C.c_float), _p(ok, C.c_uint8), C.c_int32(1 if align_scales else 0),
                           C.c_int32(1 if precomputed_depth else 0), C.byref(rmse), C.byref(scale), counts, _p(inl, C.c_uint8))
    return np.float32(rmse.value), np.float32(scale.value), tuple(counts), inl.astype(bool), rc


def stereo_from_tracks(cam, bf, left_xy, right_xy, track_status, lib=None):
    """nrs_stereo_from_tracks (host only) -> (xyz [n,3], status [n])"""
    lib = lib or load_library()
    l, r, st = _f32(left_xy).reshape(-1, 2), _f32(right_xy).reshape(-1, 2), _i32(track_status)
    n = len(l)
    assert len(r) == n and len(st) == n
    xyz, status = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
    rc = lib.nrs_stereo_from_tracks(C.byref(cam), C.c_float(bf), C.c_int32(n), _p(l, C.c_float), _p(r, C.c_float), _p(st, C.c_int32),
                                    _p(xyz, C.c_float), _p(status, C.c_int32))
    if rc != OK:
        raise NrsError(rc, "nrs_stereo_from_tracks")
    return xyz, status


def stereo_lk(ctx_stereo, cam, bf, left, right, xy, min_ssim=0.5):
    """StereoLucasKanade::ComputeStereo3D (stereo_lucas_kanade.cc:38-75): SetReferenceImage(left), Track(right, initial flow, min_ssim) and
    the disparity step.  ctx_stereo is a context kept for stereo (configured with klt_configure): these calls replace its tracker's
    reference, so it must not be the context that holds the tracking templates.  -> (xyz, status, right_xy, track_status)"""
    xy = _f32(xy).reshape(-1, 2)
    ctx_stereo.klt_set_reference(left, xy)
    rxy, st, _, _ = ctx_stereo.klt_track(right, xy, np.full(len(xy), 1, np.int32), initial_flow=True, min_ssim=min_ssim)
    xyz, status = stereo_from_tracks(cam, bf, xy, rxy, st, ctx_stereo.lib)
    return xyz, status, rxy, st


def stereo_lk_front(ctx_stereo, ctx_front, cam, bf, xy, min_ssim=0.5, image=FRONT_GRAY, shape=None):
    """nrs_stereo_match_lk_front: stereo_lk on the resident pair ctx_front holds after front_process_stereo, in the tracker state of
    ctx_stereo (a context kept for stereo, on the same device).  The two may be the same context: the call then REPLACES its tracking
    templates, as stereo_lk replaces those of its ctx_stereo.  -> (xyz, status, right_xy, track_status)"""
    hh, ww = shape or ctx_front._front_shape
    xy = _f32(xy).reshape(-1, 2)
    n = len(xy)
    xyz, status = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
    rxy, st = np.zeros((n, 2), np.float32), np.zeros(n, np.int32)
    ctx_stereo._chk(ctx_stereo.lib.nrs_stereo_match_lk_front(ctx_stereo.h, ctx_front.h, C.byref(cam), bf, ww, hh, int(image), n, _p(xy, C.c_float),
                                                             min_ssim, _p(xyz, C.c_float), _p(status, C.c_int32), _p(rxy, C.c_float), _p(st, C.c_int32)))
    return xyz, status, rxy, st


class LocalGroup:
    """Test harness: `world` ranks as threads of this process, contexts on the same GPU (include/nrs.h)."""
    def __init__(self, world, lib=None):
        self.lib = lib or load_library()
        self.world = world
        self.h = C.c_void_p()
        rc = self.lib.nrs_local_group_create(C.c_int32(world), C.byref(self.h))
        if rc != OK:
            raise NrsError(rc, "nrs_local_group_create")

    def close(self):
        if self.h:
            self.lib.nrs_local_group_destroy(self.h)
            self.h = C.c_void_p()


def _p(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


def make_camera(model, params):
    cam = Camera()
    cam.model = int(model)
    prm = np.zeros(8, np.float32)
    prm[:len(params)] = np.asarray(params, np.float32)
    for i in range(8):
        cam.params[i] = float(prm[i])
    return cam


class GraphArrays:
    """Owns contiguous copies of a flat graph dict (nrs_synth.build_graph) and the nrs_graph view."""

    def __init__(self, g):
        self.rowptr, self.col, self.eid = _i32(g["rowptr"]).copy(), _i32(g["col"]).copy(), _i32(g["eid"]).copy()
        self.e_w, self.e_d0 = _f32(g["e_w"]).copy(), _f32(g["e_d0"]).copy()
        self.e_max, self.e_min = _f32(g["e_max"]).copy(), _f32(g["e_min"]).copy()
        self.e_status = _i32(g["e_status"]).copy()
        self.c = Graph(len(self.rowptr) - 1, _p(self.rowptr, C.c_int32), _p(self.col, C.c_int32),
                       _p(self.eid, C.c_int32), len(self.e_w), _p(self.e_w, C.c_float), _p(self.e_d0, C.c_float),
                       _p(self.e_max, C.c_float), _p(self.e_min, C.c_float), _p(self.e_status, C.c_int32),
                       float(g["sigma"]), float(g["stretch_th"]))

    def as_dict(self, g):
        out = dict(g)
        out.update(e_w=self.e_w.copy(), e_max=self.e_max.copy(), e_min=self.e_min.copy(), e_status=self.e_status.copy())
        return out


class Trace:
    def __init__(self, capacity=512):
        self.buf = (LmTrial * capacity)()
        self.c = LmTrace(C.cast(self.buf, C.POINTER(LmTrial)), capacity, 0, 0)

    @property
    def trials(self):
        n = min(self.c.count, self.c.capacity)
        return [dict(round=t.round, iter=t.iter, trial=t.trial, accepted=bool(t.accepted),
                     ok=bool(t.solver_ok), inner=t.inner_iters, early=bool(t.early_rejected), lam=t.lam, chi=t.chi2,
                     chi_new=t.chi2_new, rho=t.rho) for t in self.buf[:n]]

    @property
    def iterations(self):
        return self.c.iterations


def dba_build_edges(kf_points, graph, lib=None):
    """Host-side (no GPU) edge construction, reference g2o_optimization.cc:927-1137."""
    lib = lib or load_library()
    n_kf = len(kf_points)
    kf_rowptr = np.zeros(n_kf + 1, np.int32)
    kf_rowptr[1:] = np.cumsum([len(k) for k in kf_points])
    kf_pt = _i32(np.concatenate(kf_points)) if n_kf else np.zeros(0, np.int32)
    n_points = len(graph["rowptr"]) - 1
    rp, col, w, d0, st = (_i32(graph["rowptr"]), _i32(graph["col"]), _f32(graph["w"]),
                          _f32(graph["d0"]), _i32(graph["status"]))
    ns, nd = C.c_int32(0), C.c_int32(0)
    args = [C.c_int32(n_kf), _p(kf_rowptr, C.c_int32), _p(kf_pt, C.c_int32), C.c_int32(n_points),
            _p(rp, C.c_int32), _p(col, C.c_int32), _p(w, C.c_float), _p(d0, C.c_float), _p(st, C.c_int32)]
    rc = lib.nrs_dba_build_edges(*args, C.byref(ns), None, None, C.byref(nd), None, None)
    if rc != OK:
        raise NrsError(rc, "nrs_dba_build_edges (count)")
    sp_ij = np.zeros((ns.value, 2), np.int32)
    sp_d0 = np.zeros(ns.value, np.float32)
    dm_idx = np.zeros((nd.value, 4), np.int32)
    dm_w = np.zeros(nd.value, np.float32)
    rc = lib.nrs_dba_build_edges(*args, C.byref(ns), _p(sp_ij, C.c_int32), _p(sp_d0, C.c_float),
                                 C.byref(nd), _p(dm_idx, C.c_int32), _p(dm_w, C.c_float))
    if rc != OK:
        raise NrsError(rc, "nrs_dba_build_edges (fill)")
    return dict(sp_ij=sp_ij, sp_d0=sp_d0, dm_idx=dm_idx, dm_w=dm_w)


def dba_build_edges_embedded(kf_points, is_node, graph, lib=None):
    """Host-side edge construction of the EMBEDDED window (include/nrs.h nrs_dba_build_edges_embedded, N2b): node copies, springs /
    dampers between them, skinned observations with their node copies and normalised weights."""
    lib = lib or load_library()
    n_kf = len(kf_points)
    kf_rowptr = np.zeros(n_kf + 1, np.int32)
    kf_rowptr[1:] = np.cumsum([len(k) for k in kf_points])
    kf_pt = _i32(np.concatenate(kf_points)) if n_kf else np.zeros(0, np.int32)
    n_points = len(graph["rowptr"]) - 1
    node = np.ascontiguousarray(is_node, np.uint8)
    assert len(node) == n_points
    rp, col, w, d0, st = (_i32(graph["rowptr"]), _i32(graph["col"]), _f32(graph["w"]), _f32(graph["d0"]), _i32(graph["status"]))
    nl, ns, nd, nk = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    args = [C.c_int32(n_kf), _p(kf_rowptr, C.c_int32), _p(kf_pt, C.c_int32), C.c_int32(n_points), _p(node, C.c_uint8),
            _p(rp, C.c_int32), _p(col, C.c_int32), _p(w, C.c_float), _p(d0, C.c_float), _p(st, C.c_int32)]
    rc = lib.nrs_dba_build_edges_embedded(*args, C.byref(nl), None, C.byref(ns), None, None, C.byref(nd), None, None, C.byref(nk), None, None, None)
    if rc != OK:
        raise NrsError(rc, "nrs_dba_build_edges_embedded (count)")
    lm_obs = np.zeros(nl.value, np.int32)
    sp_ij, sp_d0 = np.zeros((ns.value, 2), np.int32), np.zeros(ns.value, np.float32)
    dm_idx, dm_w = np.zeros((nd.value, 4), np.int32), np.zeros(nd.value, np.float32)
    sk_obs, sk_node, sk_omega = np.zeros(nk.value, np.int32), np.zeros((nk.value, 11), np.int32), np.zeros((nk.value, 11), np.float64)
    rc = lib.nrs_dba_build_edges_embedded(*args, C.byref(nl), _p(lm_obs, C.c_int32), C.byref(ns), _p(sp_ij, C.c_int32), _p(sp_d0, C.c_float),
                                          C.byref(nd), _p(dm_idx, C.c_int32), _p(dm_w, C.c_float), C.byref(nk), _p(sk_obs, C.c_int32),
                                          _p(sk_node, C.c_int32), _p(sk_omega, C.c_double))
    if rc != OK:
        raise NrsError(rc, "nrs_dba_build_edges_embedded (fill)")
    return dict(lm_obs=lm_obs, sp_ij=sp_ij, sp_d0=sp_d0, dm_idx=dm_idx, dm_w=dm_w, sk_obs=sk_obs, sk_node=sk_node, sk_omega=sk_omega)


class RGraph:
    """nrs_rgraph_* (include/nrs.h): the dense, device-resident RegularizationGraph of a context"""

    def __init__(self, ctx, capacity, sigma, stretch_th=1.1):
        self.ctx, self.lib, self.cap = ctx, ctx.lib, capacity
        self.h = C.c_void_p()
        ctx._chk(self.lib.nrs_rgraph_create(ctx.h, C.c_int32(capacity), C.c_float(sigma), C.c_float(stretch_th), C.byref(self.h)))

    def close(self):
        if self.h:
            self.lib.nrs_rgraph_destroy(self.h)
            self.h = C.c_void_p()

    def _pos(self, pos):
        pos = _f32(pos).reshape(-1, 3)
        assert len(pos) == self.cap
        return pos

    def set_sigma(self, sigma):
        self.ctx._chk(self.lib.nrs_rgraph_set_sigma(self.h, C.c_float(sigma)))

    def min_weight(self):
        return float(self.lib.nrs_rgraph_min_weight(self.h))

    def add_edges(self, pos, new_ids, other_ids):
        pos, a, b = self._pos(pos), _i32(new_ids), _i32(other_ids)
        self.ctx._chk(self.lib.nrs_rgraph_add_edges(self.h, _p(pos, C.c_float), C.c_int32(len(a)), _p(a, C.c_int32), C.c_int32(len(b)), _p(b, C.c_int32)))

    def update(self, pos, ids):
        pos, ids = self._pos(pos), _i32(ids)
        good = np.zeros(len(ids), np.int32)
        self.ctx._chk(self.lib.nrs_rgraph_update(self.h, _p(pos, C.c_float), C.c_int32(len(ids)), _p(ids, C.c_int32), _p(good, C.c_int32)))
        return good

    def get_edges(self, ids, cap_per_point=256):
        ids = _i32(ids)
        n = len(ids)
        cnt = np.zeros(n, np.int32)
        col, st = np.zeros((n, cap_per_point), np.int32), np.zeros((n, cap_per_point), np.int32)
        w, d0 = np.zeros((n, cap_per_point), np.float32), np.zeros((n, cap_per_point), np.float32)
        self.ctx._chk(self.lib.nrs_rgraph_get_edges(self.h, C.c_int32(n), _p(ids, C.c_int32), C.c_int32(cap_per_point), _p(cnt, C.c_int32),
                                                    _p(col, C.c_int32), _p(w, C.c_float), _p(d0, C.c_float), _p(st, C.c_int32)))
        return cnt, col, w, d0, st

    def edge(self, i, j):
        out = (C.c_float * 4)()
        st = C.c_int32(0)
        self.ctx._chk(self.lib.nrs_rgraph_edge(self.h, C.c_int32(i), C.c_int32(j), out, C.byref(st)))
        return dict(w=out[0], d0=out[1], max=out[2], min=out[3], status=st.value)

    def resize(self, new_capacity):
        """nrs_rgraph_resize: grows the graph (old edges kept, new cells "no edge"); positions passed afterwards have new_capacity rows"""
        self.ctx._chk(self.lib.nrs_rgraph_resize(self.h, C.c_int32(new_capacity)))
        self.cap = int(new_capacity)

    def grow(self, pos, new_ids, other_ids):
        """nrs_map_grow_graph (mapping.cc:238-256): every new landmark against every map point the frame holds with a position"""
        pos, a, b = self._pos(pos), _i32(new_ids), _i32(other_ids)
        self.ctx._chk(self.lib.nrs_map_grow_graph(self.ctx.h, self.h, _p(pos, C.c_float), C.c_int32(len(a)), _p(a, C.c_int32), C.c_int32(len(b)), _p(b, C.c_int32)))

    def rows(self, ids):
        ids = _i32(ids)
        n = len(ids)
        mx, mn, d0 = (np.zeros((n, self.cap), np.float32) for _ in range(3))
        st = np.zeros((n, self.cap), np.uint8)
        self.ctx._chk(self.lib.nrs_rgraph_rows(self.h, C.c_int32(n), _p(ids, C.c_int32), _p(mx, C.c_float), _p(mn, C.c_float), _p(d0, C.c_float),
                                               _p(st, C.c_uint8)))
        return mx, mn, d0, st


class TBuf:
    """nrs_tbuf_* (include/nrs.h): the device-resident TemporalBuffer of a context"""

    def __init__(self, ctx, max_buffer_size=20):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        ctx._chk(self.lib.nrs_tbuf_create(ctx.h, max_buffer_size, C.byref(self.h)))

    def close(self):
        if self.h:
            self.lib.nrs_tbuf_destroy(self.h)
            self.h = C.c_void_p()

    def clear(self):
        self.ctx._chk(self.lib.nrs_tbuf_clear(self.h))

    def insert(self, kp_id, kp_xy, lm_xyz, status, pose_qt, deform_mag, has_lm=None):
        """InsertSnapshotFromFrame: the frame's slots unfiltered (the call keeps TRACKED_WITH_3D / TRACKED).  Ids must fit an int32."""
        ids64 = np.asarray(kp_id, np.int64).reshape(-1)
        n = len(ids64)
        if n and (ids64.max() > 2**31 - 1 or ids64.min() < -2**31):
            raise ValueError("TBuf.insert: a keypoint id does not fit 32 bits")
        ids, xy, xyz, st = _i32(ids64), _f32(kp_xy).reshape(-1, 2), _f32(lm_xyz).reshape(-1, 3), _i32(status).reshape(-1)
        if len(xy) != n or len(xyz) != n or len(st) != n:
            raise ValueError("TBuf.insert: kp_id, kp_xy, lm_xyz and status differ in length")
        hl = None if has_lm is None else np.ascontiguousarray(has_lm, np.uint8).reshape(-1)
        if hl is not None and len(hl) != n:
            raise ValueError("TBuf.insert: has_lm needs one flag per slot")
        pose = _f32(pose_qt).reshape(7)
        self.ctx._chk(self.lib.nrs_tbuf_insert(self.h, n, _p(ids, C.c_int32), _p(xy, C.c_float), _p(xyz, C.c_float), _p(st, C.c_int32),
                                               _p(hl, C.c_uint8), _p(pose, C.c_float), float(deform_mag)))

    def info(self):
        """-> (snapshots held, distinct keypoint ids, triangulation candidates)"""
        f, n, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self.ctx._chk(self.lib.nrs_tbuf_info(self.h, C.byref(f), C.byref(n), C.byref(c)))
        return f.value, n.value, c.value

    def flat(self):
        """nrs_tbuf_flat -> (tb, deform_mag, ids) as nrs_frame_loop.TemporalBuffer.flat returns them (without model / prm)"""
        F, n, _ = self.info()
        ids, st = np.zeros(n, np.int32), np.zeros(n, np.int32)
        has_kp, has_lm = np.zeros((F, n), np.uint8), np.zeros((F, n), np.uint8)
        kp, lm = np.zeros((F, n, 2), np.float32), np.zeros((F, n, 3), np.float32)
        poses, mag = np.zeros((F, 7), np.float32), np.zeros(F, np.float32)
        self.ctx._chk(self.lib.nrs_tbuf_flat(self.h, _p(ids, C.c_int32), _p(has_kp, C.c_uint8), _p(kp, C.c_float), _p(has_lm, C.c_uint8),
                                             _p(lm, C.c_float), _p(st, C.c_int32), _p(poses, C.c_float), _p(mag, C.c_float)))
        tb = dict(n_frames=F, poses=poses, has_kp=has_kp.astype(bool), kp_xy=kp, has_lm=has_lm.astype(bool), lm_xyz=lm, status=st)
        return tb, mag, ids

    def map_frame(self, cam, rad_per_pixel, rigidity_th=0.004, min_track=5, index_snapshot=-1, ctx=None):
        """nrs_map_frame_tbuf: Context.map_frame's dict, with `cand` and `accepted_ids` as KEYPOINT IDS.  ctx: the context to call on
        (the buffer's own; another one is refused)"""
        ctx = ctx or self.ctx
        m = max(1, self.info()[2])
        cand, r_st, d_st, a_id = (np.zeros(m, np.int32) for _ in range(4))
        r_xyz, d_xyz, a_xyz = (np.zeros((m, 3), np.float32) for _ in range(3))
        counts = np.zeros(3, np.int32)
        nc, na = C.c_int32(0), C.c_int32(0)
        ctx._chk(self.lib.nrs_map_frame_tbuf(ctx.h, C.byref(cam), self.h, rad_per_pixel, rigidity_th, min_track, index_snapshot,
                                             C.byref(nc), _p(cand, C.c_int32), _p(r_st, C.c_int32), _p(r_xyz, C.c_float), _p(d_st, C.c_int32),
                                             _p(d_xyz, C.c_float), _p(counts, C.c_int32), C.byref(na), _p(a_id, C.c_int32), _p(a_xyz, C.c_float)))
        nc, na = nc.value, na.value
        return dict(cand=cand[:nc], rigid_status=r_st[:nc], rigid_xyz=r_xyz[:nc], deform_status=d_st[:nc], deform_xyz=d_xyz[:nc],
                    n_rigid=int(counts[0]), n_deformable=int(counts[1]), mode=int(counts[2]), accepted_ids=a_id[:na], accepted_xyz=a_xyz[:na])


class Context:
    def __init__(self, device=-1, pcg_rtol=0.0, pcg_max_iters=0, pcg_batch=0, profile=0, exact_trials=0, direct_solve=0, embedded_solver=0,
                 sharded_kft=0):
        self.lib = load_library()
        opt = Options(device, C.sizeof(Options), pcg_rtol, pcg_max_iters, pcg_batch, profile, exact_trials, direct_solve, embedded_solver,
                      sharded_kft)
        self.h = C.c_void_p()
        rc = self.lib.nrs_create(C.byref(self.h), C.byref(opt))
        if rc != OK:
            raise NrsError(rc, "nrs_create failed (no usable HIP device?)")
        _LIVE.add(self)
        for k, v in _DEBUG.items():
            self.debug_set(k, v)

    def close(self):
        if self.h:
            self.lib.nrs_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != OK:
            raise NrsError(rc, self.lib.nrs_last_error(self.h).decode())

    # ---- f3: Shi-Tomasi extraction
    def shi_configure(self, nms_window=5):
        self._chk(self.lib.nrs_shi_configure(self.h, C.c_int32(nms_window)))

    def shi_extract(self, img, prev_xy=None, mask=None, capacity=65536):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        prev = None if prev_xy is None or len(prev_xy) == 0 else _f32(np.asarray(prev_xy).reshape(-1, 2))
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        xy = np.zeros((capacity, 2), np.float32)
        ids = np.zeros(capacity, np.int32)
        n = C.c_int32(0)
        self._chk(self.lib.nrs_shi_extract(self.h, _p(img, C.c_uint8), C.c_int32(w), C.c_int32(h), C.c_int32(w),
                                           _p(m, C.c_uint8), C.c_int32(w), C.c_int32(0 if prev is None else len(prev)),
                                           _p(prev, C.c_float), C.c_int32(capacity), _p(xy, C.c_float), _p(ids, C.c_int32),
                                           C.byref(n)))
        self._shi_shape = (h, w)
        k = min(n.value, capacity)
        return xy[:k].copy(), ids[:k].copy(), n.value

    def shi_buffers(self):
        h, w = self._shi_shape
        sc = np.zeros((h, w), np.float32)
        xg = np.zeros((h, w), np.int16)
        yg = np.zeros((h, w), np.int16)
        self._chk(self.lib.nrs_shi_buffers(self.h, _p(sc, C.c_float), _p(xg, C.c_int16), _p(yg, C.c_int16)))
        return sc, xg, yg

    # ---- f5: the image front end (grey, CLAHE, the Masker's masks) and the resident hand-over to the tracker / the extractor
    def front_configure(self, filters=(), clahe_clip=3.0, tiles=(8, 8)):
        """filters: ("bright", th) / ("border", rb, re, cb, ce[, th]) / ("predefined", mask h x w uint8), in the order of filters.txt"""
        recs = (FrontFilter * max(len(filters), 1))()
        keep = []
        for r, f in zip(recs, filters):
            kind = f[0].lower()
            if kind == "bright":
                r.kind, r.p[0] = FRONT_BRIGHT, int(f[1])
            elif kind == "border":
                r.kind = FRONT_BORDER
                for j, v in enumerate(f[1:6]):
                    r.p[j] = int(v)
            elif kind == "predefined":
                m = np.ascontiguousarray(f[1], np.uint8)
                keep.append(m)
                r.kind, r.mask, r.w, r.h, r.stride = FRONT_PREDEFINED, m.ctypes.data, m.shape[1], m.shape[0], m.strides[0]
            else:
                raise ValueError("unknown filter %r" % (f[0],))
        self._chk(self.lib.nrs_front_configure(self.h, C.c_int32(len(filters)), recs if len(filters) else None, C.c_float(clahe_clip),
                                               C.c_int32(tiles[0]), C.c_int32(tiles[1])))
        self._front_n = len(filters)

    def front_process(self, img, outputs=True, stride=None, width=None, channels=1):
        """img: h x w (grey) or h x w x 3 / 4 uint8; rows may be padded (give `stride` in bytes, `width` in pixels and `channels`, img then being the raw
        h x stride byte array).  outputs: True (everything), False (nothing is downloaded: the results stay resident) or the names wanted of
        "gray", "clahe", "global", "masks".  -> dict of those"""
        img = np.asarray(img, np.uint8)
        if stride is None:
            img = np.ascontiguousarray(img)
            hh, ww = img.shape[:2]
            ch = 1 if img.ndim == 2 else img.shape[2]
            stride = img.strides[0] if hh else ww * ch
        else:
            hh, ww, ch = img.shape[0], int(width), int(channels)
        nf = getattr(self, "_front_n", 0)
        self._front_shape = (hh, ww)
        want = ("gray", "clahe", "global", "masks") if outputs is True else tuple(outputs or ())
        out = {k: np.zeros((hh, ww), np.uint8) for k in ("gray", "clahe", "global") if k in want}
        ptrs = None
        if "masks" in want:
            out["masks"] = [np.zeros((hh, ww), np.uint8) for _ in range(nf)]
            if nf:
                ptrs = (C.c_void_p * nf)(*[m.ctypes.data for m in out["masks"]])
        self._chk(self.lib.nrs_front_process(self.h, C.c_void_p(img.ctypes.data), C.c_int32(ww), C.c_int32(hh), C.c_int32(stride), C.c_int32(ch),
                                             _p(out.get("gray"), C.c_uint8), _p(out.get("clahe"), C.c_uint8), _p(out.get("global"), C.c_uint8), ptrs))
        return out

    def front_process_stereo(self, left, right, outputs=True, stride_l=None, stride_r=None, width=None, channels=1):
        """nrs_front_process_stereo: both eyes of a stereo pair in one call (the left one as front_process, the right one grey + CLAHE).  left /
        right: h x w or h x w x 3 / 4 uint8 of the same shape -- or, with stride_l / stride_r (bytes), width and channels, the raw h x stride byte
        arrays.  outputs: True, False or the names wanted of "gray", "clahe", "global", "masks", "gray_right", "clahe_right".  -> dict of those.
        The C entry point takes ONE w, h and channel count, so two arrays that differ in size or channel count cannot reach it: THIS BINDING
        refuses them, raising NrsError with NRS_ERR_INVALID before the library is called.  A right image of None goes to the library as NULL
        and is refused there."""
        left = np.asarray(left, np.uint8)
        none_right = right is None                                  # (handed to the library as NULL: it refuses)
        right = left if none_right else np.asarray(right, np.uint8)
        if (stride_l is None) != (stride_r is None):
            raise ValueError("front_process_stereo: give both strides or neither")
        if stride_l is None:
            left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
            if left.shape != right.shape:
                raise NrsError(-1, "front_process_stereo: the eyes differ in size or channel count: %s and %s" % (left.shape, right.shape))
            hh, ww = left.shape[:2]
            ch = 1 if left.ndim == 2 else left.shape[2]
            stride_l = stride_r = left.strides[0] if hh else ww * ch
        else:
            if left.shape[0] != right.shape[0]:
                raise NrsError(-1, "front_process_stereo: the eyes differ in height: %d and %d" % (left.shape[0], right.shape[0]))
            hh, ww, ch = left.shape[0], int(width), int(channels)
        nf = getattr(self, "_front_n", 0)
        names = ("gray", "clahe", "global", "gray_right", "clahe_right")
        want = names + ("masks",) if outputs is True else tuple(outputs or ())
        out = {k: np.zeros((hh, ww), np.uint8) for k in names if k in want}
        ptrs = None
        if "masks" in want:
            out["masks"] = [np.zeros((hh, ww), np.uint8) for _ in range(nf)]
            if nf:
                ptrs = (C.c_void_p * nf)(*[m.ctypes.data for m in out["masks"]])
        self._chk(self.lib.nrs_front_process_stereo(self.h, left.ctypes.data, None if none_right else right.ctypes.data, ww, hh, int(stride_l), int(stride_r), ch,
                                                    _p(out.get("gray"), C.c_uint8), _p(out.get("clahe"), C.c_uint8), _p(out.get("global"), C.c_uint8),
                                                    ptrs, _p(out.get("gray_right"), C.c_uint8), _p(out.get("clahe_right"), C.c_uint8)))
        self._front_shape = (hh, ww)                                # (after the call: a refused pair leaves the resident size as it was)
        return out

    # ---- stereo rectification: the maps once, then raw pairs into the resident pair
    def front_rectify_configure(self, src_wh, dst_wh, left, right):
        """nrs_front_rectify_configure: src_wh / dst_wh = (w, h) of a raw / a rectified eye; left / right: eye records (make_rect_eye)"""
        l, r = make_rect_eye(left), make_rect_eye(right)
        self._chk(self.lib.nrs_front_rectify_configure(self.h, int(src_wh[0]), int(src_wh[1]), int(dst_wh[0]), int(dst_wh[1]),
                                                       None if l is None else C.addressof(l), None if r is None else C.addressof(r)))
        self._rect_src, self._rect_dst = (int(src_wh[0]), int(src_wh[1])), (int(dst_wh[0]), int(dst_wh[1]))

    def front_rectify_maps(self, eye, shape=None):
        """nrs_front_rectify_maps -> (map_x, map_y), dst_h x dst_w float32, of eye 0 (left) or 1 (right)"""
        ww, hh = (shape[1], shape[0]) if shape else getattr(self, "_rect_dst", (1, 1))      # (never configured: the library refuses)
        mx, my = np.zeros((hh, ww), np.float32), np.zeros((hh, ww), np.float32)
        self._chk(self.lib.nrs_front_rectify_maps(self.h, int(eye), _p(mx, C.c_float), _p(my, C.c_float)))
        return mx, my

    def front_process_stereo_raw(self, left, right, outputs=True, stride_l=None, stride_r=None, width=None, channels=1):
        """nrs_front_process_stereo_raw: the RAW eyes of a pair, rectified on the device by the maps of front_rectify_configure, then as
        front_process_stereo.  The arguments are those of front_process_stereo, at the raw size; outputs: True, False or the names wanted of
        "gray", "clahe", "global", "masks", "gray_right", "clahe_right", "rect_left", "rect_right" (the rectified images, dst_h x dst_w or
        dst_h x dst_w x channels).  -> dict of those, all of the rectified size"""
        left = np.asarray(left, np.uint8)
        none_right = right is None
        right = left if none_right else np.asarray(right, np.uint8)
        if (stride_l is None) != (stride_r is None):
            raise ValueError("front_process_stereo_raw: give both strides or neither")
        if stride_l is None:
            left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
            if left.shape != right.shape:
                raise NrsError(-1, "front_process_stereo_raw: the eyes differ in size or channel count: %s and %s" % (left.shape, right.shape))
            hh, ww = left.shape[:2]
            ch = 1 if left.ndim == 2 else left.shape[2]
            stride_l = stride_r = left.strides[0] if hh else ww * ch
        else:
            if left.shape[0] != right.shape[0]:
                raise NrsError(-1, "front_process_stereo_raw: the eyes differ in height: %d and %d" % (left.shape[0], right.shape[0]))
            hh, ww, ch = left.shape[0], int(width), int(channels)
        dw, dh = getattr(self, "_rect_dst", (ww, hh))                # (never configured: the library refuses)
        nf = getattr(self, "_front_n", 0)
        names = ("gray", "clahe", "global", "gray_right", "clahe_right")
        want = names + ("masks", "rect_left", "rect_right") if outputs is True else tuple(outputs or ())
        out = {k: np.zeros((dh, dw), np.uint8) for k in names if k in want}
        for k in ("rect_left", "rect_right"):
            if k in want:
                out[k] = np.zeros((dh, dw) if ch == 1 else (dh, dw, ch), np.uint8)
        ptrs = None
        if "masks" in want:
            out["masks"] = [np.zeros((dh, dw), np.uint8) for _ in range(nf)]
            if nf:
                ptrs = (C.c_void_p * nf)(*[m.ctypes.data for m in out["masks"]])
        self._chk(self.lib.nrs_front_process_stereo_raw(self.h, left.ctypes.data, None if none_right else right.ctypes.data, ww, hh, int(stride_l), int(stride_r),
                                                        ch, _p(out.get("gray"), C.c_uint8), _p(out.get("clahe"), C.c_uint8), _p(out.get("global"), C.c_uint8),
                                                        ptrs, _p(out.get("gray_right"), C.c_uint8), _p(out.get("clahe_right"), C.c_uint8),
                                                        _p(out.get("rect_left"), C.c_uint8), _p(out.get("rect_right"), C.c_uint8)))
        self._front_shape = (dh, dw)
        return out

    # ---- frame resize: the tables once, then raw frames into the resident frame
    def front_resize_configure(self, src_wh, dst_wh):
        """nrs_front_resize_configure: src_wh / dst_wh = (w, h) of a raw / a resized frame (half_size gives the Endomapper app's)"""
        self._chk(self.lib.nrs_front_resize_configure(self.h, int(src_wh[0]), int(src_wh[1]), int(dst_wh[0]), int(dst_wh[1])))
        self._resize_src, self._resize_dst = (int(src_wh[0]), int(src_wh[1])), (int(dst_wh[0]), int(dst_wh[1]))

    def front_resize_taps(self):
        """nrs_front_resize_taps -> dict(sx int32 [dst_w], ax int16 [dst_w, 2], sy int32 [dst_h, 2], by int16 [dst_h, 2], box 0 / 1)"""
        dw, dh = getattr(self, "_resize_dst", (1, 1))                # (never configured: the library refuses)
        out = dict(sx=np.zeros(dw, np.int32), ax=np.zeros((dw, 2), np.int16), sy=np.zeros((dh, 2), np.int32), by=np.zeros((dh, 2), np.int16))
        box = C.c_int32(-1)
        self._chk(self.lib.nrs_front_resize_taps(self.h, out["sx"].ctypes.data, out["ax"].ctypes.data, out["sy"].ctypes.data, out["by"].ctypes.data,
                                                 C.addressof(box)))
        out["box"] = int(box.value)
        return out

    def front_process_raw(self, img, outputs=True, stride=None, width=None, channels=1):
        """nrs_front_process_raw: the RAW frame, resized on the device by the tables of front_resize_configure, then as front_process.  The
        arguments are those of front_process, at the raw size; outputs: True, False or the names wanted of "gray", "clahe", "global", "masks",
        "resized" (the resized frame, dst_h x dst_w or dst_h x dst_w x channels).  -> dict of those, all of the resized size"""
        img = np.asarray(img, np.uint8)
        if stride is None:
            img = np.ascontiguousarray(img)
            hh, ww = img.shape[:2]
            ch = 1 if img.ndim == 2 else img.shape[2]
            stride = img.strides[0] if hh else ww * ch
        else:
            hh, ww, ch = img.shape[0], int(width), int(channels)
        dw, dh = getattr(self, "_resize_dst", (ww, hh))              # (never configured: the library refuses)
        nf = getattr(self, "_front_n", 0)
        want = ("gray", "clahe", "global", "masks", "resized") if outputs is True else tuple(outputs or ())
        out = {k: np.zeros((dh, dw), np.uint8) for k in ("gray", "clahe", "global") if k in want}
        if "resized" in want:
            out["resized"] = np.zeros((dh, dw) if ch == 1 else (dh, dw, ch), np.uint8)
        ptrs = None
        if "masks" in want:
            out["masks"] = [np.zeros((dh, dw), np.uint8) for _ in range(nf)]
            if nf:
                ptrs = (C.c_void_p * nf)(*[m.ctypes.data for m in out["masks"]])
        self._chk(self.lib.nrs_front_process_raw(self.h, img.ctypes.data, ww, hh, int(stride), ch, _p(out.get("gray"), C.c_uint8),
                                                 _p(out.get("clahe"), C.c_uint8), _p(out.get("global"), C.c_uint8), ptrs,
                                                 _p(out.get("resized"), C.c_uint8)))
        self._front_shape = (dh, dw)                                 # (after the call: a refused frame leaves the resident size as it was)
        return out

    def klt_set_reference_front(self, xy, image=FRONT_GRAY, use_global_mask=True, shape=None):
        hh, ww = shape or self._front_shape
        xy = _f32(xy).reshape(-1, 2)
        self._chk(self.lib.nrs_klt_set_reference_front(self.h, C.c_int32(ww), C.c_int32(hh), C.c_int32(image), C.c_int32(1 if use_global_mask else 0),
                                                       C.c_int32(len(xy)), _p(xy, C.c_float)))

    def klt_track_front(self, xy, status, image=FRONT_GRAY, initial_flow=True, min_ssim=0.7, shape=None):
        hh, ww = shape or self._front_shape
        xy = _f32(xy).reshape(-1, 2).copy()
        st = _i32(status).copy()
        good = C.c_int32(0)
        ssim = np.full(len(xy), np.nan, np.float32)
        self._chk(self.lib.nrs_klt_track_front(self.h, C.c_int32(ww), C.c_int32(hh), C.c_int32(image), C.c_int32(len(xy)), _p(xy, C.c_float),
                                               _p(st, C.c_int32), C.c_int32(1 if initial_flow else 0), C.c_float(min_ssim), C.byref(good),
                                               _p(ssim, C.c_float)))
        return xy, st, good.value, ssim

    def shi_extract_front(self, prev_xy=None, image=FRONT_GRAY, use_global_mask=True, capacity=65536, shape=None):
        hh, ww = shape or self._front_shape
        prev = None if prev_xy is None or len(prev_xy) == 0 else _f32(np.asarray(prev_xy).reshape(-1, 2))
        xy = np.zeros((capacity, 2), np.float32)
        ids = np.zeros(capacity, np.int32)
        n = C.c_int32(0)
        self._chk(self.lib.nrs_shi_extract_front(self.h, C.c_int32(ww), C.c_int32(hh), C.c_int32(image), C.c_int32(1 if use_global_mask else 0),
                                                 C.c_int32(0 if prev is None else len(prev)), _p(prev, C.c_float), C.c_int32(capacity),
                                                 _p(xy, C.c_float), _p(ids, C.c_int32), C.byref(n)))
        self._shi_shape = (hh, ww)
        k = min(n.value, capacity)
        return xy[:k].copy(), ids[:k].copy(), n.value

    def comm_init_rccl(self, world, rank, uid):
        buf = (C.c_uint8 * len(uid)).from_buffer_copy(uid)
        self._chk(self.lib.nrs_comm_init_rccl(self.h, C.c_int32(world), C.c_int32(rank), buf, C.c_int32(len(uid))))

    def comm_init_local(self, group, rank):
        self._chk(self.lib.nrs_comm_init_local(self.h, group.h, C.c_int32(rank)))

    def comm_rank(self):
        r, w = C.c_int32(0), C.c_int32(1)
        self._chk(self.lib.nrs_comm_rank(self.h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def device_name(self):
        buf = C.create_string_buffer(256)
        self._chk(self.lib.nrs_device_name(self.h, buf, 256))
        return buf.value.decode()

    def profile(self):
        p = Profile()
        self._chk(self.lib.nrs_get_profile(self.h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in Profile._fields_}

    def reset_profile(self):
        self._chk(self.lib.nrs_reset_profile(self.h))

    # ---- a1
    def pose_only_solve(self, cam, uv, X, pose_q, pose_t, trace=None):
        uv, X = _f32(uv).reshape(-1, 2), _f32(X).reshape(-1, 3)
        n = len(uv)
        qt = np.concatenate([np.asarray(pose_q, np.float64), np.asarray(pose_t, np.float64)])
        inl = np.zeros(n, np.uint8)
        self._chk(self.lib.nrs_pose_only_solve(self.h, C.byref(cam), C.c_int32(n), _p(uv, C.c_float),
                                               _p(X, C.c_float), _p(qt, C.c_double), _p(inl, C.c_uint8),
                                               C.byref(trace.c) if trace else None))
        return qt[:4].copy(), qt[4:].copy(), inl.astype(bool)

    # ---- f2
    def triangulate_batch(self, cam, tb, cand_ids, min_track=5, debug=False):
        """tb: flat temporal buffer dict (nrs_synth.make_temporal_buffer); returns (status[n], xyz[n,3][, debug[n,4]])"""
        F, n = tb["has_kp"].shape
        poses = _f32(tb["poses"]).reshape(F, 7)
        has_kp, has_lm = np.ascontiguousarray(tb["has_kp"], np.uint8), np.ascontiguousarray(tb["has_lm"], np.uint8)
        kp, lm = _f32(tb["kp_xy"]).reshape(F, n, 2), _f32(tb["lm_xyz"]).reshape(F, n, 3)
        st, cand = _i32(tb["status"]), _i32(cand_ids)
        o_st, o_xyz = np.zeros(len(cand), np.int32), np.zeros((len(cand), 3), np.float32)
        dbg = np.zeros((len(cand), 4), np.float64) if debug else None
        self._chk(self.lib.nrs_triangulate_batch(self.h, C.byref(cam), C.c_int32(F), _p(poses, C.c_float), C.c_int32(n), _p(has_kp, C.c_uint8),
                                                 _p(kp, C.c_float), _p(has_lm, C.c_uint8), _p(lm, C.c_float), _p(st, C.c_int32), C.c_int32(len(cand)),
                                                 _p(cand, C.c_int32), C.c_int32(min_track), _p(o_st, C.c_int32), _p(o_xyz, C.c_float),
                                                 _p(dbg, C.c_double)))
        return (o_st, o_xyz, dbg) if debug else (o_st, o_xyz)

    # ---- frame mapping
    def map_frame(self, cam, tb, deform_mag, rad_per_pixel, rigidity_th=0.004, min_track=5, index_snapshot=-1):
        """Mapping::LandmarkTriangulation in one call (include/nrs.h nrs_map_frame).  tb: flat temporal buffer dict as for
        triangulate_batch.  Returns a dict: cand, rigid_status, rigid_xyz, deform_status, deform_xyz, n_rigid, n_deformable, mode
        (0 none, 1 rigid, 2 deformable), accepted_ids, accepted_xyz."""
        F, n = np.asarray(tb["has_kp"]).shape
        poses = _f32(tb["poses"]).reshape(F, 7)
        has_kp, has_lm = np.ascontiguousarray(tb["has_kp"], np.uint8), np.ascontiguousarray(tb["has_lm"], np.uint8)
        kp, lm = _f32(tb["kp_xy"]).reshape(F, n, 2), _f32(tb["lm_xyz"]).reshape(F, n, 3)
        st, mag = _i32(tb["status"]), _f32(deform_mag)
        if len(mag) != F or len(st) != n:
            raise ValueError("map_frame: deform_mag needs one value per snapshot, status one per id")
        m = max(1, int((st == 1).sum()))
        cand, r_st, d_st, a_id = (np.zeros(m, np.int32) for _ in range(4))
        r_xyz, d_xyz, a_xyz = (np.zeros((m, 3), np.float32) for _ in range(3))
        counts = np.zeros(3, np.int32)
        nc, na = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.nrs_map_frame(self.h, C.byref(cam), C.c_int32(F), _p(poses, C.c_float), C.c_int32(n), _p(has_kp, C.c_uint8),
                                         _p(kp, C.c_float), _p(has_lm, C.c_uint8), _p(lm, C.c_float), _p(st, C.c_int32), _p(mag, C.c_float),
                                         C.c_float(rad_per_pixel), C.c_float(rigidity_th), C.c_int32(min_track), C.c_int32(index_snapshot),
                                         C.byref(nc), _p(cand, C.c_int32), _p(r_st, C.c_int32), _p(r_xyz, C.c_float), _p(d_st, C.c_int32),
                                         _p(d_xyz, C.c_float), _p(counts, C.c_int32), C.byref(na), _p(a_id, C.c_int32), _p(a_xyz, C.c_float)))
        nc, na = nc.value, na.value
        return dict(cand=cand[:nc], rigid_status=r_st[:nc], rigid_xyz=r_xyz[:nc], deform_status=d_st[:nc], deform_xyz=d_xyz[:nc],
                    n_rigid=int(counts[0]), n_deformable=int(counts[1]), mode=int(counts[2]), accepted_ids=a_id[:na], accepted_xyz=a_xyz[:na])

    # ---- f6
    def init_essential(self, cam, ref_xy, cur_xy, status, n_matches, samples=None, taps=True, struct_size=None, **options):
        """EssentialMatrixInitialization::Initialize in one call.  options: the fields of nrs_init_options (defaults from
        nrs_init_options_init); samples: None or n_hypotheses x 8 compact indices.  Returns a dict: verdict, best_hypothesis, score,
        n_compact, counters (dict), E[3,3], pose_q[4], pose_t[3], inlier[n_matches] (bool), xyz[n,3], code[n] and, with taps, hyp_E,
        hyp_score, samples, labels, centres (the last two from the library's sampler only)."""
        ref, cur, st = _f32(ref_xy).reshape(-1, 2), _f32(cur_xy).reshape(-1, 2), _i32(status)
        n = len(st)
        if len(ref) != n or len(cur) != n:
            raise ValueError("init_essential: ref_xy, cur_xy and status differ in length")
        opt = InitOptions()
        self.lib.nrs_init_options_init(C.byref(opt))
        for k, v in options.items():
            if k not in dict(InitOptions._fields_) or k == "struct_size":
                raise TypeError("init_essential: unknown option %r" % k)
            setattr(opt, k, v)
        if struct_size is not None:
            opt.struct_size = struct_size
        nh = opt.n_hypotheses if opt.n_hypotheses > 0 else 16
        nc = int(np.sum(st == 1))
        smp = None
        if samples is not None:
            smp = _i32(np.asarray(samples).reshape(-1))
            if len(smp) != 8 * nh:
                raise ValueError("init_essential: samples must be n_hypotheses x 8")
        out = InitResult()
        out.struct_size = C.sizeof(InitResult)
        a = dict(inlier=np.zeros(max(n_matches, 0), np.uint8), xyz=np.zeros((n, 3), np.float32), code=np.zeros(n, np.int32))
        if taps:
            a.update(hyp_E=np.zeros((nh, 3, 3), np.float32), hyp_score=np.zeros(nh, np.int32), samples_out=np.zeros((nh, 8), np.int32),
                     labels=np.zeros(nc, np.int32), centres=np.zeros((8, 2), np.float32))
        for k, v in a.items():
            setattr(out, k, v.ctypes.data if v.size else None)
        self._chk(self.lib.nrs_init_essential(self.h, C.byref(cam), C.byref(opt), C.c_int32(n), _p(ref, C.c_float), _p(cur, C.c_float),
                                              _p(st, C.c_int32), C.c_int32(n_matches), _p(smp, C.c_int32), C.byref(out)))
        r = dict(verdict=out.verdict, best_hypothesis=out.best_hypothesis, score=out.score, n_compact=out.n_compact,
                 n_hypotheses=out.n_hypotheses, counters=dict(zip(INIT_COUNTERS, list(out.counters))),
                 E=np.array(list(out.E), np.float32).reshape(3, 3), pose_q=np.array(list(out.pose_qt)[:4], np.float32),
                 pose_t=np.array(list(out.pose_qt)[4:], np.float32), inlier=a["inlier"].astype(bool), xyz=a["xyz"], code=a["code"])
        if taps:
            r.update(hyp_E=a["hyp_E"], hyp_score=a["hyp_score"], samples=a["samples_out"])
            if samples is None:
                r.update(labels=a["labels"], centres=a["centres"])
        return r

    # ---- f6: flow-track clustering
    def dbscan_nd(self, data, eps, min_points=FLOW_MIN_POINTS, n=None, dim=None):
        """nrs_dbscan_nd on data [n, dim] fp32 -> (label [n], counts (clusters, noise points)).  n / dim: the values passed to the library
        when they are not data's shape (refusal tests)"""
        data = _f32(data)
        if data.ndim != 2:
            raise ValueError("dbscan_nd: data must be n x dim")
        m, d = data.shape
        lab, counts = np.zeros(m, np.int32), np.zeros(2, np.int32)
        self._chk(self.lib.nrs_dbscan_nd(self.h, m if n is None else n, d if dim is None else dim, data.ctypes.data if data.size else None,
                                         float(eps), int(min_points), lab.ctypes.data if m else None, counts.ctypes.data))
        return lab, counts

    def flow_tracks_cluster(self, tracks_xy, flows=True, n=None, length=None):
        """nrs_flow_tracks_cluster on tracks_xy [n, length, 2] fp32 -> (label [n], counts (clusters, noise points), flows [n, 2 (length - 1)]
        or None).  n / length: the values passed to the library when they are not the array's shape (refusal tests)"""
        t = _f32(tracks_xy)
        if t.ndim != 3 or t.shape[2] != 2:
            raise ValueError("flow_tracks_cluster: tracks_xy must be n x length x 2")
        m, ln = t.shape[0], t.shape[1]
        lab, counts = np.zeros(m, np.int32), np.zeros(2, np.int32)
        fl = np.zeros((m, max(2 * (ln - 1), 0)), np.float32) if flows else None
        self._chk(self.lib.nrs_flow_tracks_cluster(self.h, m if n is None else n, ln if length is None else length, t.ctypes.data if t.size else None,
                                                   fl.ctypes.data if fl is not None and fl.size else None, lab.ctypes.data if m else None,
                                                   counts.ctypes.data))
        return lab, counts, fl

    # ---- f8: stereo map initialisation
    def dbscan3d(self, xyz, eps=2.5, min_points=5, noise_competes=True, n=None):
        """nrs_dbscan3d -> (raw_label [n], label [n], counts (clusters, noise points, size of label 0)).  n: the count passed to the
        library when it is not len(xyz) (refusal tests)"""
        xyz = _f32(xyz).reshape(-1, 3)
        m = len(xyz)
        raw, lab, counts = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(3, np.int32)
        self._chk(self.lib.nrs_dbscan3d(self.h, C.c_int32(m if n is None else n), _p(xyz, C.c_float), C.c_double(eps), C.c_int32(min_points),
                                        C.c_int32(1 if noise_competes else 0), _p(raw, C.c_int32), _p(lab, C.c_int32), _p(counts, C.c_int32)))
        return raw, lab, counts

    def init_stereo(self, cam, left, right, xy, stride_l=None, stride_r=None, width=None, struct_size=None, result_struct_size=None, n=None,
                    **options):
        """Tracking::StereoMapInitialization up to the selected landmarks, in one call.  options: the fields of nrs_init_stereo_options
        (defaults from nrs_init_stereo_options_init).  left / right as in stereo_match_pattern.  Returns a dict: verdict, n_matched,
        n_gated, n_clusters, n_noise, n_selected, median_depth, xyz[n,3], match_status[n], code[n], raw_label[n], label[n],
        selected[n_selected], selected_xyz[n_selected,3]."""
        left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
        h = left.shape[0]
        w = left.shape[1] if width is None else int(width)
        return self._init_stereo(cam, xy, options, struct_size, result_struct_size, n, lambda opt, xy, m, out: self.lib.nrs_init_stereo(
            self.h, C.byref(cam), C.byref(opt), _p(left, C.c_uint8), _p(right, C.c_uint8), C.c_int32(w), C.c_int32(h),
            C.c_int32(stride_l or left.strides[0]), C.c_int32(stride_r or right.strides[0]), C.c_int32(m), _p(xy, C.c_float), C.byref(out)))

    def init_stereo_front(self, cam, xy, image=FRONT_GRAY, shape=None, **options):
        """nrs_init_stereo_front: init_stereo on the resident pair of front_process_stereo (only the keypoints go up); the same dict"""
        hh, ww = shape or self._front_shape
        return self._init_stereo(cam, xy, options, None, None, None, lambda opt, xy, m, out: self.lib.nrs_init_stereo_front(
            self.h, C.byref(cam), C.byref(opt), ww, hh, int(image), m, _p(xy, C.c_float), C.byref(out)))

    def _init_stereo(self, cam, xy, options, struct_size, result_struct_size, n, call):
        xy = _f32(xy).reshape(-1, 2)
        m = len(xy)
        opt = InitStereoOptions()
        self.lib.nrs_init_stereo_options_init(C.byref(opt))
        for k, v in options.items():
            if k not in dict(InitStereoOptions._fields_) or k == "struct_size":
                raise TypeError("init_stereo: unknown option %r" % k)
            setattr(opt, k, v)
        if struct_size is not None:
            opt.struct_size = struct_size
        out = InitStereoResult()
        out.struct_size = C.sizeof(InitStereoResult) if result_struct_size is None else result_struct_size
        a = dict(xyz=np.zeros((m, 3), np.float32), match_status=np.zeros(m, np.int32), code=np.zeros(m, np.int32), raw_label=np.zeros(m, np.int32),
                 label=np.zeros(m, np.int32), selected=np.zeros(m, np.int32), selected_xyz=np.zeros((m, 3), np.float32))
        for k, v in a.items():
            setattr(out, k, v.ctypes.data if v.size else None)
        self._chk(call(opt, xy, m if n is None else n, out))
        ns = out.n_selected
        r = dict(verdict=out.verdict, n_matched=out.n_matched, n_gated=out.n_gated, n_clusters=out.n_clusters, n_noise=out.n_noise,
                 n_selected=ns, median_depth=np.float32(out.median_depth), bf=np.float32(opt.bf))
        r.update(a)
        r["selected"], r["selected_xyz"] = a["selected"][:ns].copy(), a["selected_xyz"][:ns].copy()
        return r

    # ---- f7: evaluation
    def stereo_match_pattern(self, cam, bf, left, right, xy, stride_l=None, stride_r=None, width=None):
        """nrs_stereo_match_pattern -> (xyz [n,3], status [n], score [n] fp64, match_xy [n,2]).  left / right: h x w uint8, or (with width)
        h x stride arrays whose first `width` columns are the image"""
        left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
        h = left.shape[0]
        w = left.shape[1] if width is None else int(width)
        xy = _f32(xy).reshape(-1, 2)
        n = len(xy)
        xyz, status = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        score, match = np.zeros(n, np.float64), np.zeros((n, 2), np.int32)
        self._chk(self.lib.nrs_stereo_match_pattern(self.h, C.byref(cam), C.c_float(bf), _p(left, C.c_uint8), _p(right, C.c_uint8), C.c_int32(w),
                                                    C.c_int32(h), C.c_int32(stride_l or left.strides[0]), C.c_int32(stride_r or right.strides[0]),
                                                    C.c_int32(n), _p(xy, C.c_float), _p(xyz, C.c_float), _p(status, C.c_int32),
                                                    _p(score, C.c_double), _p(match, C.c_int32)))
        return xyz, status, score, match

    def stereo_match_pattern_front(self, cam, bf, xy, image=FRONT_GRAY, shape=None):
        """nrs_stereo_match_pattern_front: stereo_match_pattern on the resident pair of front_process_stereo; the same four outputs"""
        hh, ww = shape or self._front_shape
        xy = _f32(xy).reshape(-1, 2)
        n = len(xy)
        xyz, status = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        score, match = np.zeros(n, np.float64), np.zeros((n, 2), np.int32)
        self._chk(self.lib.nrs_stereo_match_pattern_front(self.h, C.byref(cam), bf, ww, hh, int(image), n, _p(xy, C.c_float), _p(xyz, C.c_float),
                                                          _p(status, C.c_int32), _p(score, C.c_double), _p(match, C.c_int32)))
        return xyz, status, score, match

    def eval_depth_ground_truth(self, cam, depth, xy):
        """nrs_eval_depth_ground_truth -> (gt_xyz [n,3], gt_status [n]); depth: h x w float32 (a row-strided view is passed as it is)"""
        depth = np.asarray(depth, np.float32)
        if depth.strides[1] != 4 or depth.strides[0] % 4:
            depth = np.ascontiguousarray(depth)
        h, w = depth.shape
        xy = _f32(xy).reshape(-1, 2)
        n = len(xy)
        gt, st = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        self._chk(self.lib.nrs_eval_depth_ground_truth(self.h, C.byref(cam), C.c_void_p(depth.ctypes.data), C.c_int32(w), C.c_int32(h),
                                                       C.c_int32(depth.strides[0] // 4), C.c_int32(n), _p(xy, C.c_float), _p(gt, C.c_float),
                                                       _p(st, C.c_int32)))
        return gt, st

    def eval_frame(self, cam, pose_q, pose_t, world_xyz, xy, depth=None, gt_xyz=None, gt_status=None):
        """nrs_eval_frame -> dict(rmse, scale, counts, gt_world [n,3], gt_status [n], rc): ground truth from a depth image, or from a
        stereo matcher's gt_xyz / gt_status.  rc = -1 with rmse = scale = NaN when the frame has too few points with ground truth"""
        qt = _f32(np.concatenate([np.asarray(pose_q, np.float32), np.asarray(pose_t, np.float32)]))
        X, xy = _f32(world_xyz).reshape(-1, 3), _f32(xy).reshape(-1, 2)
        n = len(X)
        assert len(xy) == n
        rmse, scale = C.c_float(0), C.c_float(0)
        counts = (C.c_int32 * 3)()
        gw, st = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
        d, w, h, stride, g, gs = None, 0, 0, 0, None, None
        if depth is not None:
            d = np.ascontiguousarray(depth, np.float32)
            h, w = d.shape
            stride = w
        else:
            g, gs = _f32(gt_xyz).reshape(-1, 3), _i32(gt_status)
            assert len(g) == n and len(gs) == n
        rc = self.lib.nrs_eval_frame(self.h, C.byref(cam), _p(qt, C.c_float), C.c_int32(n), _p(X, C.c_float), _p(xy, C.c_float), _p(d, C.c_float),
                                     C.c_int32(w), C.c_int32(h), C.c_int32(stride), _p(g, C.c_float), _p(gs, C.c_int32), C.byref(rmse),
                                     C.byref(scale), counts, _p(gw, C.c_float), _p(st, C.c_int32))
        if rc not in (OK, -1) or (rc == -1 and not np.isnan(rmse.value)):
            self._chk(rc)
        return dict(rmse=np.float32(rmse.value), scale=np.float32(scale.value), counts=tuple(counts), gt_world=gw, gt_status=st, rc=rc)

    # ---- a19 / a20
    def graph_select_neighbours(self, g):
        ga = GraphArrays(g)
        n, nnz = len(ga.rowptr) - 1, len(ga.col)
        rp, oc, oe = np.zeros(n + 1, np.int32), np.zeros(nnz, np.int32), np.zeros(nnz, np.int32)
        self._chk(self.lib.nrs_graph_select_neighbours(self.h, C.byref(ga.c), _p(rp, C.c_int32), _p(oc, C.c_int32),
                                                       _p(oe, C.c_int32)))
        return rp, oc[:rp[-1]].copy(), oe[:rp[-1]].copy()

    def graph_update(self, g, pos, ids):
        ga = GraphArrays(g)
        pos = _f32(pos).reshape(-1, 3)
        ids = _i32(ids)
        good = np.zeros(len(ids), np.int32)
        self._chk(self.lib.nrs_graph_update(self.h, C.byref(ga.c), _p(pos, C.c_float), C.c_int32(len(ids)),
                                            _p(ids, C.c_int32), _p(good, C.c_int32)))
        return ga.as_dict(g), good

    # ---- a2
    def track_deform_solve(self, cam, g, map_pos, f_map, f_status, f_uv, f_pos, pose_q, pose_t, scale, trace=None):
        ga = GraphArrays(g)
        map_pos = _f32(map_pos).reshape(-1, 3).copy()
        f_map, f_status = _i32(f_map), _i32(f_status).copy()
        f_uv, f_pos = _f32(f_uv).reshape(-1, 2), _f32(f_pos).reshape(-1, 3).copy()
        qt = np.concatenate([np.asarray(pose_q, np.float64), np.asarray(pose_t, np.float64)])
        med = C.c_float(0)
        n_lost = C.c_int32(0)
        lost = np.zeros(len(map_pos), np.int32)
        self._chk(self.lib.nrs_track_deform_solve(
            self.h, C.byref(cam), C.byref(ga.c), _p(map_pos, C.c_float), C.c_int32(len(f_map)), _p(f_map, C.c_int32),
            _p(f_status, C.c_int32), _p(f_uv, C.c_float), _p(f_pos, C.c_float), _p(qt, C.c_double), C.c_float(scale),
            C.byref(med), C.byref(n_lost), _p(lost, C.c_int32), C.byref(trace.c) if trace else None))
        return dict(pose_q=qt[:4].copy(), pose_t=qt[4:].copy(), f_pos=f_pos, f_status=f_status, map_pos=map_pos,
                    graph=ga.as_dict(g), median=float(med.value), lost=lost[:n_lost.value].tolist())

    def track_deform_solve_rg(self, cam, rg, map_pos, f_map, f_status, f_uv, f_pos, pose_q, pose_t, scale, trace=None, cap_per_point=128):
        """a2 on the device-resident dense graph `rg` (nrs.RGraph of this context); the graph is updated in place"""
        map_pos = _f32(map_pos).reshape(-1, 3).copy()
        assert len(map_pos) == rg.cap
        f_map, f_status = _i32(f_map), _i32(f_status).copy()
        f_uv, f_pos = _f32(f_uv).reshape(-1, 2), _f32(f_pos).reshape(-1, 3).copy()
        qt = np.concatenate([np.asarray(pose_q, np.float64), np.asarray(pose_t, np.float64)])
        med, n_lost = C.c_float(0), C.c_int32(0)
        lost = np.zeros(len(map_pos), np.int32)
        self._chk(self.lib.nrs_track_deform_solve_rg(
            self.h, C.byref(cam), rg.h, C.c_int32(rg.cap), C.c_int32(cap_per_point), _p(map_pos, C.c_float), C.c_int32(len(f_map)),
            _p(f_map, C.c_int32), _p(f_status, C.c_int32), _p(f_uv, C.c_float), _p(f_pos, C.c_float), _p(qt, C.c_double), C.c_float(scale),
            C.byref(med), C.byref(n_lost), _p(lost, C.c_int32), C.byref(trace.c) if trace else None))
        return dict(pose_q=qt[:4].copy(), pose_t=qt[4:].copy(), f_pos=f_pos, f_status=f_status, map_pos=map_pos,
                    median=float(med.value), lost=lost[:n_lost.value].tolist())

    def track_deform_solve_embedded(self, cam, rg, map_pos, f_map, f_status, f_uv, f_pos, f_node, pose_q, pose_t, scale, trace=None, cap_per_point=128):
        """N2 (include/nrs.h nrs_track_deform_solve_embedded): a2 with a node set; the other optimised landmarks are skinned to their nodes"""
        map_pos = _f32(map_pos).reshape(-1, 3).copy()
        assert len(map_pos) == rg.cap
        f_map, f_status = _i32(f_map), _i32(f_status).copy()
        f_uv, f_pos = _f32(f_uv).reshape(-1, 2), _f32(f_pos).reshape(-1, 3).copy()
        f_node = np.ascontiguousarray(f_node, np.uint8)
        assert len(f_node) == len(f_map)
        qt = np.concatenate([np.asarray(pose_q, np.float64), np.asarray(pose_t, np.float64)])
        med, n_lost = C.c_float(0), C.c_int32(0)
        lost = np.zeros(len(map_pos), np.int32)
        self._chk(self.lib.nrs_track_deform_solve_embedded(
            self.h, C.byref(cam), rg.h, C.c_int32(rg.cap), C.c_int32(cap_per_point), _p(map_pos, C.c_float), C.c_int32(len(f_map)),
            _p(f_map, C.c_int32), _p(f_status, C.c_int32), _p(f_uv, C.c_float), _p(f_pos, C.c_float), _p(f_node, C.c_uint8), _p(qt, C.c_double),
            C.c_float(scale), C.byref(med), C.byref(n_lost), _p(lost, C.c_int32), C.byref(trace.c) if trace else None))
        return dict(pose_q=qt[:4].copy(), pose_t=qt[4:].copy(), f_pos=f_pos, f_status=f_status, map_pos=map_pos,
                    median=float(med.value), lost=lost[:n_lost.value].tolist())

    def dba_pack_hash(self):
        """checksums of the packed arrays of the resident BA problem (include/nrs.h nrs_dba_pack_hash); [21] = 1 if device-built"""
        out = (C.c_uint64 * 24)()
        self._chk(self.lib.nrs_dba_pack_hash(self.h, out))
        return list(out)

    def dba_stats(self):
        """sizes of the resident BA problem on this rank (include/nrs.h nrs_dba_stats)"""
        st = (C.c_int64 * 5)()
        self._chk(self.lib.nrs_dba_stats(self.h, st))
        return dict(rows=st[0], packed_rows=st[1], spring_slots=st[2], damper_slots=st[3], device_bytes=st[4])

    def dba_skin_stats(self):
        """skinned observations of the resident embedded window on this rank (include/nrs.h nrs_dba_skin_stats)"""
        st = (C.c_int64 * 3)()
        self._chk(self.lib.nrs_dba_skin_stats(self.h, st))
        return [st[0], st[1], st[2]]

    # ---- N2: skinned mode
    def skin_select_nodes(self, pos, n_nodes, eligible=None):
        """farthest point sampling of n_nodes graph nodes among the eligible points (pick order)"""
        pos = _f32(pos).reshape(-1, 3)
        el = None if eligible is None else np.ascontiguousarray(eligible, np.uint8)
        out = np.zeros(n_nodes, np.int32)
        self._chk(self.lib.nrs_skin_select_nodes(self.h, C.c_int32(len(pos)), _p(pos, C.c_float), _p(el, C.c_uint8) if el is not None else None,
                                                 C.c_int32(n_nodes), _p(out, C.c_int32)))
        return out

    # ---- a21-a23
    def klt_configure(self, win=21, max_level=4, max_iters=10, epsilon=1e-4, min_eig=1e-4):
        cfg = KltConfig(win, max_level, max_iters, epsilon, min_eig)
        self._klt_levels = max_level + 1
        self._chk(self.lib.nrs_klt_configure(self.h, C.byref(cfg)))

    def klt_clear(self):
        self._chk(self.lib.nrs_klt_clear(self.h))

    def klt_num_points(self):
        return self.lib.nrs_klt_num_points(self.h)

    def klt_set_reference(self, img, xy, mask=None):
        img = np.ascontiguousarray(img, np.uint8)
        xy = _f32(xy).reshape(-1, 2)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self._chk(self.lib.nrs_klt_set_reference(self.h, _p(img, C.c_uint8), C.c_int32(img.shape[1]), C.c_int32(img.shape[0]),
                                                 C.c_int32(img.strides[0]), _p(m, C.c_uint8), C.c_int32(len(xy)), _p(xy, C.c_float)))

    def klt_track(self, img, xy, status, initial_flow=True, min_ssim=0.7):
        img = np.ascontiguousarray(img, np.uint8)
        xy = _f32(xy).reshape(-1, 2).copy()
        st = _i32(status).copy()
        good = C.c_int32(0)
        ssim = np.full(len(xy), np.nan, np.float32)
        self._chk(self.lib.nrs_klt_track(self.h, _p(img, C.c_uint8), C.c_int32(img.shape[1]), C.c_int32(img.shape[0]),
                                         C.c_int32(img.strides[0]), C.c_int32(len(xy)), _p(xy, C.c_float), _p(st, C.c_int32),
                                         C.c_int32(1 if initial_flow else 0), C.c_float(min_ssim), C.byref(good), _p(ssim, C.c_float)))
        return xy, st, good.value, ssim

    def klt_get_template(self, idx):
        L = getattr(self, "_klt_levels", 5)
        xy = np.zeros(2, np.float32)
        gray, grad = np.zeros((L, 21, 21), np.int16), np.zeros((L, 21, 21, 2), np.int16)
        mean, valid = np.zeros((L, 2), np.float32), np.zeros(L, np.uint8)
        self._chk(self.lib.nrs_klt_get_template(self.h, C.c_int32(idx), _p(xy, C.c_float), _p(gray, C.c_int16),
                                                _p(grad, C.c_int16), _p(mean, C.c_float), _p(valid, C.c_uint8)))
        return dict(xy=xy, gray=gray, grad=grad, mean=mean, valid=valid)

    def klt_insert_template(self, t):
        xy, gray, grad = _f32(t["xy"]), np.ascontiguousarray(t["gray"], np.int16), np.ascontiguousarray(t["grad"], np.int16)
        mean, valid = _f32(t["mean"]), np.ascontiguousarray(t["valid"], np.uint8)
        self._chk(self.lib.nrs_klt_insert_template(self.h, _p(xy, C.c_float), _p(gray, C.c_int16), _p(grad, C.c_int16),
                                                   _p(mean, C.c_float), _p(valid, C.c_uint8)))

    def klt_get_templates(self, first, count):
        """list of `count` template dicts (same layout as klt_get_template), one device read."""
        L = getattr(self, "_klt_levels", 5)
        xy = np.zeros((count, 2), np.float32)
        gray, grad = np.zeros((count, L, 21, 21), np.int16), np.zeros((count, L, 21, 21, 2), np.int16)
        mean, valid = np.zeros((count, L, 2), np.float32), np.zeros((count, L), np.uint8)
        self._chk(self.lib.nrs_klt_get_templates(self.h, C.c_int32(first), C.c_int32(count), _p(xy, C.c_float), _p(gray, C.c_int16),
                                                 _p(grad, C.c_int16), _p(mean, C.c_float), _p(valid, C.c_uint8)))
        return [dict(xy=xy[i], gray=gray[i], grad=grad[i], mean=mean[i], valid=valid[i]) for i in range(count)]

    def klt_archive_templates(self, slots, keys):
        """copy the templates of tracker slots into this context's device-side archive under `keys` (include/nrs.h nrs_klt_archive_templates)"""
        slots, keys = _i32(slots), _i32(keys)
        assert len(slots) == len(keys)
        self._chk(self.lib.nrs_klt_archive_templates(self.h, C.c_int32(len(slots)), _p(slots, C.c_int32), _p(keys, C.c_int32)))

    def klt_insert_archived(self, src, keys, xy):
        """append the archive entries `keys` of context `src` to this context's tracker at positions xy (nrs_klt_insert_archived)"""
        keys, xy = _i32(keys), _f32(xy).reshape(-1, 2)
        assert len(keys) == len(xy)
        self._chk(self.lib.nrs_klt_insert_archived(self.h, src.h, C.c_int32(len(keys)), _p(keys, C.c_int32), _p(xy, C.c_float)))

    def point_reuse(self, cam, pose_q, pose_t, wh, map_pos, frame_slot, slot_status, lost, min_ssim=0.75, insert_new=True):
        """Tracking::PointReuse in one call on this context's resident pyramid and archive (include/nrs.h nrs_point_reuse).  frame_slot: per
        map point the frame slot that holds it or -1; slot_status: the frame's LandmarkStatus per slot; lost: map indices.  Returns
        dict(n_cand, cand_id, seed_xy, xy, status, accepted (bool), n_reused, n_new), the arrays trimmed to n_cand."""
        qt = np.concatenate([_f32(pose_q).reshape(4), _f32(pose_t).reshape(3)]).astype(np.float32)
        map_pos = _f32(map_pos).reshape(-1, 3)
        frame_slot, slot_status = _i32(frame_slot).reshape(-1), _i32(slot_status).reshape(-1)
        lost = _i32(sorted(int(x) for x in lost)) if isinstance(lost, (set, frozenset)) else _i32(lost).reshape(-1)
        n = len(map_pos)
        assert len(frame_slot) == n
        cap = max(n, 1)
        cand, st, acc = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        seed, xy = np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32)
        n_cand, n_reused, n_new = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.nrs_point_reuse(
            self.h, C.byref(cam), _p(qt, C.c_float), C.c_int32(int(wh[0])), C.c_int32(int(wh[1])), C.c_int32(n), _p(map_pos, C.c_float),
            _p(frame_slot, C.c_int32), C.c_int32(len(slot_status)), _p(slot_status, C.c_int32), C.c_int32(len(lost)), _p(lost, C.c_int32),
            C.c_float(min_ssim), C.c_int32(1 if insert_new else 0), C.byref(n_cand), _p(cand, C.c_int32), _p(seed, C.c_float), _p(xy, C.c_float),
            _p(st, C.c_int32), _p(acc, C.c_int32), C.byref(n_reused), C.byref(n_new)))
        k = n_cand.value
        return dict(n_cand=k, cand_id=cand[:k].copy(), seed_xy=seed[:k].copy(), xy=xy[:k].copy(), status=st[:k].copy(), accepted=acc[:k] != 0,
                    n_reused=n_reused.value, n_new=n_new.value)

    def klt_insert_templates(self, ts):
        """append several templates (each as returned by klt_get_template; levels beyond this tracker's are ignored)."""
        L = getattr(self, "_klt_levels", 5)
        if not ts:
            return
        xy = np.ascontiguousarray(np.stack([_f32(t["xy"]) for t in ts]), np.float32)
        gray = np.ascontiguousarray(np.stack([np.asarray(t["gray"], np.int16)[:L] for t in ts]))
        grad = np.ascontiguousarray(np.stack([np.asarray(t["grad"], np.int16)[:L] for t in ts]))
        mean = np.ascontiguousarray(np.stack([_f32(t["mean"])[:L] for t in ts]), np.float32)
        valid = np.ascontiguousarray(np.stack([np.asarray(t["valid"], np.uint8)[:L] for t in ts]))
        self._chk(self.lib.nrs_klt_insert_templates(self.h, C.c_int32(len(ts)), _p(xy, C.c_float), _p(gray, C.c_int16),
                                                    _p(grad, C.c_int16), _p(mean, C.c_float), _p(valid, C.c_uint8)))

    # ---- a3
    def _dba_args(self, cam, poses_qt, lm_xyz, lm_kf, lm_uv, edges, scale):
        self._keep = (np.ascontiguousarray(poses_qt, np.float64).reshape(-1, 7), _f32(lm_xyz).reshape(-1, 3),
                      _i32(lm_kf), _f32(lm_uv).reshape(-1, 2), _i32(edges["sp_ij"]).reshape(-1, 2),
                      _f32(edges["sp_d0"]), _i32(edges["dm_idx"]).reshape(-1, 4), _f32(edges["dm_w"]))
        pq, xyz, kf, uv, sp, d0, dm, dw = self._keep
        return [self.h, C.byref(cam), C.c_int32(len(pq)), _p(pq, C.c_double), C.c_int32(len(xyz)),
                _p(xyz, C.c_float), _p(kf, C.c_int32), _p(uv, C.c_float), C.c_int32(len(sp)),
                _p(sp, C.c_int32), _p(d0, C.c_float), C.c_int32(len(dm)), _p(dm, C.c_int32),
                _p(dw, C.c_float), C.c_float(scale)]

    def dba_solve(self, cam, poses_qt, lm_xyz, lm_kf, lm_uv, edges, scale, iters=5, trace=None):
        args = self._dba_args(cam, np.array(poses_qt, np.float64), np.array(lm_xyz, np.float32),
                              lm_kf, lm_uv, edges, scale)
        self._chk(self.lib.nrs_dba_solve(*args, C.c_int32(iters), C.byref(trace.c) if trace else None))
        return self._keep[0].copy(), self._keep[1].copy()

    def _window_args(self, poses_qt, kf_points, xyz, uv):
        """what the four one-call window wrappers marshal alike: (n_kf, kf_rowptr, kf_pt, poses n_kf x 7, points as a fresh fp32 copy the call
        writes into, uv), one row of xyz and of uv per entry of kf_points"""
        n_kf = len(kf_points)
        kf_rowptr = np.zeros(n_kf + 1, np.int32)
        kf_rowptr[1:] = np.cumsum([len(k) for k in kf_points])
        kf_pt = _i32(np.concatenate(kf_points))
        pq = np.ascontiguousarray(np.array(poses_qt, np.float64)).reshape(-1, 7)
        xyz = np.array(xyz, np.float32).reshape(-1, 3).copy()
        uv = _f32(uv).reshape(-1, 2)
        assert len(pq) == n_kf and len(xyz) == len(kf_pt) == len(uv)
        return n_kf, kf_rowptr, kf_pt, pq, xyz, uv

    def _embedded_window_counts(self, n_kf):
        """the counts of the resident embedded window, for the downloads and taps that size their arrays by them"""
        n = [C.c_int32(0) for _ in range(4)]
        self._chk(self.lib.nrs_dba_window_edges_embedded(self.h, None, C.byref(n[0]), None, C.byref(n[1]), None, None, C.byref(n[2]), None, None, C.byref(n[3]), None, None, None))
        self._n_kf, self._n_lm, self._n_sp, self._n_dm, self._n_skin = n_kf, n[0].value, n[1].value, n[2].value, n[3].value

    def dba_solve_window(self, cam, poses_qt, kf_points, lm_xyz, lm_uv, graph, scale, iters=5, trace=None):
        """LocalDeformableBundleAdjustment in one call (include/nrs.h nrs_dba_solve_window): edge construction included"""
        n_kf, kf_rowptr, kf_pt, pq, xyz, uv = self._window_args(poses_qt, kf_points, lm_xyz, lm_uv)
        rp, col, w, d0, st = (_i32(graph["rowptr"]), _i32(graph["col"]), _f32(graph["w"]), _f32(graph["d0"]), _i32(graph["status"]))
        self._chk(self.lib.nrs_dba_solve_window(self.h, C.byref(cam), C.c_int32(n_kf), _p(pq, C.c_double), _p(kf_rowptr, C.c_int32), _p(kf_pt, C.c_int32),
                                                _p(xyz, C.c_float), _p(uv, C.c_float), C.c_int32(len(rp) - 1), _p(rp, C.c_int32), _p(col, C.c_int32),
                                                _p(w, C.c_float), _p(d0, C.c_float), _p(st, C.c_int32), C.c_float(scale), C.c_int32(iters),
                                                C.byref(trace.c) if trace else None))
        return pq, xyz

    def dba_solve_window_rg(self, cam, poses_qt, kf_points, lm_xyz, lm_uv, rg, scale, iters=5, trace=None, cap_per_point=0):
        """LocalDeformableBundleAdjustment served by the device-resident graph rg (include/nrs.h nrs_dba_solve_window_rg): kf_points hold
        map-point indices = the graph's; cap_per_point = the first GetEdges prefix (<= 0: the library's default), doubled while a walk runs off"""
        n_kf, kf_rowptr, kf_pt, pq, xyz, uv = self._window_args(poses_qt, kf_points, lm_xyz, lm_uv)
        self._chk(self.lib.nrs_dba_solve_window_rg(self.h, C.byref(cam), C.c_int32(n_kf), _p(pq, C.c_double), _p(kf_rowptr, C.c_int32), _p(kf_pt, C.c_int32),
                                                   _p(xyz, C.c_float), _p(uv, C.c_float), rg.h, C.c_int32(cap_per_point), C.c_float(scale), C.c_int32(iters),
                                                   C.byref(trace.c) if trace else None))
        return pq, xyz

    def dba_window_rg_stats(self):
        """dict(n_points, cap, rounds, ran_off_first) of the resident window dba_solve_window_rg made (nrs_dba_window_rg_stats)"""
        out = (C.c_int64 * 4)()
        self._chk(self.lib.nrs_dba_window_rg_stats(self.h, out))
        return dict(n_points=int(out[0]), cap=int(out[1]), rounds=int(out[2]), ran_off_first=int(out[3]))

    def dba_window_edge_counts(self):
        """(springs, dampers) of the resident window"""
        ns, nd = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.nrs_dba_window_edges(self.h, C.byref(ns), None, None, C.byref(nd), None, None))
        return ns.value, nd.value

    def dba_window_edges(self):
        """edge lists of the resident window as the device built them (None if they were built on the host)"""
        ns, nd = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.nrs_dba_window_edges(self.h, C.byref(ns), None, None, C.byref(nd), None, None))
        sp_ij, sp_d0 = np.zeros((ns.value, 2), np.int32), np.zeros(ns.value, np.float32)
        dm_idx, dm_w = np.zeros((nd.value, 4), np.int32), np.zeros(nd.value, np.float32)
        rc = self.lib.nrs_dba_window_edges(self.h, C.byref(ns), _p(sp_ij, C.c_int32), _p(sp_d0, C.c_float), C.byref(nd), _p(dm_idx, C.c_int32), _p(dm_w, C.c_float))
        if rc == -5:
            return None
        self._chk(rc)
        return dict(sp_ij=sp_ij, sp_d0=sp_d0, dm_idx=dm_idx, dm_w=dm_w)

    def dba_solve_window_embedded(self, cam, poses_qt, kf_points, obs_xyz, obs_uv, is_node, graph, scale, iters=5, trace=None):
        """The embedded window in one call (include/nrs.h nrs_dba_solve_window_embedded): the lists of dba_build_edges_embedded are built
        on the device.  obs_xyz / obs_uv are per observation (position in the concatenation of kf_points).  Returns (poses_qt, obs_xyz):
        node copies optimised, skinned observations at their skinned position, observations bound to nothing unchanged."""
        n_kf, kf_rowptr, kf_pt, pq, xyz, uv = self._window_args(poses_qt, kf_points, obs_xyz, obs_uv)
        node = None if is_node is None else np.ascontiguousarray(is_node, np.uint8)
        rp, col, w, d0, st = (_i32(graph["rowptr"]), _i32(graph["col"]), _f32(graph["w"]), _f32(graph["d0"]), _i32(graph["status"]))
        assert node is None or len(node) == len(rp) - 1
        self._chk(self.lib.nrs_dba_solve_window_embedded(self.h, C.byref(cam), C.c_int32(n_kf), _p(pq, C.c_double), _p(kf_rowptr, C.c_int32), _p(kf_pt, C.c_int32),
                                                         _p(xyz, C.c_float), _p(uv, C.c_float), C.c_int32(len(rp) - 1),
                                                         None if node is None else _p(node, C.c_uint8), _p(rp, C.c_int32), _p(col, C.c_int32),
                                                         _p(w, C.c_float), _p(d0, C.c_float), _p(st, C.c_int32), C.c_float(scale), C.c_int32(iters),
                                                         C.byref(trace.c) if trace else None))
        self._embedded_window_counts(n_kf)
        return pq, xyz

    def dba_solve_window_rg_embedded(self, cam, poses_qt, kf_points, obs_xyz, obs_uv, rg, is_node, scale, iters=5, trace=None, cap_per_point=0):
        """The embedded window served by the device-resident graph rg (include/nrs.h nrs_dba_solve_window_rg_embedded): kf_points hold
        map-point indices = the graph's, is_node is indexed by them and has rg.cap entries; cap_per_point as for dba_solve_window_rg.
        Returns (poses_qt, obs_xyz) as dba_solve_window_embedded; dba_window_edges_embedded and dba_window_rg_stats answer afterwards."""
        n_kf, kf_rowptr, kf_pt, pq, xyz, uv = self._window_args(poses_qt, kf_points, obs_xyz, obs_uv)
        node = None if is_node is None else np.ascontiguousarray(is_node, np.uint8)
        assert node is None or len(node) == rg.cap
        self._chk(self.lib.nrs_dba_solve_window_rg_embedded(self.h, C.byref(cam), C.c_int32(n_kf), _p(pq, C.c_double), _p(kf_rowptr, C.c_int32), _p(kf_pt, C.c_int32),
                                                            _p(xyz, C.c_float), _p(uv, C.c_float), rg.h, None if node is None else _p(node, C.c_uint8),
                                                            C.c_int32(cap_per_point), C.c_float(scale), C.c_int32(iters), C.byref(trace.c) if trace else None))
        self._embedded_window_counts(n_kf)
        return pq, xyz

    def dba_window_edges_embedded(self):
        """lists of the resident window dba_solve_window_embedded made: the keys of dba_build_edges_embedded plus on_device (1: built on
        the device); NrsError NRS_ERR_STATE when the resident window was made by another call.  On a rank of a communicator the counts
        and sk_obs are the window's and sk_node / sk_omega the rank's rows [sk_base, sk_base + sk_held) (dba_window_slice_embedded);
        sk_base / sk_held are in the dict as well"""
        dev, nl, ns, nd, nk = (C.c_int32(0) for _ in range(5))
        sl = self.dba_window_slice_embedded()
        self._chk(self.lib.nrs_dba_window_edges_embedded(self.h, C.byref(dev), C.byref(nl), None, C.byref(ns), None, None, C.byref(nd), None, None, C.byref(nk), None, None, None))
        lm_obs = np.zeros(nl.value, np.int32)
        sp_ij, sp_d0 = np.zeros((ns.value, 2), np.int32), np.zeros(ns.value, np.float32)
        dm_idx, dm_w = np.zeros((nd.value, 4), np.int32), np.zeros(nd.value, np.float32)
        sk_obs, sk_node, sk_omega = np.zeros(nk.value, np.int32), np.zeros((sl["sk_held"], 11), np.int32), np.zeros((sl["sk_held"], 11), np.float64)
        self._chk(self.lib.nrs_dba_window_edges_embedded(self.h, C.byref(dev), C.byref(nl), _p(lm_obs, C.c_int32), C.byref(ns), _p(sp_ij, C.c_int32), _p(sp_d0, C.c_float),
                                                         C.byref(nd), _p(dm_idx, C.c_int32), _p(dm_w, C.c_float), C.byref(nk), _p(sk_obs, C.c_int32),
                                                         _p(sk_node, C.c_int32), _p(sk_omega, C.c_double)))
        return dict(lm_obs=lm_obs, sp_ij=sp_ij, sp_d0=sp_d0, dm_idx=dm_idx, dm_w=dm_w, sk_obs=sk_obs, sk_node=sk_node, sk_omega=sk_omega, on_device=dev.value,
                    sk_base=sl["sk_base"], sk_held=sl["sk_held"])

    def dba_window_slice_embedded(self):
        """this rank's share of the resident window dba_solve_window_embedded made (include/nrs.h nrs_dba_window_slice_embedded):
        dict(sk_base, sk_held, k0, k1, stage_bytes, sk_stage_bytes); a whole window: 0, n_skin, 0, n_kf"""
        out = (C.c_int64 * 6)()
        self._chk(self.lib.nrs_dba_window_slice_embedded(self.h, out))
        return dict(zip(("sk_base", "sk_held", "k0", "k1", "stage_bytes", "sk_stage_bytes"), (int(v) for v in out)))

    def dba_upload(self, cam, poses_qt, lm_xyz, lm_kf, lm_uv, edges, scale):
        args = self._dba_args(cam, poses_qt, lm_xyz, lm_kf, lm_uv, edges, scale)
        self._n_kf, self._n_lm = len(self._keep[0]), len(self._keep[1])
        self._n_sp, self._n_dm = len(self._keep[4]), len(self._keep[6])
        self._chk(self.lib.nrs_dba_upload(*args))

    # ---- N2b: the embedded window (nrs_dba_*_embedded): w = nrs_synth.embedded_window(p, e), e = dba_build_edges_embedded(...)
    def _dba_args_embedded(self, cam, poses_qt, w, e, scale):
        args = self._dba_args(cam, poses_qt, w["lm_xyz"], w["lm_kf"], w["lm_uv"], e, scale)
        self._keep_sk = (_i32(w["sk_kf"]), _f32(w["sk_uv"]).reshape(-1, 2), np.array(w["sk_xyz"], np.float32).reshape(-1, 3).copy(),
                         _i32(e["sk_node"]).reshape(-1, 11), np.ascontiguousarray(e["sk_omega"], np.float64).reshape(-1, 11))
        kf, uv, xyz, node, om = self._keep_sk
        self._n_skin = len(kf)
        return args[:-1] + [C.c_int32(len(kf)), _p(kf, C.c_int32), _p(uv, C.c_float), _p(xyz, C.c_float), _p(node, C.c_int32), _p(om, C.c_double), args[-1]]

    def dba_upload_embedded(self, cam, poses_qt, w, e, scale):
        args = self._dba_args_embedded(cam, poses_qt, w, e, scale)
        self._n_kf, self._n_lm = len(self._keep[0]), len(self._keep[1])
        self._n_sp, self._n_dm = len(self._keep[4]), len(self._keep[6])
        self._chk(self.lib.nrs_dba_upload_embedded(*args))

    def dba_download_skinned(self):
        xyz = np.zeros((self._n_skin, 3), np.float64)
        self._chk(self.lib.nrs_dba_download_skinned(self.h, _p(xyz, C.c_double)))
        return xyz

    def dba_solve_embedded(self, cam, poses_qt, w, e, scale, iters=5, trace=None):
        """one shot; returns (poses_qt, node copies fp32, skinned points fp32)"""
        args = self._dba_args_embedded(cam, np.array(poses_qt, np.float64), dict(w, lm_xyz=np.array(w["lm_xyz"], np.float32)), e, scale)
        self._chk(self.lib.nrs_dba_solve_embedded(*args, C.c_int32(iters), C.byref(trace.c) if trace else None))
        return self._keep[0].copy(), self._keep[1].copy(), self._keep_sk[2].copy()

    def dba_reset(self):
        self._chk(self.lib.nrs_dba_reset(self.h))

    def dba_optimize(self, iters=5, trace=None):
        self._chk(self.lib.nrs_dba_optimize(self.h, C.c_int32(iters), C.byref(trace.c) if trace else None))

    def dba_download(self):
        pq = np.zeros((self._n_kf, 7), np.float64)
        xyz = np.zeros((self._n_lm, 3), np.float64)
        self._chk(self.lib.nrs_dba_download(self.h, _p(pq, C.c_double), _p(xyz, C.c_double)))
        return pq, xyz

    def dba_residuals(self):
        rr = np.zeros((self._n_lm, 2), np.float64)
        rs = np.zeros(self._n_sp, np.float64)
        rd = np.zeros((self._n_dm, 3), np.float64)
        self._chk(self.lib.nrs_dba_residuals(self.h, _p(rr, C.c_double), _p(rs, C.c_double), _p(rd, C.c_double)))
        return rr, rs, rd

    def debug_pcg_solve(self, Hpp21, bp, D6, Hpl18, bl, lam=0.0):
        """include/nrs.h nrs_debug_pcg_solve: returns (x[6 + 3n], PCG iterations)."""
        D6 = np.ascontiguousarray(D6, np.float64).reshape(-1, 6)
        n = len(D6)
        Hpp21, bp = np.ascontiguousarray(Hpp21, np.float64), np.ascontiguousarray(bp, np.float64)
        Hpl18 = np.ascontiguousarray(Hpl18, np.float64).reshape(n, 18)
        bl = np.ascontiguousarray(bl, np.float64).reshape(n, 3)
        x = np.zeros(6 + 3 * n, np.float64)
        it = C.c_int32(0)
        self._chk(self.lib.nrs_debug_pcg_solve(self.h, C.c_int32(n), _p(Hpp21, C.c_double), _p(bp, C.c_double), _p(D6, C.c_double),
                                               _p(Hpl18, C.c_double), _p(bl, C.c_double), C.c_double(lam), _p(x, C.c_double), C.byref(it)))
        return x, it.value

    def nd_cache_stats(self):
        """include/nrs.h nrs_debug_nd_cache_stats: (problems that reused a cached plan, plans built)"""
        out = np.zeros(2, np.int64)
        self._chk(self.lib.nrs_debug_nd_cache_stats(self.h, _p(out, C.c_int64)))
        return int(out[0]), int(out[1])

    def debug_nd_solve(self, pos, last, pairs, Dn, Vp, bn, lam=0.0, repeats=0):
        """include/nrs.h nrs_debug_nd_solve: the direct (nested-dissection) solver's device kernels on an explicit block system.
        Returns (ok, x [n,3], stats dict, ms per solve)."""
        pos = np.ascontiguousarray(pos, np.float64)
        n = len(pos)
        last = None if last is None else np.ascontiguousarray(last, np.uint8)
        pairs = _i32(np.asarray(pairs).reshape(-1, 2))
        Dn, Vp, bn = (np.ascontiguousarray(a, np.float64) for a in (Dn, Vp, bn))
        x = np.zeros((n, 3))
        st = np.zeros(8, np.int64)
        ms = C.c_double(0)
        rc = self.lib.nrs_debug_nd_solve(self.h, C.c_int32(n), _p(pos, C.c_double), None if last is None else _p(last, C.c_uint8), C.c_int32(len(pairs)),
                                         _p(pairs, C.c_int32), _p(Dn, C.c_double), _p(Vp, C.c_double), _p(bn, C.c_double), C.c_double(lam),
                                         C.c_int32(repeats), _p(x, C.c_double), _p(st, C.c_int64), C.byref(ms))
        if rc not in (0, -6):
            self._chk(rc)
        keys = ("fronts", "levels", "max_s", "max_b", "L_doubles", "U_doubles", "flops", "workgroups")
        return rc == 0, x, dict(zip(keys, st.tolist())), ms.value

    def debug_set(self, name, value):
        """a debug / A-B switch of THIS context (include/nrs.h nrs_debug_set); value None: unset"""
        if self.h:
            self._chk(self.lib.nrs_debug_set(self.h, name.encode(), None if value is None else str(value).encode()))

    def debug_kft_info(self):
        """the keyframe-block factorisation of the resident embedded window: dict(on, K, ld, nb, m, mib, nf[K], np[K])"""
        o = np.zeros(6 + 2 * max(1, self._n_kf), np.int32)
        self._chk(self.lib.nrs_debug_kft(self.h, C.c_double(0.0), C.c_int32(0), C.c_int32(0), None, None, _p(o, C.c_int32)))
        K = self._n_kf
        return dict(on=bool(o[0]), K=int(o[1]), ld=int(o[2]), nb=int(o[3]), m=int(o[4]), mib=int(o[5]), nf=o[6:6 + K].copy(), np=o[6 + K:6 + 2 * K].copy())

    def debug_kft_block(self, lam, k, coupling=False):
        ld = self.debug_kft_info()["ld"]
        a = np.zeros((ld, ld), np.float64)
        self._chk(self.lib.nrs_debug_kft(self.h, C.c_double(lam), C.c_int32(2 if coupling else 1), C.c_int32(k), None, _p(a, C.c_double), None))
        return a

    def debug_kft_apply(self, lam, r):
        r = np.ascontiguousarray(r, np.float64)
        u = np.zeros_like(r)
        self._chk(self.lib.nrs_debug_kft(self.h, C.c_double(lam), C.c_int32(3), C.c_int32(0), _p(r, C.c_double), _p(u, C.c_double), None))
        return u

    def debug_kft_share(self):
        """this rank's share of the keyframe-block factorisation: dict(k0, nk, m, r_m, kib, handovers) (one GPU: the whole window)"""
        o = np.zeros(6, np.int32)
        self._chk(self.lib.nrs_debug_kft(self.h, C.c_double(0.0), C.c_int32(5), C.c_int32(0), None, None, _p(o, C.c_int32)))
        return dict(k0=int(o[0]), nk=int(o[1]), m=int(o[2]), r_m=int(o[3]), kib=int(o[4]), handovers=int(o[5]))

    def debug_kft_index(self):
        o = np.zeros((self._n_lm, 2), np.int32)
        self._chk(self.lib.nrs_debug_kft(self.h, C.c_double(0.0), C.c_int32(4), C.c_int32(0), None, None, _p(o, C.c_int32)))
        return o

    def dba_gradient(self):
        n = 6 * self._n_kf + 3 * self._n_lm
        b = np.zeros(n, np.float64)
        d = np.zeros(n, np.float64)
        self._chk(self.lib.nrs_dba_gradient(self.h, _p(b, C.c_double), _p(d, C.c_double)))
        return b, d


def skinned_status(f_status, f_map, nodes):
    """Skinned mode (include/nrs.h, N2): the nodes keep TRACKED_WITH_3D (0), every other TRACKED_WITH_3D point of the frame
    becomes TRACKED (1: in the frame, no 3D) and is carried by stage 2 of the pose-and-deformation solve"""
    st = np.array(f_status, np.int32)
    nodes = np.asarray(nodes, np.int64)
    is_node = np.zeros(int(max(np.max(f_map), nodes.max() if nodes.size else -1)) + 1, bool)
    is_node[nodes] = True
    fm = np.asarray(f_map)
    demote = (st == 0) & (fm >= 0) & ~is_node[np.maximum(fm, 0)]
    st[demote] = 1
    return st
