"""Frame-loop harness: this build's counterpart of the tracked-frame branch of
Tracking::TrackImage (reference modules/tracking/tracking.cc:72-112): DataAssociation (LK,
:304-307) -> CameraPoseEstimation (motion-model seed + pose-only solve, :309-319) ->
CameraPoseAndDeformationEstimation (:321-333) -> PointReuse (:394-506) -> KeyFrameInsertion
cadence (:336-392) -> SetLastFrame.  It only orchestrates: every numerical step is a call through a
*backend* -- `GpuBackend` = the C ABI of libnrs_hip.so through ctypes (one context for the main
tracker, one for the two-level reuse tracker -- or, with device_reuse=True, PointReuse as one call
on the main context: nrs_point_reuse); the tests plug the oracle in behind the same calls.

Keyframes extract new Shi-Tomasi features (tracking.cc:350-372): they enter the frame
as TRACKED observations without a map point and are followed by LK from then on.  The map is started by `MonoInitializer` +
`FrameLoop.from_initialization` (tracking.cc:136-214).  With mapping=True the loop also runs the FrameMapping branch of Mapping::DoMapping
(mapping.cc:36-63) after every tracked frame -- the temporal buffer's snapshot (temporal_buffer.cc:28-56), Mapping::LandmarkTriangulation
in one backend call, AddGeometryToKeypoint, graph growth -- and Tracking::UpdateTriangulatedPoints (tracking.cc:508-521) at the start of
the next one, so those features become map points.  With keyframe_ba=True (on top of mapping=True) the other branch runs as well: the loop
keeps the map's keyframes and its unmapped queue (map.cc:37-72), runs Mapping::KeyFrameMapping = LocalDeformableBundleAdjustment on the
last five keyframes in one backend call (`dba_window`) and Mapping::UpdateTrackingFrameFromKeyFrame (mapping.cc:44-58, 266-270); without
it the loop logs on those frames that it skipped the step.  Not reproduced: visualisation.

Poses are Sophus::SE3f in the reference: unit quaternion + translation in float32, and so is the
motion-model algebra here (`se3f_*`)."""
import numpy as np

F32 = np.float32
TRACKED_WITH_3D, TRACKED, JUST_TRIANGULATED, BAD = 0, 1, 2, 3     # utilities/landmark_status.h:23-30


# ---- SE3f (xyzw quaternion, translation), float32 arithmetic ---------------------------------
def quat_mul_f(a, b):
    ax, ay, az, aw = [F32(v) for v in a]
    bx, by, bz, bw = [F32(v) for v in b]
    q = np.array([aw * bx + ax * bw + ay * bz - az * by,
                  aw * by - ax * bz + ay * bw + az * bx,
                  aw * bz + ax * by - ay * bx + az * bw,
                  aw * bw - ax * bx - ay * by - az * bz], F32)
    return (q / F32(np.sqrt(np.dot(q, q)))).astype(F32)


def quat_rot_f(q, v):
    x, y, z, w = [F32(c) for c in q]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], F32)
    return (R @ np.asarray(v, F32)).astype(F32)


def se3f_mul(a, b):
    return quat_mul_f(a[0], b[0]), (np.asarray(a[1], F32) + quat_rot_f(a[0], b[1])).astype(F32)


def se3f_act(a, X):
    """a * X for many points, float32, one fixed elementwise expression per coordinate."""
    x, y, z, w = [F32(c) for c in a[0]]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], F32)
    X = np.asarray(X, F32).reshape(-1, 3)
    t = np.asarray(a[1], F32)
    return np.stack([R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1] + R[r, 2] * X[:, 2] + t[r] for r in range(3)], 1).astype(F32)


def se3f_inv(a):
    qi = np.array([-a[0][0], -a[0][1], -a[0][2], a[0][3]], F32)
    return qi, (-quat_rot_f(qi, a[1])).astype(F32)


def project_f32(model, prm, p):
    """CameraModel::Project in float32 (calibration/pin_hole.cc:27-33, kannala_brandt_8.cc:34-51); the
    KB8 trigonometry as defined in include/nrs.h (double function rounded to float)."""
    prm = np.asarray(prm, F32)
    p = np.asarray(p, F32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    if model == 0:
        return np.stack([prm[0] * x / z + prm[2], prm[1] * y / z + prm[3]], 1).astype(F32)
    r2 = x * x + y * y
    th = np.arctan2(np.sqrt(r2).astype(np.float64), z.astype(np.float64)).astype(F32)
    psi = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(F32)
    th2 = th * th
    th3 = th * th2
    th5 = th3 * th2
    th7 = th5 * th2
    th9 = th7 * th2
    r = th + prm[4] * th3 + prm[5] * th5 + prm[6] * th7 + prm[7] * th9
    return np.stack([prm[0] * r * np.cos(psi.astype(np.float64)).astype(F32) + prm[2],
                     prm[1] * r * np.sin(psi.astype(np.float64)).astype(F32) + prm[3]], 1).astype(F32)


class GpuBackend:
    """The product path: one nrs context for the main tracker and, made on first use, one for PointReuse's two-level tracker (with
    device_reuse=True PointReuse is one call on the main context and the second one is never made)."""

    def __init__(self, nrs, model, prm, klt_opts, dense_graph=False, cap_per_point=64, direct_solve=0, n_nodes=0, front=None, device_reuse=False,
                 device_tbuf=False, rectify=None, resize=None):
        """n_nodes > 0: EMBEDDED-DEFORMATION mode (include/nrs.h nrs_track_deform_solve_embedded; needs the dense graph): n_nodes map points
        (farthest-point sampling on the initial map, nrs_skin_select_nodes) carry the deformation vertices for the whole sequence, every
        other tracked point is skinned to <= 11 of them in the pose-and-deformation solve of each frame (tracking.cc:321-333's call).  Mapping
        keeps that node set (map points added later are always skinned) and keyframe BA runs as nrs_dba_solve_window_rg_embedded
        front: None / False = the images handed to the loop are grey and go to the tracker as they are, without masks (as before).  True or a
        list of filters (nrs.Context.front_configure) = the loop is handed the RAW frames of System::TrackImage (SLAM/system.cc:113-132): each
        is uploaded once through nrs_front_process, LK and Shi-Tomasi run on the resident grey image (tracking.cc:92,353,367) and
        SetReferenceImage / ExtractFeatures take the resident Global mask.  PointReuse's own tracker, a second context, still gets
        the grey bytes from the host -- unless device_reuse is on.
        device_reuse: True = FrameLoop.point_reuse makes ONE call, nrs_point_reuse, on the main context: candidates, the two-level tracker on
        the pyramid this frame's klt_track built, the 5.99 gate and the append of the new slots (include/nrs.h); no image goes anywhere.
        False (the default) = the two-context path: host projection, reuse_track_archived on ctx_reuse, insert_archived.
        device_tbuf: True = the loop's TemporalBuffer is the resident one of the main context (include/nrs.h nrs_tbuf): a frame enters
        with one upload (tbuf_insert) and frame mapping reads it in place (map_frame_resident), which hands keypoint ids back.
        False (the default) = nrs_frame_loop.TemporalBuffer on the host, flattened and uploaded whole by every map_frame.
        rectify: None (the default) = a stereo pair handed to front_stereo is rectified already.  dict(src_wh=(w, h), dst_wh=(w, h), left=eye
        record, right=eye record) (nrs.Context.front_rectify_configure; needs the front mode) = front_stereo is handed the RAW eyes, as the
        camera gives them, and rectifies them on the device (nrs_front_process_stereo_raw): every later step sees the rectified pair.
        resize: None (the default) = a frame handed to the loop has the size it is tracked at.  dict(src_wh=(w, h), dst_wh=(w, h))
        (nrs.Context.front_resize_configure; needs the front mode; nrs.half_size gives the dst_wh of apps/endomapper.cc:65-69) = every
        single-frame step is handed the RAW frame, as the video decoder gives it, and resizes it on the device (nrs_front_process_raw):
        every later step sees the resized frame.  front_stereo is unaffected: no loader resizes a pair."""
        self.nrs = nrs
        self.device_tbuf, self.tb = bool(device_tbuf), None
        self.dense, self.cap, self.rg = dense_graph or n_nodes > 0, cap_per_point, None
        self.n_nodes, self.node_flag = n_nodes, None
        self.cam = nrs.make_camera(model, prm)
        self.ctx = nrs.Context(direct_solve=direct_solve)      # (nrs_options.direct_solve: the linear solver of the pose-and-deformation solve)
        self._ctx_reuse = None                                 # (made by the first step that needs it: the ctx_reuse property)
        self.device_reuse, self.n_device_reuse = bool(device_reuse), 0
        self.klt_opts = klt_opts
        self.ctx.klt_configure(klt_opts["win"], klt_opts["max_level"], klt_opts["max_iters"], klt_opts["epsilon"], klt_opts["min_eig"])
        self.front = bool(front) or isinstance(front, (list, tuple))
        self._front_im, self._front_gray = None, None
        self._front_right, self._front_fresh, self.n_front_calls = None, None, 0      # (n_front_calls: front-end calls made, one or two eyes each)
        if self.front:
            self.ctx.front_configure(front if isinstance(front, (list, tuple)) else ())
        self.rectify = rectify is not None
        if self.rectify:
            if not self.front:
                raise ValueError("rectify needs the front mode (front=True or a list of filters)")
            self.ctx.front_rectify_configure(rectify["src_wh"], rectify["dst_wh"], rectify["left"], rectify["right"])
        self.resize = resize is not None
        if self.resize:
            if not self.front:
                raise ValueError("resize needs the front mode (front=True or a list of filters)")
            self.ctx.front_resize_configure(resize["src_wh"], resize["dst_wh"])

    @property
    def ctx_reuse(self):
        if self._ctx_reuse is None:
            self._ctx_reuse = self.nrs.Context()
        return self._ctx_reuse

    # front mode: one nrs_front_process per frame.  The loop hands the SAME array to every step of a frame and starts each frame with
    # klt_track, which therefore always processes; the later steps process only when they see another array.  With resize the frame is
    # the raw one and the call is nrs_front_process_raw: what is resident afterwards, and the grey handed back, is the resized frame
    def _front_frame(self, im, force=False):
        if force or im is not self._front_im:
            process = self.ctx.front_process_raw if self.resize else self.ctx.front_process
            self._front_gray = process(im, outputs=("gray",))["gray"]
            self._front_im, self._front_right, self._front_fresh = im, None, None      # (a single frame invalidates the resident right eye)
            self.n_front_calls += 1
        return self._front_gray

    # front mode, stereo: one nrs_front_process_stereo per pair -- the same identity rule on (left, right).  Afterwards the left eye is the
    # resident frame of every step above (they see the same `left` array and do not process again) and both eyes are there for init_stereo /
    # stereo_pattern / stereo_lk.  force: the start of a frame (FrameLoop.track_image_with_stereo); the klt_track that follows on the same
    # left array then tracks on the resident eye instead of processing it a second time.  With rectify the eyes are the raw ones and the
    # call is nrs_front_process_stereo_raw: what is resident afterwards, and the grey handed back, is the rectified pair
    def front_stereo(self, left, right, force=False):
        if not self.front:
            raise ValueError("front_stereo needs the front mode (front=True or a list of filters)")
        if force or left is not self._front_im or right is not self._front_right:
            process = self.ctx.front_process_stereo_raw if self.rectify else self.ctx.front_process_stereo
            self._front_gray = process(left, right, outputs=("gray",))["gray"]
            self._front_im, self._front_right = left, right
            self.n_front_calls += 1
            if force:
                self._front_fresh = left

    # main tracker
    def klt_set_reference(self, im, pts):
        if self.front:
            self._front_frame(im)
            return self.ctx.klt_set_reference_front(pts, self.nrs.FRONT_GRAY, True)
        self.ctx.klt_set_reference(im, pts)

    def klt_track(self, im, pts, status, min_ssim):
        if self.front:
            if im is self._front_fresh:                            # this frame's pair has just been processed: its left eye is resident
                self._front_fresh = None
            else:
                self._front_frame(im, force=True)
            xy, st, good, _ = self.ctx.klt_track_front(pts, status, self.nrs.FRONT_GRAY, initial_flow=True, min_ssim=min_ssim)
            return xy, st
        xy, st, good, _ = self.ctx.klt_track(im, pts, status, initial_flow=True, min_ssim=min_ssim)
        return xy, st

    def klt_get_templates(self, n):
        return self.ctx.klt_get_templates(0, n)

    def klt_insert_template(self, t):
        self.ctx.klt_insert_template(t)

    def klt_insert_templates(self, ts):                  # (one call, one upload: PointReuse's new slots of a frame)
        self.ctx.klt_insert_templates(ts)

    # The map's photometric information stays on the device (include/nrs.h nrs_klt_archive_templates): archived by map point id at
    # keyframes, inserted from there when a point is reused.  (NRS_FRAME_LOOP_HOST_TEMPLATES=1: through the host, as before round 5.)
    def archive_templates(self, slots, mps):
        self.ctx.klt_archive_templates(slots, mps)

    def insert_archived(self, mps, xy):
        self.ctx.klt_insert_archived(self.ctx, mps, xy)

    # PointReuse in one call on the main context (include/nrs.h nrs_point_reuse): the image is the pyramid of this frame's klt_track
    def point_reuse(self, pose, wh, map_pos, frame_slot, slot_status, lost, min_ssim, insert_new=True):
        self.n_device_reuse += 1
        return self.ctx.point_reuse(self.cam, pose[0], pose[1], wh, map_pos, frame_slot, slot_status, lost, min_ssim, insert_new)

    def reuse_track_archived(self, im, pts, mps, min_ssim):
        o = self.klt_opts
        self.ctx_reuse.klt_clear()
        self.ctx_reuse.klt_configure(o["win"], 1, o["max_iters"], o["epsilon"], o["min_eig"])
        self.ctx_reuse.klt_insert_archived(self.ctx, mps, pts)
        if self.front:
            im = self._front_frame(im)
        xy, st, good, _ = self.ctx_reuse.klt_track(im, pts, np.zeros(len(pts), np.int32), initial_flow=True, min_ssim=min_ssim)
        return xy, st

    # the tracker PointReuse builds for its candidates (maxLevel 1, tracking.cc:422-424)
    def reuse_track(self, im, pts, templates, min_ssim):
        o = self.klt_opts
        self.ctx_reuse.klt_clear()
        self.ctx_reuse.klt_configure(o["win"], 1, o["max_iters"], o["epsilon"], o["min_eig"])
        self.ctx_reuse.klt_insert_templates([dict(t, xy=np.asarray(p, F32)) for p, t in zip(pts, templates)])
        if self.front:
            im = self._front_frame(im)
        xy, st, good, _ = self.ctx_reuse.klt_track(im, pts, np.zeros(len(pts), np.int32), initial_flow=True, min_ssim=min_ssim)
        return xy, st

    def extract_features(self, im, held_xy, mask=None):
        if self.front:
            self._front_frame(im)
            xy, ids, _ = self.ctx.shi_extract_front(held_xy, self.nrs.FRONT_GRAY, True)
            return xy, ids
        xy, ids, _ = self.ctx.shi_extract(im, held_xy, mask)
        return xy, ids

    def pose_only(self, uv, X, q, t):
        q2, t2, _ = self.ctx.pose_only_solve(self.cam, uv, X, q, t)
        return q2, t2

    # EssentialMatrixInitialization::Initialize (tracking.cc:161-165's call) on the device: include/nrs.h nrs_init_essential
    def init_essential(self, ref_xy, cur_xy, status, n_matches, **options):
        return self.ctx.init_essential(self.cam, ref_xy, cur_xy, status, n_matches, taps=False, **options)

    # MonocularMapInitializer::FeatureTracksClustering (monocular_map_initializer.cc:185-219) on the device: include/nrs.h
    # nrs_flow_tracks_cluster.  tracks: [n, length, 2] keypoints of the full-length tracks in ascending feature index -> labels [n]
    def flow_cluster(self, tracks):
        label, _, _ = self.ctx.flow_tracks_cluster(tracks, flows=False)
        return label

    # Tracking::StereoMapInitialization (tracking.cc:216-263) on the device: include/nrs.h nrs_init_stereo.  Without the front mode the images
    # are grey bytes from the host; in front mode they are the RAW frames, processed once as a pair (front_stereo) and matched where they
    # lie (nrs_init_stereo_front).  The result carries the selected keypoints for FrameLoop.from_stereo_initialization
    def init_stereo(self, left, right, kp, **options):
        kp = np.asarray(kp, F32).reshape(-1, 2)
        if self.front:
            self.front_stereo(left, right)
            r = self.ctx.init_stereo_front(self.cam, kp, self.nrs.FRONT_GRAY, **options)
        else:
            r = self.ctx.init_stereo(self.cam, left, right, kp, **options)
        r["selected_keypoints"] = kp[r["selected"]].copy()
        return r

    def dbscan3d(self, xyz, eps=2.5, min_points=5, noise_competes=True):
        return self.ctx.dbscan3d(xyz, eps, min_points, noise_competes)

    # dense_graph: the map's RegularizationGraph at the reference's density -- every pair of initial map points connected
    # (modules/map/map.cc:148-166) -- resident on the device; otherwise the caller's flat graph
    def make_graph(self, graph, X0):
        if not self.dense:
            return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in graph.items()}
        ids = np.arange(len(X0), dtype=np.int32)
        self.rg = self.nrs.RGraph(self.ctx, len(X0), graph["sigma"], graph["stretch_th"])
        self.rg.add_edges(np.asarray(X0, F32), ids, ids)
        if self.n_nodes > 0:                                       # the node set of the sequence: fixed map points
            nodes = self.ctx.skin_select_nodes(np.asarray(X0, F32), min(self.n_nodes, len(X0)), np.ones(len(X0), bool))
            self.node_flag = np.zeros(len(X0), np.uint8)
            self.node_flag[nodes] = 1
        return self.rg

    def track_deform(self, graph, map_pos, f_map, f_status, f_uv, f_pos, q, t, scale):
        self.last_trace = self.nrs.Trace(1024)
        if self.node_flag is not None:
            n = len(map_pos)                                       # (as below: a grown graph's capacity runs ahead of the map)
            r = self.ctx.track_deform_solve_embedded(self.cam, graph, map_pos if graph.cap == n else self._padded(map_pos), f_map, f_status, f_uv, f_pos,
                                                     self.node_flag[np.asarray(f_map)], q, t, scale, self.last_trace, max(self.cap, 128))
            r["map_pos"] = np.asarray(r["map_pos"])[:n]
            r["graph"] = graph
            return r
        if self.dense:
            n = len(map_pos)                                       # (a grown graph's capacity runs ahead of the map: rows beyond it have no edge)
            r = self.ctx.track_deform_solve_rg(self.cam, graph, map_pos if graph.cap == n else self._padded(map_pos), f_map, f_status, f_uv, f_pos, q, t,
                                               scale, self.last_trace, self.cap)
            r["map_pos"] = np.asarray(r["map_pos"])[:n]
            r["graph"] = graph                                     # updated in place on the device
            return r
        return self.ctx.track_deform_solve(self.cam, graph, map_pos, f_map, f_status, f_uv, f_pos, q, t, scale, self.last_trace)

    # ---- frame mapping (include/nrs.h "Frame mapping")
    def map_frame(self, tb, deform_mag, rad_per_pixel, rigidity_th=0.004, min_track=5):
        return self.ctx.map_frame(self.cam, tb, deform_mag, rad_per_pixel, rigidity_th, min_track, -1)

    # ---- the same on the resident TemporalBuffer (device_tbuf=True; include/nrs.h "The resident TemporalBuffer")
    def tbuf_reset(self, max_buffer_size=20):
        if self.tb is not None:
            self.tb.close()
        self.tb = self.nrs.TBuf(self.ctx, max_buffer_size)

    def tbuf_insert(self, kp_id, kp, pos, status, pose, deform_mag):
        self.tb.insert(kp_id, kp, pos, status, np.concatenate([pose[0], pose[1]]).astype(F32), deform_mag)

    def map_frame_resident(self, rad_per_pixel, rigidity_th=0.004, min_track=5):
        """map_frame's dict; `cand` and `accepted_ids` are keypoint ids"""
        return self.tb.map_frame(self.cam, rad_per_pixel, rigidity_th, min_track, -1)

    # ---- keyframe mapping: LocalDeformableBundleAdjustment on the resident graph (include/nrs.h nrs_dba_solve_window_rg; in the
    # embedded-deformation mode nrs_dba_solve_window_rg_embedded with the sequence's node set: lm_xyz is then per observation -- node
    # copies optimised, skinned observations at their skinned position, observations bound to no node unchanged)
    def dba_window(self, poses_qt, kf_points, lm_xyz, lm_uv, graph, scale, iters=5):
        if not self.dense:
            raise ValueError("keyframe BA needs the dense graph (dense_graph=True)")
        tr = self.nrs.Trace(256)
        if self.node_flag is not None:
            pq, xyz = self.ctx.dba_solve_window_rg_embedded(self.cam, poses_qt, kf_points, lm_xyz, lm_uv, graph, self._node_flag_at(graph.cap), scale, iters, tr, self.cap)
            e = self.ctx.dba_window_edges_embedded()
            return dict(poses_qt=pq, lm_xyz=xyz, n_spring=len(e["sp_d0"]), n_damper=len(e["dm_w"]), trials=len(tr.trials))
        pq, xyz = self.ctx.dba_solve_window_rg(self.cam, poses_qt, kf_points, lm_xyz, lm_uv, graph, scale, iters, tr, self.cap)
        ns, nd = self.ctx.dba_window_edge_counts()
        return dict(poses_qt=pq, lm_xyz=xyz, n_spring=ns, n_damper=nd, trials=len(tr.trials))

    def _padded(self, map_pos):
        """positions by point index for the dense graph: capacity rows (the graph grows in doubled steps, the map one point at a time)"""
        pos = np.zeros((self.rg.cap, 3), F32)
        pos[:len(map_pos)] = map_pos
        return pos

    def _node_flag_at(self, cap):
        """the node flags by graph index, extended with zeros to `cap` entries"""
        if len(self.node_flag) >= cap:
            return self.node_flag
        return np.concatenate([self.node_flag, np.zeros(cap - len(self.node_flag), np.uint8)])

    def grow_graph(self, graph, map_pos, new_ids, other_ids):
        """mapping.cc:238-256 on the dense graph, resized in amortised steps (doubled, not +1) to hold len(map_pos) points"""
        if not self.dense:
            raise ValueError("mapping needs the dense graph (dense_graph=True)")
        if len(map_pos) > self.rg.cap:
            self.rg.resize(max(len(map_pos), 2 * self.rg.cap))
        if self.node_flag is not None:                             # the node set stays the one of the initial map: new map points are skinned
            self.node_flag = self._node_flag_at(self.rg.cap)
        self.rg.grow(self._padded(map_pos), new_ids, other_ids)
        return self.rg

    # ---- evaluation (include/nrs.h "f7: evaluation"): FrameEvaluator::EvaluateFrameReconstruction and its sources of ground truth
    def eval_frame(self, q, t, X, kp, depth=None, gt_xyz=None, gt_status=None):
        return self.ctx.eval_frame(self.cam, q, t, X, kp, depth=depth, gt_xyz=gt_xyz, gt_status=gt_status)

    # (front mode: left / right are the raw frames; the pair is processed once -- front_stereo -- and matched where it lies)
    def stereo_pattern(self, left, right, kp, bf):
        if self.front:
            self.front_stereo(left, right)
            xyz, st, _, _ = self.ctx.stereo_match_pattern_front(self.cam, bf, kp, self.nrs.FRONT_GRAY)
            return xyz, st
        xyz, st, _, _ = self.ctx.stereo_match_pattern(self.cam, bf, left, right, kp)
        return xyz, st

    # the reference's LK stereo matcher owns its tracker (SLAM/system.cc:45-54): a third context, made on first use, so that the
    # tracking templates of self.ctx are left alone.  In front mode it reads the pair resident in self.ctx (nrs_stereo_match_lk_front)
    def stereo_lk(self, left, right, kp, bf, min_ssim=0.5):
        if getattr(self, "ctx_stereo", None) is None:
            o = self.klt_opts
            self.ctx_stereo = self.nrs.Context()
            self.ctx_stereo.klt_configure(o["win"], o["max_level"], o["max_iters"], o["epsilon"], o["min_eig"])
        if self.front:
            self.front_stereo(left, right)
            xyz, st, _, _ = self.nrs.stereo_lk_front(self.ctx_stereo, self.ctx, self.cam, bf, kp, min_ssim, self.nrs.FRONT_GRAY)
            return xyz, st
        xyz, st, _, _ = self.nrs.stereo_lk(self.ctx_stereo, self.cam, bf, left, right, kp, min_ssim)
        return xyz, st

    def close(self):
        if self.rg is not None:
            self.rg.close()
        if self.tb is not None:
            self.tb.close()
        if getattr(self, "ctx_stereo", None) is not None:
            self.ctx_stereo.close()
        self.ctx.close()
        if self._ctx_reuse is not None:
            self._ctx_reuse.close()


class MonoInitializer:
    """MonocularMapInitializer (modules/tracking/monocular_map_initializer.cc:52-307) on flat arrays over a backend: ProcessNewImage /
    DataAssociation / ResetInitialization / AddFeatureTracks / RigidInitialization / InitializationRefinement.  A feature's id is its index in
    the arrays of the current reference (they are never reordered between two resets), so a feature track is its first keypoint, its last one
    and its length.  n_tracks_in_image_ is taken as the
    number of TRACKED statuses after the tracker's call -- what LucasKanadeTracker::Track returns.  max_features thins the extractor's list
    evenly, mask is handed to the extractor's filter (ExtractFeatures, :135-153).

    cluster_tracks=True adds FeatureTracksClustering (:185-219): AddFeatureTracks then keeps the keypoints of every image since the reset (a
    keypoint is appended only where the status is TRACKED), and every image that is not a reset hands the tracks of the maximal length, in
    ascending feature index (the reference: the order of a hash map), to backend.flow_cluster.  The log entry gains `full_tracks` (their
    indices) and `feature_labels`, a successful result `track_labels`, aligned with `index` -- a track's label is its own, where
    InitializationRefinement (:260) indexes the labels, which are in full-length-track order, by keypoint.  Off (the default) nothing of
    this runs and the log is what it was."""
    NO_DATA, RECENTLY_RESET, OK = 0, 1, 2

    def __init__(self, backend, klt_min_ssim=0.5, min_tracks=100, max_images=30, max_features=None, cluster_tracks=False, **init_options):
        self.b, self.min_ssim, self.min_tracks, self.max_images, self.max_features = backend, klt_min_ssim, min_tracks, max_images, max_features
        self.cluster_tracks = bool(cluster_tracks)
        self.history = []                                        # cluster_tracks: (keypoints, TRACKED mask) of every image since the reset
        self.init_options = init_options
        self.state = self.NO_DATA
        self.kp = self.ref_kp = np.zeros((0, 2), F32)
        self.status = np.zeros(0, np.int32)
        self.track_len = np.zeros(0, np.int32)
        self.max_len, self.images, self.n_tracks = 0, 0, 0
        self.log = []

    def reset(self, im, mask=None):                              # ResetInitialization (:80-103)
        xy, _ = self.b.extract_features(im, None, mask)
        xy = np.asarray(xy, F32).reshape(-1, 2)
        if self.max_features is not None and len(xy) > self.max_features:          # evenly over the extractor's (row-major) order
            xy = xy[(np.arange(self.max_features) * len(xy)) // self.max_features]
        self.kp, self.ref_kp = xy.copy(), xy.copy()
        self.b.klt_set_reference(im, self.kp)
        self.status = np.full(len(xy), TRACKED, np.int32)
        self.track_len = np.zeros(len(xy), np.int32)
        self.max_len, self.images = 0, 0
        self.history = []
        self.state = self.RECENTLY_RESET

    def data_association(self, im, mask=None):                   # (:105-133)
        if self.state == self.NO_DATA:
            self.reset(im, mask)
        else:
            self.kp, self.status = self.b.klt_track(im, self.kp, self.status, self.min_ssim)
            self.kp, self.status = np.asarray(self.kp, F32), np.asarray(self.status, np.int32)
            self.n_tracks = int((self.status == TRACKED).sum())
            if self.n_tracks < self.min_tracks:
                self.reset(im, mask)
            else:
                self.images += 1
                self.state = self.OK
                if self.images > self.max_images:
                    self.reset(im, mask)
        self.track_len[self.status == TRACKED] += 1              # AddFeatureTracks (:155-166)
        self.max_len += 1
        if self.cluster_tracks:
            self.history.append((self.kp.copy(), self.status == TRACKED))

    def feature_tracks_clustering(self):
        """FeatureTracksClustering (:185-219) -> (full_tracks: indices of the tracks of the maximal length, ascending; feature_labels)"""
        full = np.nonzero(self.track_len == self.max_len)[0].astype(np.int32)
        if len(full) == 0:
            return full, np.zeros(0, np.int32)
        tracks = np.stack([kp[full] for kp, _ in self.history], axis=1).astype(F32)       # [n, length, 2]; every mask is set on these rows
        return full, np.asarray(self.b.flow_cluster(tracks), np.int32)

    def process_new_image(self, im, mask=None):
        """ProcessNewImage (:52-78): None ("Just reset" / "Rigid Initialization failed") or the InitializationResults as a dict"""
        self.data_association(im, mask)
        entry = dict(reset=self.state == self.RECENTLY_RESET, n_features=len(self.kp), n_tracks=self.n_tracks, verdict=None)
        self.log.append(entry)
        if self.state == self.RECENTLY_RESET:
            return None
        if self.cluster_tracks:
            full, labels = self.feature_tracks_clustering()
            entry.update(full_tracks=full, feature_labels=labels)
        entry.update(ref_xy=self.ref_kp.copy(), cur_xy=self.kp.copy(), status=self.status.copy())
        r = self.b.init_essential(self.ref_kp, self.kp, self.status, self.n_tracks, **self.init_options)
        entry["verdict"] = int(r["verdict"])
        if r["verdict"] != 0:
            return None
        # InitializationRefinement + BuildInitializationResults (:235-307): triangulated landmarks whose track has the maximal length
        keep = np.nonzero((np.asarray(r["code"]) == 0) & (self.track_len == self.max_len))[0]
        xyz = np.asarray(r["xyz"], F32)[keep]
        res = dict(index=keep, reference_keypoints=self.ref_kp[keep].copy(), current_keypoints=self.kp[keep].copy(),
                   reference_landmark_positions=xyz.copy(), current_landmark_positions=xyz.copy(),
                   pose_q=np.asarray(r["pose_q"], F32), pose_t=np.asarray(r["pose_t"], F32))
        if self.cluster_tracks:                                  # keep is a subset of the full-length tracks
            res["track_labels"] = labels[np.searchsorted(full, keep)].copy()
        entry["n_map_points"] = len(keep)
        return res


def sigma_f32(data):
    """Sigma (modules/utilities/statistics_toolbox.cc:25-50): fp32, sequential"""
    acc = F32(0)
    for v in data:
        acc = F32(acc + F32(v))
    mu = F32(acc / F32(len(data)))
    acc = F32(0)
    for v in data:
        d = F32(F32(v) - mu)
        acc = F32(acc + F32(d * d))
    return F32(np.sqrt(F32(acc / F32(len(data)))))


class TemporalBuffer:
    """TemporalBuffer (modules/map/temporal_buffer.cc:28-56) as a list of snapshots, and its flat form for nrs_map_frame.  The reference
    pops the oldest snapshot when size() > max_buffer_size BEFORE it inserts: from 20 it goes to 21 without a pop, from 21 to 20 and back to
    21 -- never more than max + 1 = 21 snapshots, the limit of the flat interface."""

    def __init__(self, max_buffer_size=20):
        self.max, self.snaps = max_buffer_size, []

    def insert(self, kp_id, kp_xy, pos, status, pose_q, pose_t, deform_mag):
        keep = (status == TRACKED_WITH_3D) | (status == TRACKED)   # InsertSnapshotFromFrame: GetKeypointsWithStatus({TRACKED_WITH_3D, TRACKED})
        snap = dict(ids=np.asarray(kp_id, np.int64)[keep], xy=np.asarray(kp_xy, F32)[keep], pos=np.asarray(pos, F32)[keep],
                    status=np.asarray(status, np.int32)[keep], pose=np.concatenate([pose_q, pose_t]).astype(F32), mag=F32(deform_mag))
        if len(self.snaps) > self.max:
            self.snaps.pop(0)
        self.snaps.append(snap)

    def flat(self, model, prm):
        """(tb, deform_mag, ids): the dict nrs.Context.map_frame reads over the keypoint ids the buffer holds, ascending (row j = ids[j])"""
        ids = np.unique(np.concatenate([s["ids"] for s in self.snaps]))
        F, n = len(self.snaps), len(ids)
        tb = dict(n_frames=F, poses=np.array([s["pose"] for s in self.snaps], F32), has_kp=np.zeros((F, n), bool), kp_xy=np.zeros((F, n, 2), F32),
                  has_lm=np.zeros((F, n), bool), lm_xyz=np.zeros((F, n, 3), F32), status=np.full(n, BAD, np.int32), model=model, prm=prm)
        for f, s in enumerate(self.snaps):
            j = np.searchsorted(ids, s["ids"])
            tb["has_kp"][f, j] = True
            tb["kp_xy"][f, j] = s["xy"]
            tb["has_lm"][f, j] = True                              # mapppoint_tracks_ holds every keypoint of a snapshot (:41), zeros for TRACKED
            tb["lm_xyz"][f, j] = s["pos"]
        tb["status"][np.searchsorted(ids, self.snaps[-1]["ids"])] = self.snaps[-1]["status"]
        return tb, np.array([s["mag"] for s in self.snaps], F32), ids


class KeyFrame:
    """KeyFrame(Frame&) (modules/map/keyframe.cc:26-55) on flat arrays: the TRACKED_WITH_3D slots of the frame, then the TRACKED ones (position
    zero, no map point); everything else stays behind.  kp_id is carried along so that Frame::SetFromKeyFrame gives the slots their ids back."""

    def __init__(self, kf_id, kp, pos, status, map_index, kp_id, pose):
        status = np.asarray(status, np.int32)
        order = np.concatenate([np.nonzero(status == TRACKED_WITH_3D)[0], np.nonzero(status == TRACKED)[0]])
        self.id = int(kf_id)
        self.kp, self.pos = np.asarray(kp, F32)[order].copy(), np.asarray(pos, F32)[order].copy()
        self.status, self.map_index = status[order].copy(), np.asarray(map_index, np.int32)[order].copy()
        self.kp_id = np.asarray(kp_id, np.int64)[order].copy()
        self.pos[self.status == TRACKED] = 0
        self.map_index[self.status == TRACKED] = -1
        self.pose = (np.asarray(pose[0], F32).copy(), np.asarray(pose[1], F32).copy())


class UnmappedQueue:
    """Map::unmapped_keyframes_ as the reference handles it: InsertKeyFrame pushes the id at the back (map.cc:42),
    GetNextUnmappedKeyFrame returns the keyframe at the FRONT and pops the BACK (map.cc:62-72).  With one id queued the two are the same
    keyframe; with more, the oldest is handed out again and again while the newer ones are dropped unmapped.  Reproduced, not repaired."""

    def __init__(self):
        self.ids = []

    def push(self, kf_id):
        self.ids.append(int(kf_id))

    def next(self):
        if not self.ids:
            return None
        front = self.ids[0]
        self.ids.pop()
        return front


class FrameLoop:
    """State of Tracking + the slice of Map / Frame it touches, on flat arrays."""

    def __init__(self, backend, project_f32, wh, scale, kp0, X0, graph, pose_q, pose_t, im0,
                 klt_min_ssim=0.7, images_to_insert_keyframe=5, extract_on_keyframes=True, mapping=False, rad_per_pixel=None, rigidity_th=0.004,
                 camera=None, max_buffer_size=20, keyframe_ba=False):
        """mapping=True (needs a dense-graph backend, rad_per_pixel = Mapping::Options::rad_per_pixel and camera = (model, params) for the
        flat temporal buffer): the FrameMapping branch of Mapping::DoMapping after every tracked frame, see the module's header.
        keyframe_ba=True (needs mapping=True and a backend with dba_window): the KeyFrameMapping branch as well."""
        self.b, self.project, self.wh, self.scale = backend, project_f32, wh, float(scale)
        n = len(kp0)
        self.mapping = bool(mapping)
        self.keyframe_ba = bool(keyframe_ba)
        if self.keyframe_ba and not self.mapping:
            raise ValueError("keyframe_ba=True needs mapping=True")
        if self.keyframe_ba and not hasattr(backend, "dba_window"):
            raise ValueError("keyframe_ba=True needs a backend with dba_window")
        if self.mapping:
            if not getattr(backend, "dense", False):
                raise ValueError("mapping=True needs a backend that keeps the all-pairs graph (dense_graph=True)")
            if rad_per_pixel is None or camera is None:
                raise ValueError("mapping=True needs rad_per_pixel and camera=(model, params)")
            self.rpp, self.rigidity_th, self.camera = float(rad_per_pixel), float(rigidity_th), camera
            # Keypoint::class_id (a persistent id per slot), the TemporalBuffer and Map::unmapped_keyframes_: the initialisation leaves two
            # keyframes unmapped (tracking.cc:194-195) and its own DoMapping call takes one (map.cc:62-72), so one is left for the first frame
            self.kp_id = np.arange(n, dtype=np.int64)
            self.next_kp_id = n
            self.dev_tbuf = bool(getattr(backend, "device_tbuf", False))     # the backend holds the buffer on the device
            if self.dev_tbuf:
                self.tbuf = None
                backend.tbuf_reset(max_buffer_size)
            else:
                self.tbuf = TemporalBuffer(max_buffer_size)
            self.unmapped_keyframes = 1
            self.deform_median = 0.0
        # current frame: slot i observes map point map_index[i]
        self.kp = np.asarray(kp0, F32).copy()
        self.pos = np.asarray(X0, F32).copy()
        self.status = np.zeros(n, np.int32)
        self.map_index = np.arange(n, dtype=np.int32)
        # map
        self.map_pos = np.asarray(X0, F32).copy()                  # MapPoint::GetLastWorldPosition
        # the caller's flat graph, or (a backend that keeps one) the all-pairs graph of the map
        self.graph = backend.make_graph(graph, X0) if hasattr(backend, "make_graph") else \
            {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in graph.items()}
        self.pose = (np.asarray(pose_q, F32), np.asarray(pose_t, F32))
        self.last_pose = self.pose
        self.motion = (np.array([0, 0, 0, 1], F32), np.zeros(3, F32))
        self.min_ssim, self.kf_every, self.since_kf = klt_min_ssim, images_to_insert_keyframe, 0
        self.extract = extract_on_keyframes
        # initial keyframe: klt reference + photometric information of every map point (tracking.cc:201-209)
        self.b.klt_set_reference(im0, self.kp)
        import os
        self.dev_templates = hasattr(self.b, "archive_templates") and not os.environ.get("NRS_FRAME_LOOP_HOST_TEMPLATES")
        if self.dev_templates:
            self.templates = None
            self.b.archive_templates(np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32))
        else:
            self.templates = self.b.klt_get_templates(n)
        if self.keyframe_ba:
            # Map::keyframes_ and Map::unmapped_keyframes_.  The initial keyframe is queued: one unmapped keyframe is left for the first
            # frame, as `unmapped_keyframes = 1` above has it, so both settings take the KeyFrameMapping branch on the same frames
            self.keyframes, self.next_kf_id, self.unmapped = {}, 0, UnmappedQueue()
            self.insert_keyframe()
        self.log = []

    @classmethod
    def from_initialization(cls, backend, project_f32, wh, result, im, stretch_th=1.1, **kw):
        """The tail of Tracking::MonocularMapInitialization (tracking.cc:147-213) on a MonoInitializer result: scale = 3 / the nth_element
        median of the landmark depths, Sigma of the depths, positions and the pose translation times scale, the all-pairs graph at
        3 sigma scale (the backend keeps it: a dense-graph backend is required), klt_set_reference on the current image and the template
        archive (both in __init__).  The loop starts at the current frame, every map point TRACKED_WITH_3D."""
        if not getattr(backend, "dense", False):
            raise ValueError("from_initialization needs a backend that keeps the all-pairs graph (dense_graph=True)")
        X = np.asarray(result["current_landmark_positions"], F32)
        depths = X[:, 2].astype(F32)
        k = len(depths) // 2
        scale = F32(F32(3) / np.partition(depths, k)[k])
        sigma = sigma_f32(depths)
        sigma_graph = F32(F32(sigma * scale) * F32(3))
        Xs = (np.asarray(result["reference_landmark_positions"], F32) * scale).astype(F32)
        t = (np.asarray(result["pose_t"], F32) * scale).astype(F32)
        loop = cls(backend, project_f32, wh, scale, result["current_keypoints"], Xs, dict(sigma=float(sigma_graph), stretch_th=stretch_th),
                   result["pose_q"], t, im, **kw)
        loop.pos = (X * scale).astype(F32)
        loop.init_sigma, loop.init_sigma_graph = sigma, sigma_graph
        if loop.keyframe_ba:
            # tracking.cc:190-195: BOTH frames become keyframes -- the reference frame (its keypoints, the reference positions, the identity
            # pose) and the current one -- and both are queued; the initialisation's own DoMapping (SLAM/system.cc:128) then takes the
            # front and pops the back, which leaves the reference keyframe for the loop's first frame.  (That call's BA has two keyframes
            # and returns at OPT:922; its SetFromKeyFrame is not restated: the loop starts from the current frame, as without keyframe_ba.)
            loop.keyframes, loop.next_kf_id, loop.unmapped = {}, 0, UnmappedQueue()
            loop.insert_keyframe(kp=np.asarray(result["reference_keypoints"], F32), pos=Xs,
                                 pose=(np.array([0, 0, 0, 1], F32), np.zeros(3, F32)))
            loop.insert_keyframe()
            loop.unmapped.next()
        return loop

    @classmethod
    def from_stereo_initialization(cls, backend, project_f32, wh, result, im_left, sigma=10.5, stretch_th=1.1, **kw):
        """The tail of Tracking::StereoMapInitialization (tracking.cc:252-288) on a backend's init_stereo result: identity pose, scale 1 (the
        map is metric), the selected keypoints and positions, every one TRACKED_WITH_3D, the all-pairs graph at sigma = 10.5 (:268; the
        backend keeps it: a dense-graph backend is required), klt_set_reference on the left image and the template archive (both in
        __init__).  The reference makes ONE keyframe (:283-286) and System::TrackImageWithStereo's own DoMapping (SLAM/system.cc:150)
        takes it from the unmapped queue (a one-keyframe BA returns at once), so the loop's first frame finds no unmapped keyframe and
        takes the FrameMapping branch -- the mono start's first frame takes KeyFrameMapping."""
        if not getattr(backend, "dense", False):
            raise ValueError("from_stereo_initialization needs a backend that keeps the all-pairs graph (dense_graph=True)")
        if int(result["verdict"]) != 0 or int(result["n_selected"]) == 0:
            raise ValueError("from_stereo_initialization: the initialisation selected no point (verdict %d)" % int(result["verdict"]))
        kp, X = np.asarray(result["selected_keypoints"], F32).reshape(-1, 2), np.asarray(result["selected_xyz"], F32).reshape(-1, 3)
        loop = cls(backend, project_f32, wh, 1.0, kp, X, dict(sigma=float(sigma), stretch_th=stretch_th),
                   np.array([0, 0, 0, 1], F32), np.zeros(3, F32), im_left, **kw)
        loop.status[:] = TRACKED_WITH_3D
        loop.init_median_depth = F32(result["median_depth"])
        if loop.mapping:
            loop.unmapped_keyframes = 0
        if loop.keyframe_ba:
            # __init__ has made and queued the one keyframe (an identity-pose copy of this frame); the initialisation's own DoMapping takes it
            loop.unmapped.next()
        return loop

    # ---- KeyFrame(frame) + Map::InsertKeyFrame (keyframe.cc:26-55, map.cc:37-45); kp / pos / pose: another frame's, slot for slot
    def insert_keyframe(self, kp=None, pos=None, pose=None):
        kf = KeyFrame(self.next_kf_id, self.kp if kp is None else kp, self.pos if pos is None else pos, self.status, self.map_index, self.kp_id,
                      self.pose if pose is None else pose)
        self.next_kf_id += 1
        self.keyframes[kf.id] = kf
        self.unmapped.push(kf.id)
        return kf

    # ---- tracking.cc:72-112 (tracked branch)
    def track_image(self, im):
        if self.mapping:
            self.update_triangulated_points()                      # tracking.cc:87
        lost = self.track_camera_and_deformation(im)
        reused = self.point_reuse(im, lost)
        n3d = int((self.status == TRACKED_WITH_3D).sum())
        kf = False
        if n3d >= 10:
            kf = self.keyframe_insertion(im)
            self.last_pose = self.pose
        self.log.append(dict(pose_q=self.pose[0].copy(), pose_t=self.pose[1].copy(), lost=sorted(int(x) for x in lost),
                             reused=reused, n_tracked=n3d, keyframe=kf, n_2d=int((self.status == TRACKED).sum()),
                             kp_2d=self.kp[self.map_index < 0].copy(),
                             status_by_map=self._status_by_map(), pos_by_map=self._pos_by_map()))
        if self.mapping and n3d >= 10:
            # Map::SetLastFrame (tracking.cc:105, map.cc:106-118), then System::TrackImage's DoMapping (SLAM/system.cc:128)
            if self.dev_tbuf:
                self.b.tbuf_insert(self.kp_id, self.kp, self.pos, self.status, self.pose, self.deform_median)
            else:
                self.tbuf.insert(self.kp_id, self.kp, self.pos, self.status, self.pose[0], self.pose[1], self.deform_median)
            self.log[-1]["mapping"] = self.do_mapping(kf)
            self.log[-1]["map_size"] = len(self.map_pos)
            self.log[-1]["status_after_mapping"] = self._status_by_map()
        return n3d >= 10

    # ---- System::TrackImageWithStereo (SLAM/system.cc:134-160): ImageProcessing on both images (:137-138), the masks from the left one
    # (:144), TrackImage and DoMapping on the left (:146-150) and -- compiled out in the reference by `if (false && ...)` at :153, so off by
    # default here -- the evaluation against the stereo matcher.  Needs a front-mode backend: the pair is processed in ONE call, the tracker's
    # klt_track of this frame runs on the resident left eye, and evaluate() matches the resident pair.
    def track_image_with_stereo(self, left, right, evaluate=False, matcher="pattern", bf=1.0):
        if not getattr(self.b, "front", False) or not hasattr(self.b, "front_stereo"):
            raise ValueError("track_image_with_stereo needs a front-mode backend (GpuBackend(front=...))")
        self.b.front_stereo(left, right, force=True)
        self.stereo_pair = (left, right)
        ok = self.track_image(left)
        if evaluate:
            self.evaluate(right=right, matcher=matcher, left=left, bf=bf)
        return ok

    # ---- Mapping::DoMapping (mapping.cc:36-54) without the BA: a pending keyframe takes the KeyFrameMapping branch, which is skipped
    def do_mapping(self, keyframe_inserted):
        if self.keyframe_ba:                                       # (keyframe_insertion has queued the new keyframe)
            kf_id = self.unmapped.next()                           # Map::GetNextUnmappedKeyFrame
            if kf_id is None:
                return self.frame_mapping()
            ba = self.keyframe_mapping()
            self.set_from_keyframe(self.keyframes[kf_id])
            return dict(skipped=None, ba=ba, set_from=kf_id, triangulated=[], mode=None)
        if keyframe_inserted:
            self.unmapped_keyframes += 1
        if self.unmapped_keyframes > 0:
            self.unmapped_keyframes -= 1
            return dict(skipped="KeyFrameMapping", triangulated=[], mode=None)
        return self.frame_mapping()

    # ---- Mapping::KeyFrameMapping = LocalDeformableBundleAdjustment (mapping.cc:56-58, OPT:892-1161) on the backend's one call
    def keyframe_mapping(self):
        ids = sorted(self.keyframes)[-5:]                          # the five largest ids (OPT:894-920), flattened oldest first (OPT:930)
        if len(ids) < 3:
            return None                                            # OPT:922-924
        kfs = [self.keyframes[i] for i in ids]
        m3 = [kf.status == TRACKED_WITH_3D for kf in kfs]          # in keyframe index order (GetMapPointsIdsWithStatus)
        kf_points = [kf.map_index[m].astype(np.int32) for kf, m in zip(kfs, m3)]
        lm_xyz = np.concatenate([kf.pos[m] for kf, m in zip(kfs, m3)]).astype(F32)
        lm_uv = np.concatenate([kf.kp[m] for kf, m in zip(kfs, m3)]).astype(F32)
        poses_qt = np.array([np.concatenate([kf.pose[0], kf.pose[1]]) for kf in kfs], np.float64)
        r = self.b.dba_window(poses_qt, kf_points, lm_xyz, lm_uv, self.graph, self.scale, 5)
        # OPT:1146-1160, over inserted_landmarks: the keyframes that contributed a landmark get their pose (fp64 unit quaternion and
        # translation, each cast to fp32) and KeyFrame::LandmarkPositions() of those slots back.  The map points' own positions are
        # not written (map_pos stays).
        pq, xyz = np.asarray(r["poses_qt"], np.float64).reshape(-1, 7), np.asarray(r["lm_xyz"]).reshape(-1, 3)
        at = 0
        for k, (kf, m) in enumerate(zip(kfs, m3)):
            n = int(m.sum())
            if n:
                kf.pose = (pq[k, :4].astype(F32), pq[k, 4:].astype(F32))
                kf.pos[m] = xyz[at:at + n].astype(F32)
            at += n
        return dict(n_kf=len(kfs), n_lm=at, n_spring=int(r["n_spring"]), n_damper=int(r["n_damper"]), trials=int(r["trials"]))

    # ---- Mapping::UpdateTrackingFrameFromKeyFrame -> Frame::SetFromKeyFrame (mapping.cc:266-270, frame.cc:47-77).  last_frame_ and
    # current_frame_ are one object in the reference, so the motion model's "last pose" is the keyframe's as well.  The keyframe may be
    # older than the frame (UnmappedQueue): reproduced, not repaired.
    def set_from_keyframe(self, kf):
        order = np.concatenate([np.nonzero(kf.status == TRACKED_WITH_3D)[0], np.nonzero(kf.status == TRACKED)[0]])
        self.kp, self.pos, self.status = kf.kp[order].copy(), kf.pos[order].copy(), kf.status[order].copy()
        self.map_index, self.kp_id = kf.map_index[order].copy(), kf.kp_id[order].copy()
        self.pos[self.status == TRACKED] = 0
        self.pose = (kf.pose[0].copy(), kf.pose[1].copy())
        self.last_pose = self.pose

    # ---- Mapping::LandmarkTriangulation (mapping.cc:65-257) on the backend's one call
    def frame_mapping(self):
        if self.dev_tbuf:
            r = self.b.map_frame_resident(self.rpp, self.rigidity_th, 5)
            acc = np.asarray(r["accepted_ids"], np.int64)          # keypoint ids already: the device translated the rows
        else:
            tb, mag, ids = self.tbuf.flat(self.camera[0], self.camera[1])
            r = self.b.map_frame(tb, mag, self.rpp, self.rigidity_th, 5)
            acc = ids[np.asarray(r["accepted_ids"], np.int64)]     # keypoint ids, ascending (the order of the candidates)
        out = dict(skipped=None, triangulated=[int(i) for i in acc], mode=int(r["mode"]), n_rigid=int(r["n_rigid"]),
                   n_deformable=int(r["n_deformable"]), n_candidates=len(r["cand"]))
        if not len(acc):
            return out
        slot_of = {int(k): i for i, k in enumerate(self.kp_id)}
        slots = np.array([slot_of[int(k)] for k in acc])
        n0 = len(self.map_pos)
        new_mp = np.arange(n0, n0 + len(acc), dtype=np.int32)      # Map::CreateAndInsertMapPoint: the next map point ids
        xyz = np.asarray(r["accepted_xyz"], F32)
        self.pos[slots], self.status[slots], self.map_index[slots] = xyz, JUST_TRIANGULATED, new_mp     # Frame::AddGeometryToKeypoint
        self.map_pos = np.vstack([self.map_pos, xyz]).astype(F32)
        # :238-256: every new landmark against the frame's map points with a position, the new ones included
        has = ((self.status == TRACKED_WITH_3D) | (self.status == JUST_TRIANGULATED)) & (self.map_index >= 0)
        self.graph = self.b.grow_graph(self.graph, self.map_pos, new_mp, self.map_index[has].astype(np.int32))
        return out

    # ---- Tracking::UpdateTriangulatedPoints (tracking.cc:508-521)
    def update_triangulated_points(self):
        slots = np.nonzero(self.status == JUST_TRIANGULATED)[0].astype(np.int32)
        if not len(slots):
            return
        if self.dev_templates:
            self.b.archive_templates(slots, self.map_index[slots].astype(np.int32))
        else:
            tpl = self.b.klt_get_templates(len(self.map_index))
            self.templates = list(self.templates) + [None] * (len(self.map_pos) - len(self.templates))
            for i in slots:
                self.templates[int(self.map_index[i])] = tpl[int(i)]
        self.status[slots] = TRACKED_WITH_3D

    # ---- FrameEvaluator::EvaluateFrameReconstruction (frame_evaluator.cc:35-52), called after track_image as System::TrackImageWithDepth
    # does (SLAM/system.cc:162-187)
    def evaluate(self, depth=None, right=None, matcher="pattern", left=None, bf=1.0):
        """Scores the current frame: the TRACKED_WITH_3D slots against a depth image (fp32, h x w) or against a stereo matcher run on
        (left, right) grey images -- matcher "pattern" (StereoPatternMatching) or "lk" (StereoLucasKanade); bf is the matcher's baseline_.
        Appends dict(rmse, scale, counts, n, rc) to self.rmse and returns it (rmse NaN, rc -1: too few points with ground truth); the
        world-frame ground truth of the evaluated slots is kept in self.ground_truth (slot indices in self.ground_truth_slots).
        With a front-mode backend left / right are the RAW frames and the matcher runs on the resident pair (processed once; nothing is
        processed when they are the arrays track_image_with_stereo has just been given); left may then be left out after
        track_image_with_stereo: it is that call's left frame."""
        if not hasattr(self, "rmse"):
            self.rmse = []
        if left is None and right is not None and getattr(self.b, "front", False) and getattr(self, "stereo_pair", None) is not None:
            left = self.stereo_pair[0]
        slots = np.nonzero(self.status == TRACKED_WITH_3D)[0]
        kp, X = self.kp[slots], self.pos[slots]
        if depth is not None:
            r = self.b.eval_frame(self.pose[0], self.pose[1], X, kp, depth=depth)
        else:
            if right is None or left is None:
                raise ValueError("evaluate: a depth image, or the left and right images of a stereo pair")
            if matcher not in ("pattern", "lk"):
                raise ValueError("evaluate: matcher %r" % (matcher,))
            gt, st = (self.b.stereo_pattern if matcher == "pattern" else self.b.stereo_lk)(left, right, kp, bf)
            r = self.b.eval_frame(self.pose[0], self.pose[1], X, kp, gt_xyz=gt, gt_status=st)
        self.ground_truth, self.ground_truth_slots = r["gt_world"], slots
        rec = dict(rmse=r["rmse"], scale=r["scale"], counts=r["counts"], n=len(slots), rc=r["rc"])
        self.rmse.append(rec)
        return rec

    def _status_by_map(self):
        s = np.full(len(self.map_pos), -1, np.int32)
        m = self.map_index >= 0                                    # slots without a map point: extracted 2D features
        s[self.map_index[m]] = self.status[m]
        return s

    def _pos_by_map(self):
        p = np.zeros((len(self.map_pos), 3), F32)
        m = self.map_index >= 0
        p[self.map_index[m]] = self.pos[m]
        return p

    # ---- tracking.cc:291-333
    def track_camera_and_deformation(self, im):
        self.kp, self.status = self.b.klt_track(im, self.kp, self.status, self.min_ssim)
        self.pose = se3f_mul(self.motion, self.pose)               # motion-model seed
        m = self.status == TRACKED_WITH_3D
        q, t = self.b.pose_only(self.kp[m], self.pos[m], self.pose[0].astype(np.float64), self.pose[1].astype(np.float64))
        self.pose = (np.asarray(q, np.float64).astype(F32), np.asarray(t, np.float64).astype(F32))
        mm = self.map_index >= 0                                   # the optimisation walks Frame::IndexToMapPointId (OPT:212-236)
        r = self.b.track_deform(self.graph, self.map_pos, self.map_index[mm], self.status[mm], self.kp[mm], self.pos[mm],
                                self.pose[0].astype(np.float64), self.pose[1].astype(np.float64), self.scale)
        self.pose = (np.asarray(r["pose_q"], np.float64).astype(F32), np.asarray(r["pose_t"], np.float64).astype(F32))
        self.pos[mm], self.status[mm] = np.asarray(r["f_pos"], F32), np.asarray(r["f_status"], np.int32)
        self.map_pos, self.graph = np.asarray(r["map_pos"], F32), r["graph"]
        self.deform_median = float(r.get("median", 0.0)) if hasattr(r, "get") else 0.0      # Frame::SetDeformationMaginitud (OPT:455)
        self.motion = se3f_mul(self.pose, se3f_inv(self.last_pose))
        return set(int(x) for x in r["lost"])

    # ---- tracking.cc:394-506
    def point_reuse(self, im, lost):
        w, h = self.wh
        in_frame = np.full(len(self.map_pos), -1, np.int64)
        has_mp = self.map_index >= 0
        in_frame[self.map_index[has_mp]] = np.nonzero(has_mp)[0]
        if self.dev_templates and getattr(self.b, "device_reuse", False) and hasattr(self.b, "point_reuse"):
            # one backend call: candidates, tracking, gate and the append of the new slots' photometric information
            r = self.b.point_reuse(self.pose, self.wh, self.map_pos, in_frame.astype(np.int32), self.status, sorted(int(x) for x in lost), 0.75, True)
            if not r["n_cand"]:
                self.last_reuse = dict(cand_id=np.zeros(0, np.int64), accepted=np.zeros(0, bool))
                return 0
            return self._reuse_bookkeeping(in_frame, np.asarray(r["cand_id"], np.int64), np.asarray(r["xy"], F32), np.asarray(r["accepted"], bool), True)
        pc = se3f_act(self.pose, self.map_pos)
        uv = self.project(pc) if len(pc) else np.zeros((0, 2), F32)
        inside = (uv[:, 0] >= 0) & (uv[:, 0] < w) & (uv[:, 1] >= 0) & (uv[:, 1] < h)
        # candidates: the points lost in this frame and the map points the frame does not hold (tracking.cc:404-420), in front of the camera and
        # inside the image -- one pass over the map, ascending map index (the reference walks a std::set)
        present = np.zeros(len(self.map_pos), bool)
        held = np.nonzero(in_frame >= 0)[0]
        st_held = self.status[in_frame[held]]
        present[held] = (st_held == TRACKED_WITH_3D) | (st_held == JUST_TRIANGULATED)
        is_cand = np.zeros(len(self.map_pos), bool)
        if lost:
            is_cand[np.fromiter((int(x) for x in lost), np.int64, len(lost))] = True
        if len(pc):
            is_cand |= ~present & (pc[:, 2] >= 0) & inside
            is_cand &= inside & ~np.isnan(uv).any(1)
        cand = np.nonzero(is_cand)[0]
        if not len(cand):
            self.last_reuse = dict(cand_id=np.zeros(0, np.int64), accepted=np.zeros(0, bool))
            return 0
        seeds = uv[cand].astype(F32)
        if self.dev_templates:
            xy, st = self.b.reuse_track_archived(im, seeds, cand.astype(np.int32), 0.75)
        else:
            xy, st = self.b.reuse_track(im, seeds, [self.templates[int(mp)] for mp in cand], 0.75)
        # accepted: tracked, and within sqrt(5.99) px of the projection (fp32 arithmetic, element by element as the scalar form)
        xy = np.asarray(xy)
        ex = uv[cand, 0].astype(F32) - xy[:, 0].astype(F32)
        ey = uv[cand, 1].astype(F32) - xy[:, 1].astype(F32)
        ok = (np.asarray(st) == TRACKED_WITH_3D) & ~(ex * ex + ey * ey > F32(5.99))
        return self._reuse_bookkeeping(in_frame, cand, xy, ok, False)

    # tracking.cc:449-503: what the accepted candidates do to the frame.  appended: the backend has already appended the new slots'
    # photometric information to its tracker (the one-call path)
    def _reuse_bookkeeping(self, in_frame, cand, xy, ok, appended):
        self.last_reuse = dict(cand_id=np.asarray(cand, np.int64).copy(), accepted=np.asarray(ok, bool).copy())      # (for tests and probes)
        slot = in_frame[cand]
        upd = ok & (slot >= 0)                          # the frame holds a slot for the point: it is refreshed
        if upd.any():
            self.kp[slot[upd]] = xy[upd]
            self.pos[slot[upd]] = self.map_pos[cand[upd]]
            self.status[slot[upd]] = TRACKED_WITH_3D
        new = ok & (slot < 0)                           # candidates that enter the frame as new slots, in candidate order (one append below)
        new_k, new_mp = [int(k) for k in np.nonzero(new)[0]], [int(mp) for mp in cand[new]]
        reused = int(ok.sum())
        if new_mp:                                      # (the slots and their photometric information, appended in the loop's order)
            nk, nm = np.asarray(new_k), np.asarray(new_mp)
            self.kp = np.vstack([self.kp, xy[nk]]).astype(F32)
            self.pos = np.vstack([self.pos, self.map_pos[nm]]).astype(F32)
            self.status = np.concatenate([self.status, np.full(len(nm), TRACKED_WITH_3D, np.int32)]).astype(np.int32)
            self.map_index = np.concatenate([self.map_index, nm]).astype(np.int32)
            if self.mapping:                                       # a re-inserted map point gets a fresh class_id
                self.kp_id = np.concatenate([self.kp_id, self.next_kp_id + np.arange(len(nm))])
                self.next_kp_id += len(nm)
            if appended:
                return reused
            if self.dev_templates:
                self.b.insert_archived(nm.astype(np.int32), xy[nk].astype(F32))
                return reused
            tpl = [dict(self.templates[mp], xy=xy[k].astype(F32)) for k, mp in zip(new_k, new_mp)]
            if hasattr(self.b, "klt_insert_templates"):
                self.b.klt_insert_templates(tpl)
            else:
                for t in tpl:
                    self.b.klt_insert_template(t)
        return reused

    # ---- tracking.cc:336-392
    def keyframe_insertion(self, im):
        if self.since_kf < self.kf_every:
            self.since_kf += 1
            return False
        self.since_kf = 0
        if self.extract:
            # ExtractFeaturesInFrame (tracking.cc:374-382): the extractor is told the keypoints the frame
            # holds (TRACKED_WITH_3D and TRACKED, in slot order); new corners become TRACKED observations
            held = (self.status == TRACKED_WITH_3D) | (self.status == TRACKED)
            xy, _ = self.b.extract_features(im, self.kp[held])
            k = len(xy)
            self.kp = np.vstack([self.kp, xy]).astype(F32)
            self.pos = np.vstack([self.pos, np.zeros((k, 3), F32)]).astype(F32)
            self.status = np.concatenate([self.status, np.full(k, TRACKED, np.int32)]).astype(np.int32)
            self.map_index = np.concatenate([self.map_index, np.full(k, -1, np.int32)]).astype(np.int32)
            if self.mapping:                                       # extracted corners get fresh class_ids
                self.kp_id = np.concatenate([self.kp_id, self.next_kp_id + np.arange(k)])
                self.next_kp_id += k
        # KeyFrame(frame) + Frame::SetFromKeyFrame (keyframe.cc:26-55, frame.cc:47-77): the slots with 3D, then
        # the TRACKED ones; everything else leaves the frame
        order = np.concatenate([np.nonzero(self.status == TRACKED_WITH_3D)[0], np.nonzero(self.status == TRACKED)[0]])
        self.kp, self.pos, self.status, self.map_index = self.kp[order], self.pos[order], self.status[order], self.map_index[order]
        if self.mapping:
            self.kp_id = self.kp_id[order]
        self.pos[self.status == TRACKED] = 0
        self.map_index[self.status == TRACKED] = -1               # only the 3D slots keep their map point (frame.cc:56-62)
        if self.keyframe_ba:
            self.insert_keyframe()                                 # tracking.cc:354-358: the keyframe of this frame, queued for the mapping
        self.b.klt_set_reference(im, self.kp)
        if self.dev_templates:                                     # Frame::MapPointIdToIndex: slots that have a map point
            slots = np.nonzero(self.map_index >= 0)[0].astype(np.int32)
            self.b.archive_templates(slots, self.map_index[slots].astype(np.int32))
            return True
        tpl = self.b.klt_get_templates(len(self.map_index))
        for i, mp in enumerate(self.map_index):
            if mp >= 0:
                self.templates[mp] = tpl[i]
        return True
