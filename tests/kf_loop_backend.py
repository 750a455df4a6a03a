"""The oracle backend of the frame loop with keyframe BA (test infrastructure): tests/map_loop_backend.MappingOracleBackend plus
dba_window -- the twin of nrs_frame_loop.GpuBackend.dba_window -- answered by the restatements: DenseGraph.get_edges of every map point
of the window (the whole list, as the reference's GetEdges returns it), nrs_oracle.dba_build over them, then the C++ restatement of
dba_solve (oracle/nrs_cpu.py; tests/test_oracle_cpp_cpu.py holds it to nrs_oracle.dba_solve).  And the sequence run the keyframe tests
share: tests/map_loop_backend.py's 25 frames with keyframe_ba=True."""
import functools

import numpy as np

import map_loop_backend as B
import nrs_cpu as CPU
import nrs_frame_loop as FL
import nrs_oracle as O


def full_lists(graph, points):
    """CSR over the graph's points holding DenseGraph.get_edges(p), whole, for every p in `points` (empty rows elsewhere)"""
    n = graph.n
    rows = {int(p): graph.get_edges(int(p)) for p in np.unique(np.asarray(points))}
    rowptr = np.zeros(n + 1, np.int64)
    for p, r in rows.items():
        rowptr[p + 1] = len(r[0])
    rowptr = np.cumsum(rowptr)
    col, w, d0, st = np.zeros(rowptr[-1], np.int32), np.zeros(rowptr[-1], np.float32), np.zeros(rowptr[-1], np.float32), np.zeros(rowptr[-1], np.int32)
    for p, r in rows.items():
        sl = slice(rowptr[p], rowptr[p + 1])
        col[sl], w[sl], d0[sl], st[sl] = r
    return dict(rowptr=rowptr.astype(np.int32), col=col, w=w, d0=d0, status=st)


class KeyframeOracleBackend(B.MappingOracleBackend):
    def dba_window(self, poses_qt, kf_points, lm_xyz, lm_uv, graph, scale, iters=5):
        nbr = full_lists(graph, np.concatenate(kf_points))
        e = O.dba_build(kf_points, nbr["rowptr"], nbr["col"], nbr["w"], nbr["d0"], nbr["status"])
        pq = np.asarray(poses_qt, np.float64).reshape(-1, 7)
        q, t, x, trace, _ = CPU.dba_solve(self.model, self.prm, pq[:, :4], pq[:, 4:], lm_xyz, e["lm_kf"], lm_uv, e["sp_ij"], e["sp_d0"], e["dm_idx"], e["dm_w"],
                                          scale, iters)
        self.windows = getattr(self, "windows", []) + [dict(kf_points=[np.asarray(k).copy() for k in kf_points], edges=e)]
        return dict(poses_qt=np.concatenate([q, t], 1), lm_xyz=np.asarray(x, np.float64).astype(np.float32), n_spring=len(e["sp_d0"]), n_damper=len(e["dm_w"]),
                    trials=len(trace))


def run(backend, n_frames=B.N_FRAMES, keyframe_ba=True, hook=None):
    sq = B.sequence()
    proj = lambda pc: FL.project_f32(sq["model"], sq["prm"], pc)
    loop = FL.FrameLoop(backend, proj, sq["wh"], sq["scale"], sq["kp0"], sq["X0"], sq["graph"], sq["pose_q"][0], sq["pose_t"][0], sq["images"][0],
                        images_to_insert_keyframe=B.KF_EVERY, mapping=True, rad_per_pixel=B.RAD_PER_PIXEL, camera=(sq["model"], sq["prm"]),
                        keyframe_ba=keyframe_ba)
    for f in range(1, n_frames):
        assert loop.track_image(sq["images"][f])
        if hook:
            hook(loop, f)
    return loop


@functools.lru_cache(maxsize=None)
def oracle_run():
    """the oracle-backed loop with keyframe BA over the whole sequence, computed once and shared (read only): (loop, backend, per-frame
    snapshots taken right after each frame: pose, the frame's 3D slots, map_pos)"""
    sq = B.sequence()
    b = KeyframeOracleBackend(sq["model"], sq["prm"], B.OPTS, dense_graph=True)
    snaps = []

    def hook(loop, f):
        snaps.append(dict(pose=(loop.pose[0].copy(), loop.pose[1].copy()), last_pose=(loop.last_pose[0].copy(), loop.last_pose[1].copy()),
                          kp=loop.kp.copy(), pos=loop.pos.copy(), status=loop.status.copy(), map_index=loop.map_index.copy(), kp_id=loop.kp_id.copy(),
                          map_pos=loop.map_pos.copy()))
    return run(b, hook=hook), b, snaps
