"""The oracle backend of the frame loop with the two mapping calls (test infrastructure): oracle/frame_loop_backend.OracleBackend plus
map_frame over tests/map_oracle.py and grow_graph over oracle/rgraph_oracle.DenseGraph -- the twins of nrs_frame_loop.GpuBackend's --
and the sequence the loop's mapping tests share."""
import functools

import numpy as np

import map_oracle as M
import nrs_frame_loop as FL
import nrs_synth as S
import rgraph_oracle as RG
from frame_loop_backend import OracleBackend

OPTS = dict(win=21, max_level=3, max_iters=10, epsilon=1e-4, min_eig=1e-4)
N_FRAMES, KF_EVERY = 25, 5
# Mapping::Options::rad_per_pixel for this sequence: the camera moves about 0.0012 rad of parallax per frame, so the rigid window
# [10, 20] x rad_per_pixel holds tracks of three to five frames -- the features a keyframe extracts, a few frames later
RAD_PER_PIXEL = 0.0003


class MappingOracleBackend(OracleBackend):
    def map_frame(self, tb, deform_mag, rad_per_pixel, rigidity_th=0.004, min_track=5):
        return M.landmark_triangulation(tb, deform_mag, rad_per_pixel, rigidity_th, min_track, -1)

    def grow_graph(self, graph, map_pos, new_ids, other_ids):
        n = len(map_pos)
        if n > graph.st.shape[0]:                                  # a DenseGraph of the new size with the old state in its corner
            g = RG.DenseGraph(n, float(graph.sigma), float(graph.stretch_th))
            m = graph.st.shape[0]
            for name in ("maxd", "mind", "d0", "st"):
                getattr(g, name)[:m, :m] = getattr(graph, name)
            graph = g
        graph.add_edges(np.asarray(map_pos, np.float32), np.asarray(new_ids), np.asarray(other_ids))
        return graph


@functools.lru_cache(maxsize=None)
def sequence():
    return S.make_frame_sequence(150, N_FRAMES, 41, half_size=True, deform_amp=0.1)


def run(backend, mapping, n_frames=N_FRAMES):
    sq = sequence()
    proj = lambda pc: FL.project_f32(sq["model"], sq["prm"], pc)
    kw = dict(mapping=True, rad_per_pixel=RAD_PER_PIXEL, camera=(sq["model"], sq["prm"])) if mapping else {}
    loop = FL.FrameLoop(backend, proj, sq["wh"], sq["scale"], sq["kp0"], sq["X0"], sq["graph"], sq["pose_q"][0], sq["pose_t"][0], sq["images"][0],
                        images_to_insert_keyframe=KF_EVERY, **kw)
    for f in range(1, n_frames):
        assert loop.track_image(sq["images"][f])
    return loop


class _Spy(MappingOracleBackend):
    """records what reaches the pose-and-deformation solve: (map ids, statuses) per frame"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.deform_calls = []

    def track_deform(self, graph, map_pos, f_map, f_status, *rest):
        self.deform_calls.append((np.asarray(f_map).copy(), np.asarray(f_status).copy(), len(map_pos)))
        return super().track_deform(graph, map_pos, f_map, f_status, *rest)


@functools.lru_cache(maxsize=None)
def oracle_run():
    """the oracle-backed loop with mapping over the whole sequence, computed once and shared (read only): (loop, backend)"""
    sq = sequence()
    b = _Spy(sq["model"], sq["prm"], OPTS, dense_graph=True)
    return run(b, True), b
