"""The oracle backend of the frame loop with mapping and keyframe BA in the EMBEDDED-deformation mode (test infrastructure):
tests/kf_loop_backend.KeyframeOracleBackend with a node set -- the twin of nrs_frame_loop.GpuBackend(n_nodes=...).  The node set is the
one chosen on the initial map (oracle/frame_loop_backend.py); map points added by mapping get a zero flag, so they are always skinned.
dba_window is answered by the restatements: DenseGraph.get_edges of every map point of the window (whole lists),
embedded_oracle.dba_build_embedded over them, then the C++ restatement of dba_solve_embedded (oracle/nrs_cpu.py;
tests/test_oracle_cpp_cpu.py holds it to embedded_oracle.dba_solve_embedded).  What the oracle does with an observation that reaches no
node copy is the rule: it constrains nothing and its position comes back unchanged.  And the sequence run the embedded keyframe tests
share: tests/map_loop_backend.py's 25 frames, 40 of its map points as nodes."""
import functools

import numpy as np

import embedded_oracle as E
import kf_loop_backend as K
import map_loop_backend as B
import nrs_cpu as CPU
import nrs_synth as S

N_NODES = 40


class EmbeddedKeyframeOracleBackend(K.KeyframeOracleBackend):
    def __init__(self, model, prm, klt_opts, n_nodes=N_NODES):
        super().__init__(model, prm, klt_opts, dense_graph=True, n_nodes=n_nodes)

    def grow_graph(self, graph, map_pos, new_ids, other_ids):
        graph = super().grow_graph(graph, map_pos, new_ids, other_ids)
        if len(self.node_flag) < graph.n:                           # new map points are never nodes
            self.node_flag = np.concatenate([self.node_flag, np.zeros(graph.n - len(self.node_flag), np.uint8)])
        return graph

    def dba_window(self, poses_qt, kf_points, lm_xyz, lm_uv, graph, scale, iters=5):
        nbr = K.full_lists(graph, np.concatenate(kf_points))
        flag = self.node_flag[:graph.n]
        e = E.dba_build_embedded(kf_points, flag, nbr["rowptr"], nbr["col"], nbr["w"], nbr["d0"], nbr["status"])
        obs = dict(lm_xyz=np.asarray(lm_xyz, np.float32).reshape(-1, 3), lm_uv=np.asarray(lm_uv, np.float32).reshape(-1, 2),
                   lm_kf=np.concatenate([np.full(len(k), i, np.int32) for i, k in enumerate(kf_points)]))
        w = S.embedded_window(obs, e)
        pq = np.asarray(poses_qt, np.float64).reshape(-1, 7)
        q, t, x, sk, trace, _ = CPU.dba_solve_embedded(self.model, self.prm, pq[:, :4], pq[:, 4:], w["lm_xyz"], w["lm_kf"], w["lm_uv"], e["sp_ij"], e["sp_d0"],
                                                       e["dm_idx"], e["dm_w"], w["sk_kf"], w["sk_uv"], w["sk_xyz"], e["sk_node"], e["sk_omega"], scale, iters)
        xyz = obs["lm_xyz"].copy()                                  # per observation: bound to nothing = unchanged
        xyz[e["lm_obs"]] = np.asarray(x, np.float64).astype(np.float32)
        xyz[e["sk_obs"]] = np.asarray(sk, np.float64).reshape(-1, 3).astype(np.float32)
        self.windows = getattr(self, "windows", []) + [dict(kf_points=[np.asarray(k).copy() for k in kf_points], edges=e, flag=flag.copy(), n_map=graph.n)]
        return dict(poses_qt=np.concatenate([q, t], 1), lm_xyz=xyz, n_spring=len(e["sp_d0"]), n_damper=len(e["dm_w"]), trials=len(trace))


@functools.lru_cache(maxsize=None)
def oracle_run():
    """the oracle-backed embedded loop with mapping and keyframe BA over the whole sequence, computed once and shared (read only)"""
    sq = B.sequence()
    b = EmbeddedKeyframeOracleBackend(sq["model"], sq["prm"], B.OPTS)
    return K.run(b), b
