"""Windows of tests/test_gpu_embedded_window.py (and of the CPU check that they are not vacuous): make_dba_problem windows with
embedded_problem node sets, in two neighbour forms --
  nodes   the node-only lists (nrs_synth.node_lists)
  full    the window's full graph p["nbr"] with the same flags, so that walks pass over neighbours that are not nodes, and with about
          3 % of its connection statuses set to NRS_GRAPH_BAD by a seeded draw, so that walks are cut short."""
import numpy as np

import nrs_synth as S

GRAPH_BAD = S.GRAPH_BAD                                              # include/nrs.h NRS_GRAPH_BAD
# (map points, keyframes, nodes, seed, camera model, keyword arguments of make_dba_problem)
CASES = [(300, 4, 40, 53, S.PINHOLE, {}), (600, 6, 80, 54, S.PINHOLE, {}), (400, 5, 60, 55, S.KB8, dict(dropout=0.3))]
FORMS = ("nodes", "full")
_cache = {}


def window(case, form):
    """(p, flag, nb) of a case; built once, shared and left unchanged"""
    key = (case[:4], form)
    if key not in _cache:
        n, k, m, seed, model, kw = case
        if case[:4] not in _cache:
            p = S.make_dba_problem(n, k, seed, model, **kw)
            _cache[case[:4]] = (p,) + tuple(S.embedded_problem(p, m))
        p, flag, nodes = _cache[case[:4]]
        if form == "nodes":
            nb = nodes
        else:
            nb = {key2: np.array(v) for key2, v in p["nbr"].items()}
            rng = np.random.default_rng(1000 + seed)
            nb["status"][rng.uniform(size=len(nb["status"])) < 0.03] = GRAPH_BAD
        _cache[key] = (p, flag, nb)
    return _cache[key]


def walk_stats(p, flag, nb):
    """the skinned walks of nrs_dba_build_edges_embedded restated: per observation that is not a node the number of node copies its walk
    accepts; and the number of observations (of any kind) whose walk over node copies stops at a BAD connection"""
    rp, col, st = nb["rowptr"], nb["col"], nb["status"]
    accepted, cut = [], 0
    for pts in p["kf_points"]:
        here = np.zeros(len(flag), bool)
        here[pts] = True
        here &= np.asarray(flag) != 0
        for q in pts:
            n_reg, stopped = 0, False
            for e in range(rp[q], rp[q + 1]):
                if n_reg > 10:
                    break
                if st[e] == GRAPH_BAD:
                    stopped = True
                    break
                if here[col[e]]:
                    n_reg += 1
            cut += stopped
            if not flag[q]:
                accepted.append(n_reg)
    return np.array(accepted), cut


def check_not_vacuous(case, form, p, flag, nb, e):
    """the conditions under which a comparison of the lists says something, on the HOST lists e"""
    n_obs = sum(len(x) for x in p["kf_points"])
    accepted, cut = walk_stats(p, flag, nb)
    assert n_obs > 256                                               # more than one workgroup
    assert len(e["lm_obs"]) + len(accepted) == n_obs
    assert len(e["sp_ij"]) >= 1 and len(e["dm_idx"]) >= 1 and len(e["sk_obs"]) >= 1
    assert len(e["sk_obs"]) == (accepted > 0).sum()
    if form == "full":                                               # (BAD statuses, and lists that hold few nodes: the node-only lists of
        assert ((e["sk_node"] >= 0).sum(1) < 11).any()               # the denser windows fill all 11 slots of every skinned observation)
        assert (accepted == 0).any()                                 # an observation bound to nothing
        assert cut >= 1                                              # a walk cut short by a BAD status
        assert (nb["status"] == GRAPH_BAD).any() and (np.asarray(flag)[nb["col"]] == 0).any()
    if case[5].get("dropout"):
        assert len(set(len(x) for x in p["kf_points"])) > 1
