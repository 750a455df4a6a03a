"""Inputs of tests/test_gpu_window_rg_embedded.py (test infrastructure, no GPU needed to build them): the windows of
tests/window_rg_cases.py -- an all-pairs graph with BAD connections, lists cut by min_weight, keyframes that each drop a third of their
points -- with a node set (nrs_synth.embedded_problem's flags), and the CPU side of the comparison: the ran-off rule of include/nrs.h
restated for the three embedded walks on the oracle's full lists.  It is the twin of window_rg_cases.walks_that_run_off with the node
table in place of the keyframe sets: a walk passes over every neighbour that is not a NODE COPY of its keyframe without counting it."""
import functools

import numpy as np

import nrs_oracle as O
import nrs_synth as S
import window_rg_cases as W

# nodes per window: about n / 6.  CASES are the windows the lists, the solve and the every-point-a-node comparison run on: each meets every
# condition of tests/test_window_rg_embedded_cases_cpu.py.  The 120-point window (208 observations: too few for them) serves only where a
# graph that small is needed: the run-off at the limit and the refusals.
NODES = {"120x3": 20, "900x6_kb8": 150, "2000x5": 333}
CASES = ["900x6_kb8", "2000x5"]
SMALL = "120x3"


@functools.lru_cache(maxsize=None)
def case(name):
    """the window of window_rg_cases.case(name) (shared, left unchanged) plus flag: uint8 per map point, 1 = node"""
    c = dict(W.case(name))
    flag, _ = S.embedded_problem(c["p"], NODES[name])
    c["flag"] = np.ascontiguousarray(flag, np.uint8)
    assert int(c["flag"].sum()) == NODES[name]
    return c


def _node_tables(c):
    """per keyframe: bool per map point, True where the keyframe holds a node copy of it"""
    tabs = []
    for pts in c["p"]["kf_points"]:
        t = np.zeros(c["n"], bool)
        t[np.asarray(pts)] = True
        tabs.append(t & (c["flag"] != 0))
    return tabs


def _walk(nbr, pt, cap, here, nxt=None):
    """the host loop of one walk over the first `cap` entries of pt's list (None: the whole list): (accepted, how it ended), the end
    being "bad" (a BAD entry), "count" (an entry that arrives with more than 10 accepted) or "end" (the entries ran out)"""
    lo, hi = int(nbr["rowptr"][pt]), int(nbr["rowptr"][pt + 1])
    if cap is not None:
        hi = min(hi, lo + cap)
    n_reg = 0
    for e in range(lo, hi):
        if n_reg > 10:
            return n_reg, "count"
        if nbr["status"][e] == O.GRAPH_BAD:
            return n_reg, "bad"
        o = int(nbr["col"][e])
        if here[o] and (nxt is None or nxt[o]):
            n_reg += 1
    return n_reg, "end"


def walks(c, cap=None):
    """every walk of the embedded window as (kind, observation, map point, accepted, end, ran_off) with kind "spring" / "damper" (a node
    copy; the damper walk where the next keyframe holds a copy of the node too) or "skin" (any other observation), on the oracle's lists cut
    to `cap` entries.  ran_off: the list is LONGER than cap, the walk came to the end of the prefix without a BAD entry and with no more
    than 10 accepted."""
    p, nbr, flag = c["p"], c["nbr"], c["flag"]
    tabs = _node_tables(c)
    out, i = [], 0
    for k, pts in enumerate(p["kf_points"]):
        for pt in pts:
            pt = int(pt)
            full = int(nbr["rowptr"][pt + 1]) - int(nbr["rowptr"][pt])
            cut = cap is not None and full > cap
            kinds = [("skin", None)]
            if flag[pt]:
                kinds = [("spring", None)]
                if k + 1 < len(tabs) and tabs[k + 1][pt]:
                    kinds.append(("damper", tabs[k + 1]))
            for kind, nxt in kinds:
                n_reg, end = _walk(nbr, pt, cap, tabs[k], nxt)
                out.append((kind, i, pt, n_reg, end, bool(cut and end == "end" and n_reg <= 10)))
            i += 1
    return out


def walks_that_run_off(c, cap):
    """(walks that run off at a prefix of cap entries, walks in all, skinned walks among those that run off)"""
    w = walks(c, cap)
    return sum(x[5] for x in w), len(w), sum(x[5] for x in w if x[0] == "skin")


def final_cap(c, first, limit):
    cap = min(first, limit)
    rounds = 1
    while walks_that_run_off(c, cap)[0]:
        assert cap < limit
        cap = min(limit, 2 * cap)
        rounds += 1
    return cap, rounds
