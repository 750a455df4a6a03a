"""Inputs of tests/test_gpu_window_rg.py (test infrastructure, no GPU needed to build them): a BA window over an all-pairs graph whose
lists hold BAD connections and are cut by min_weight, keyframes that each drop their own third of the points -- and the CPU side of the
comparison: the oracle's DenseGraph in the same state, its full lists, and the ran-off rule of include/nrs.h restated on them."""
import functools

import numpy as np

import nrs_oracle as O
import nrs_synth as S
import rgraph_oracle as RG

STRETCH_TH = 0.06
# (points, keyframes, camera model, seed): 120 x 3 and 900 x 6 take the host packer or the device packer by their padded rows
# (256 per keyframe: 768 and 4608 against the threshold of 2048), 2000 x 5 pinhole takes the device packer
CASES = {"120x3": (120, 3, S.PINHOLE, 5), "900x6_kb8": (900, 6, S.KB8, 7), "2000x5": (2000, 5, S.PINHOLE, 11)}


@functools.lru_cache(maxsize=None)
def case(name):
    n, n_kf, model, seed = CASES[name]
    p = S.make_dba_problem(n, n_kf, seed, model, dropout=1.0 / 3.0)          # every keyframe drops its own random third
    sc = p["scene"]
    X0 = np.asarray(sc["X0"], np.float32)
    d = np.sqrt(((X0[:, None, :] - X0[None, :, :]) ** 2).sum(-1))
    # 1.5 sigma = 0.7 x the diameter: points in the middle keep every connection above min_weight, so GetEdges goes on into their BAD
    # connections (regularization_graph.cc:71-87 breaks at the FIRST weight below min_weight of the sorted list); the lists of points
    # near the rim are cut inside the NEUTRAL class and hold no BAD entry
    sigma = float(d.max() * 0.7 / 1.5)
    # the update's positions: the deformed surface with a jitter that stretches the nearest pairs past the threshold (BAD connections at the
    # end of most lists), and one point in ten moved by a good part of sigma: most connections of such a point are BAD, its walks end early
    rng = np.random.default_rng(seed)
    X1 = np.asarray(sc["Xk_true"][-1], np.float64) + rng.normal(0, 0.02 * sigma, (n, 3))
    far = rng.choice(n, n // 10, replace=False)
    X1[far] += rng.normal(0, 0.4 * sigma, (len(far), 3))
    X1 = X1.astype(np.float32)
    g = RG.DenseGraph(n, sigma, STRETCH_TH)
    ids = np.arange(n)
    g.add_edges(X0, ids, ids)
    for i in ids:
        g.update_vertex(X1, int(i))
    rows = [g.get_edges(int(i)) for i in ids]
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r[0]) for r in rows])
    nbr = dict(rowptr=rowptr.astype(np.int32), col=np.concatenate([r[0] for r in rows]).astype(np.int32), w=np.concatenate([r[1] for r in rows]).astype(np.float32),
               d0=np.concatenate([r[2] for r in rows]).astype(np.float32), status=np.concatenate([r[3] for r in rows]).astype(np.int32))
    return dict(name=name, n=n, n_kf=n_kf, p=p, X0=X0, X1=X1, sigma=sigma, oracle_graph=g, nbr=nbr)


def walks_that_run_off(c, cap):
    """The ran-off rule on the oracle's lists cut to `cap` entries: (walks that run off, walks in all).  A walk (the springs of an
    observation; its dampers where the next keyframe holds the point) over a list LONGER than cap runs off when it comes to the end of the
    first cap entries without having met a BAD one and with no more than 10 regularisers counted (a neighbour the keyframe -- for dampers
    both keyframes -- does not observe is passed over without counting)."""
    p, nbr = c["p"], c["nbr"]
    kfs = [set(int(x) for x in k) for k in p["kf_points"]]
    ran = total = 0
    for k, pts in enumerate(p["kf_points"]):
        for pt in pts:
            lo, hi = int(nbr["rowptr"][pt]), int(nbr["rowptr"][pt + 1])
            for damper in (False, True):
                if damper and (k + 1 >= len(kfs) or int(pt) not in kfs[k + 1]):
                    continue
                total += 1
                if hi - lo <= cap:
                    continue
                n_reg, ended = 0, False
                for e in range(lo, lo + cap):
                    if n_reg > 10 or nbr["status"][e] == O.GRAPH_BAD:
                        ended = True
                        break
                    o = int(nbr["col"][e])
                    if o in kfs[k] and (not damper or o in kfs[k + 1]):
                        n_reg += 1
                ran += (not ended) and n_reg <= 10
    return ran, total


def final_cap(c, first, limit):
    cap = min(first, limit)
    rounds = 1
    while walks_that_run_off(c, cap)[0]:
        assert cap < limit
        cap = min(limit, 2 * cap)
        rounds += 1
    return cap, rounds
