"""The node-selection cases tests/test_skin_cases_cpu.py vets on the CPU and tests/test_gpu_skin_cases.py runs on the device
(nrs_skin_select_nodes, kernel k_fps of csrc/nrs_skin.hip): each case is built once, with the oracle's picks, and handed out read-only.

A case = dict(name, pos, eligible or None, m, picks = oracle/skin_oracle.select_nodes).  A refusal = dict(name, pos, eligible or None, m,
words = what the message must hold).  Every case has n <= 2200.

k_fps is ONE workgroup of FPS_BLK = 1024 threads, 16 waves of 64.  Thread t holds the rows t, t + 1024, ... (a "trip" is one pass of the
workgroup over 1024 rows), keeps its own first maximum, then a wave-shuffle arg-max and a 16-entry LDS arg-max decide: ties go to the
lowest index at each of the three levels.  What exercises which level:
  sizes             seeded random clouds around the strides: below one wave, one wave, one trip, two trips and one row
  lattice           13 x 13 x 13 integer lattice in a seeded row order: squared distances are small integers, so most rounds tie -- within a
                    thread, within a wave and across waves, and the winner's wave is usually not the lowest tied one (lattice_holds)
  lattice_masked    ... 60 % eligible; lattice_one_wave: only the rows of wave 15 are eligible (both trips)
  coincident        1500 copies of one point: EVERY round is a tie of everything that is left, picks 0, 1, 2, ...
  late_first        n = 2049, eligible from row 1030 on: nothing eligible in the first trip; exactly m eligible
  overflow          eight points of magnitude 1e20: the squared distance is +inf on both sides, running minima that stay +inf tie
  nonfinite_*_lost  NaN / +-inf on rows that are NOT eligible: the picks are those of the same cloud with these rows zeroed"""
import functools

import numpy as np

import skin_oracle as K

F32 = np.float32
FPS_BLK, WAVE = 1024, 64
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)
LATTICE_MINIMA = dict(same_thread=20, same_wave=50, cross_wave=50, winner_not_lowest_wave=50)


def literal(pos, m, ok):
    """farthest point sampling as a plain double loop over points and picks (fp32 scalars): the statement the oracle is held to"""
    pos = pos.astype(np.float32)
    sel = [int(np.argmax(ok))]
    with np.errstate(over="ignore"):
        while len(sel) < m:
            best, bi = np.float32(-1), -1
            for j in range(len(pos)):
                if not ok[j] or j in sel:
                    continue
                dmin = np.float32(np.inf)
                for s in sel:
                    d = pos[j] - pos[s]
                    d2 = np.float32(np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])) + np.float32(d[2] * d[2])
                    dmin = min(dmin, np.float32(d2))
                if dmin > best:
                    best, bi = dmin, j
            sel.append(bi)
    return np.asarray(sel, np.int32)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _case(name, pos, eligible, m, picks_of=None):
    """picks_of: the cloud the oracle runs on, where it is not `pos` itself"""
    pos = np.ascontiguousarray(pos, F32)
    el = None if eligible is None else np.ascontiguousarray(eligible, bool)
    return _freeze(dict(name=name, pos=pos, eligible=el, m=int(m), picks=K.select_nodes(pos if picks_of is None else picks_of, int(m), el)))


def _refusal(name, pos, eligible, m, words):
    pos = np.ascontiguousarray(pos, F32)
    el = None if eligible is None else np.ascontiguousarray(eligible, bool)
    return _freeze(dict(name=name, pos=pos, eligible=el, m=int(m), words=tuple(words)))


def _sizes_ms(n):
    return sorted({m for m in (1, 2, min(n, 70)) if m <= n})        # (n <= 65: min(n, 70) = n, every point a node, in pick order)


@functools.lru_cache(maxsize=None)
def _cloud(n):
    return np.random.default_rng(100 + n).uniform(-20, 20, (n, 3)).astype(F32)


@functools.lru_cache(maxsize=None)
def _lattice():
    g = np.arange(13, dtype=F32)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(p[np.random.default_rng(5).permutation(len(p))])


def _late_first():
    n = 2049
    el = np.arange(n) >= 1030
    return _cloud(n), el, int(el.sum())


def _overflow():
    rng = np.random.default_rng(8)
    pos = rng.uniform(-20, 20, (108, 3)).astype(F32)
    rows = np.sort(rng.permutation(np.arange(1, 108))[:8])          # row 0 stays ordinary: pick 0, at +inf from all eight
    sign = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], F32)
    pos[rows] = sign[rng.permutation(8)] * F32(1e20)                # the eight corners: (2e20)^2 overflows in fp32
    return pos, rows


def _nonfinite(value):
    """n = 1100 (two trips), 70 % eligible; `value` on one coordinate of six rows that are not eligible, one of them in the second trip"""
    rng = np.random.default_rng(9)
    n = 1100
    pos = rng.uniform(-20, 20, (n, 3)).astype(F32)
    el = rng.uniform(size=n) < 0.7
    lost = np.nonzero(~el)[0]
    rows = np.concatenate([lost[:3], lost[lost >= FPS_BLK][:1], lost[-2:]])
    bad = pos.copy()
    bad[rows, np.arange(len(rows)) % 3] = value
    zeroed = pos.copy()
    zeroed[rows] = 0
    return bad, zeroed, el, rows


def _lost_case(name, value):
    bad, zeroed, el, _ = _nonfinite(value)
    return _case(name, bad, el, 70, picks_of=zeroed)                # the oracle runs on the cloud with these rows set to zero


def _one_wave_mask(n, wave):
    return (np.arange(n) % FPS_BLK) // WAVE == wave


_BUILD = {}
for _n in SIZES:
    for _m in _sizes_ms(_n):
        _BUILD["sizes_n%d_m%d" % (_n, _m)] = (lambda n, m: lambda name: _case(name, _cloud(n), None, m))(_n, _m)
_BUILD.update(
    lattice=lambda name: _case(name, _lattice(), None, 200),
    lattice_masked=lambda name: _case(name, _lattice(), np.random.default_rng(6).uniform(size=2197) < 0.6, 60),
    lattice_one_wave=lambda name: _case(name, _lattice(), _one_wave_mask(2197, 15), 60),
    coincident=lambda name: _case(name, np.tile(np.array([1.5, -2.25, 60.0], F32), (1500, 1)), None, 1500),
    coincident_masked=lambda name: _case(name, np.tile(np.array([1.5, -2.25, 60.0], F32), (1500, 1)), np.arange(1500) % 3 == 0, 500),
    late_first=lambda name: _case(name, *_late_first()),
    overflow=lambda name: _case(name, _overflow()[0], None, 30),
    nonfinite_nan_lost=lambda name: _lost_case(name, np.nan),
    nonfinite_inf_lost=lambda name: _lost_case(name, np.inf),
    nonfinite_minus_inf_lost=lambda name: _lost_case(name, -np.inf))
CASES = list(_BUILD)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILD[name](name)


def _nonfinite_eligible(name, value):
    """the cloud of nonfinite_*_lost with `value` on two ELIGIBLE rows as well, the first of them beyond the first trip's first wave: the
    message names the lower one"""
    bad, _, el, _ = _nonfinite(value)
    rows = np.nonzero(el)[0]
    first, second = int(rows[rows >= 100][0]), int(rows[rows >= FPS_BLK][0])
    bad = bad.copy()
    bad[first, 1] = value
    bad[second, 2] = value
    return _refusal(name, bad, el, 70, ["eligible point %d " % first, "non-finite"])


def _nan_at(pos, row):
    pos = pos.copy()
    pos[row, 0] = np.nan
    return pos


def _late_refusals():
    pos, el, count = _late_first()
    return {"late_first_one_too_many": lambda name: _refusal(name, pos, el, count + 1, ["%d nodes wanted" % (count + 1), "%d eligible" % count]),
            "none_eligible": lambda name: _refusal(name, pos, np.zeros(len(pos), bool), 1, ["1 nodes wanted", "0 eligible"])}


_BUILD_REFUSALS = dict(_late_refusals(),
                       nan_eligible=lambda name: _nonfinite_eligible(name, np.nan),
                       inf_eligible=lambda name: _nonfinite_eligible(name, np.inf),
                       minus_inf_eligible=lambda name: _nonfinite_eligible(name, -np.inf),
                       nan_no_mask=lambda name: _refusal(name, _nan_at(_cloud(65), 64), None, 2, ["eligible point 64 ", "non-finite"]))
REFUSALS = list(_BUILD_REFUSALS)
GOOD_AFTER_REFUSAL = "sizes_n1025_m70"                             # the good call that follows every refusal on the same context


@functools.lru_cache(maxsize=None)
def refusal(name):
    return _BUILD_REFUSALS[name](name)


def sqdist_matrix(pos):
    """the full fp32 squared-distance matrix in the kernel's operation order, (dx*dx + dy*dy) + dz*dz, every product and sum rounded"""
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = (pos[:, None, a] - pos[None, :, a] for a in range(3))
        return ((dx * dx + dy * dy) + dz * dz).astype(F32)


def restatement(pos, m, eligible, dist=None):
    """independent of skin_oracle.select_nodes: a pick is the arg-max, over the eligible points not yet picked, of the column-wise
    minimum of the distance matrix over the picked rows (np.argmax: the first maximum).  Nothing is carried from round to round"""
    n = len(pos)
    ok = np.ones(n, bool) if eligible is None else np.asarray(eligible, bool)
    dist = sqdist_matrix(pos) if dist is None else dist
    picks = [int(np.nonzero(ok)[0][0])]
    free = ok.copy()
    while len(picks) < m:
        free[picks[-1]] = False
        assert free.any()
        picks.append(int(np.argmax(np.where(free, dist[picks].min(0), F32(-1)))))
    return np.asarray(picks, np.int32)


def tie_rounds(c):
    """From the oracle's picks alone (integer positions: exact in int64).  Per round, the rows that attain the maximum of the running
    minima; -> dict of counts of rounds with: any tie; two tied rows held by one thread (congruent mod FPS_BLK); two tied rows in one
    wave; tied rows in different waves; the winner in a wave that is not the lowest-numbered tied wave.  Asserts on the way that the
    pick IS the lowest tied row"""
    pos = c["pos"].astype(np.int64)
    assert np.array_equal(pos, c["pos"])
    ok = np.ones(len(pos), bool) if c["eligible"] is None else c["eligible"]
    mind = np.where(ok, np.iinfo(np.int64).max, -1)
    counts = dict(rounds=0, any_tie=0, same_thread=0, same_wave=0, cross_wave=0, winner_not_lowest_wave=0)
    for k in range(1, c["m"]):
        last = int(c["picks"][k - 1])
        live = mind >= 0
        mind[live] = np.minimum(mind[live], ((pos[live] - pos[last]) ** 2).sum(1))
        mind[last] = -1
        tied = np.nonzero(mind == mind.max())[0]
        assert mind.max() >= 0 and c["picks"][k] == tied[0], k
        thread, wave = tied % FPS_BLK, (tied % FPS_BLK) // WAVE
        counts["rounds"] += 1
        counts["any_tie"] += len(tied) > 1
        counts["same_thread"] += len(set(thread)) < len(tied)
        counts["same_wave"] += len(set(wave)) < len(tied)
        counts["cross_wave"] += len(set(wave)) > 1
        counts["winner_not_lowest_wave"] += int(wave[0]) != int(wave.min())
    return {k: int(v) for k, v in counts.items()}


def lattice_holds(c):
    """-> the counts of tie_rounds, at or above LATTICE_MINIMA: the three tie rules of k_fps decide picks of this case"""
    counts = tie_rounds(c)
    for k, least in LATTICE_MINIMA.items():
        assert counts[k] >= least, (k, counts)
    return counts
