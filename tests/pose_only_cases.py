"""The a1 (CameraPoseOptimization, nrs_pose_only_solve) cases tests/test_pose_only_cases_cpu.py vets on the CPU (NumPy oracle against the
C++ restatement) and tests/test_gpu_pose_only_forms.py runs through the C ABI in all three kernel forms of csrc/nrs_pose_only.hip:

  A  one workgroup, points cached in LDS        n <= 7168  (hipFuncSetAttribute from n = 2458)
  B  one workgroup, points read from global     7169 <= n < 32768, or NRS_PO_NO_CACHE=1
  C  many workgroups (k_po_pass / k_po_step)    n >= 32768, or NRS_PO_MULTI_MIN; NRS_PO_MULTI_GROUPS=<g> caps its grid

ONE tracking problem is generated per camera model and its active points are SLICED to exactly n (uv[:n], X[:n]): sizes are exact and
generation is paid once.  A case is a dict: model, prm, uv (n, 2) f32, X (n, 3) f32, pose_q, pose_t (the seed).  `case(name)` builds it
once and `oracle(name)` runs oracle/nrs_oracle.py pose_only_solve on it once; both are shared by every test and must not be written to.

Names: pin_<n> / kb8_<n> (the size ladders and the hand-over pair), far_seed, all_outliers_after_round0, behind_camera."""
import functools

import numpy as np

import nrs_oracle as O
import nrs_synth as S

F32 = np.float32

# every size at which the code takes another path, and one either side: rank-deficient and exactly determined H (1, 2, 3), a wave
# (64), the single workgroup (512), a slot of the many-workgroup form (256), the dynamic-LDS attribute (20 n > 48 KiB from 2458), the
# LDS cache's limit (7168), and a form B frame well inside its range
LADDER_PINHOLE = (1, 2, 3, 5, 6, 7, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2457, 2458, 7168, 7169, 12000)
LADDER_KB8 = (3, 65, 513, 7169)
HANDOVER = (32767, 32768)                     # the default hand-over from form B to form C
NARROW_PINHOLE = (1, 5, 255, 256, 257, 513, 1500, 7169)     # form C on a grid of 1-3 workgroups
NARROW_KB8 = (513,)
LADDER = ["pin_%d" % n for n in LADDER_PINHOLE] + ["kb8_%d" % n for n in LADDER_KB8]
NARROW = ["pin_%d" % n for n in NARROW_PINHOLE] + ["kb8_%d" % n for n in NARROW_KB8]
CONTROL = ["far_seed", "all_outliers_after_round0", "behind_camera"]
NAMES = LADDER + ["pin_1500"] + ["pin_%d" % n for n in HANDOVER] + CONTROL

# ---- tolerances ---------------------------------------------------------------------------------------------------------------------
# a1's bar (tests/test_gpu_pose_only.py): quaternion components 1e-6, translation 1e-5 map units.
TOL_Q, TOL_T = 1e-6, 1e-5
# Below 6 points H = J^T J has rank 2 n < 6 (or is exactly determined, n = 3) and only lambda makes H + lambda I positive definite: the
# step is the fp64 sums' rounding divided by lambda ~ 1e-5 max diag, so the ORDER of the sums shows in the pose.  The bar there is 10 x
# the disagreement of the two CPU oracles (NumPy: pairwise sums over edge arrays; C++: a serial loop), never below TOL_Q / TOL_T.
# Measured by tests/test_pose_only_cases_cpu.py (max |dq|, max |dt| between O.pose_only_solve and CPU.pose_only_solve):
#   pin_1   dq 5.7e-15   dt 3.4e-14
#   pin_2   dq 4.4e-15   dt 2.8e-14
#   pin_3   dq 2.5e-14   dt 1.6e-13
#   pin_5   dq 7.9e-16   dt 4.9e-15
#   kb8_3   dq 7.0e-15   dt 5.9e-14
# (no larger than at 6 points and above, 1.6e-14 / 9.9e-14 at pin_6: lambda = 1e-5 max diag H keeps the damped system well
# conditioned on these frames).  10 x every one of them is far below the floor, so the floor it is: no size needs a wider bar.
SMALL_N_MEASURED = {"pin_1": (5.7e-15, 3.4e-14), "pin_2": (4.4e-15, 2.8e-14), "pin_3": (2.5e-14, 1.6e-13), "pin_5": (7.9e-16, 4.9e-15),
                    "kb8_3": (7.0e-15, 5.9e-14)}
SMALL_N_TOL = {k: (max(TOL_Q, 10 * dq), max(TOL_T, 10 * dt)) for k, (dq, dt) in SMALL_N_MEASURED.items()}

# the forms differ from one another in the order of their fp64 sums only (tests/test_gpu_pose_only.py, the 100k-point frame)
TOL_Q_FORMS, TOL_T_FORMS = 1e-9, 1e-8

# a point whose float chi2 lies this close (relative) to the 5.99 gate may be classified either way by another summation order
GATE, GATE_BAND_REL, GATE_BAND_MAX = 5.99, 1e-6, 2
NOISE = 3e-7                                   # conftest.compare_lm_traces: where the oracle's own decisions reach the fp32 noise floor


def n_points(name):
    return len(case(name)["uv"])


def tolerance(name):
    """(q, t) bar of the device against the oracle on case `name`"""
    if n_points(name) < 6:
        return SMALL_N_TOL[name]
    return TOL_Q, TOL_T


# ---- the two generated problems --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem(model):
    n, seed = {S.PINHOLE: (42000, 31), S.KB8: (9500, 32)}[model]
    tp = S.make_tracking_problem(n, seed, model)
    m = tp["status"] == 0
    uv, X = np.ascontiguousarray(tp["uv"][m], F32), np.ascontiguousarray(tp["X_prev"][m], F32)
    assert len(uv) >= {S.PINHOLE: HANDOVER[1], S.KB8: max(LADDER_KB8)}[model]
    return dict(model=tp["model"], prm=tp["prm"], uv=uv, X=X, pose_q=tp["pose_q"], pose_t=tp["pose_t"])


def _slice(model, n, pose_q=None, pose_t=None):
    p = _problem(model)
    return dict(model=p["model"], prm=p["prm"], uv=p["uv"][:n].copy(), X=p["X"][:n].copy(),
                pose_q=p["pose_q"].copy() if pose_q is None else pose_q, pose_t=p["pose_t"].copy() if pose_t is None else pose_t)


def _moved_seed(p, rot, shift, seed):
    """the problem's seed pose rotated by `rot` radians about a seeded axis and shifted by `shift` map units, as floats"""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=3)
    w *= rot / np.linalg.norm(w)
    dt = rng.normal(size=3)
    dt *= shift / np.linalg.norm(dt)
    k = w / rot
    dq = np.array([*(np.sin(rot / 2) * k), np.cos(rot / 2)])
    q = _quat_mul(dq, p["pose_q"])
    return q.astype(F32).astype(np.float64), (p["pose_t"] + dt).astype(F32).astype(np.float64)


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def _far_seed():
    """600 points, the seed 1.6 rad and 3 map units off: round 0 opens with three rejected trials, well above the noise floor"""
    q, t = _moved_seed(_problem(S.PINHOLE), 1.6, 3.0, 103)
    return _slice(S.PINHOLE, 600, q, t)


def _all_outliers():
    """600 points, the seed 1.0 rad and 2 map units off: round 0 runs its ten iterations into a pose that fits nothing, every edge is
    an outlier behind it, and rounds 1 and 2 have no active edge"""
    q, t = _moved_seed(_problem(S.PINHOLE), 1.0, 2.0, 103)
    return _slice(S.PINHOLE, 600, q, t)


N_BEHIND = 10


def _behind_camera():
    """300 points; every 30th is mirrored through the camera's z = 0 plane at the seed (negative camera-frame depth, none at 0)"""
    c = _slice(S.PINHOLE, 300)
    R = O.quat_to_R(O.quat_normalize(c["pose_q"]))
    idx = np.arange(0, 300, 30)
    assert len(idx) == N_BEHIND
    pc = c["X"][idx].astype(np.float64) @ R.T + c["pose_t"]
    pc[:, 2] = -pc[:, 2]
    c["X"][idx] = ((pc - c["pose_t"]) @ R).astype(F32)
    return c


def depth_at_seed(c):
    R = O.quat_to_R(O.quat_normalize(c["pose_q"]))
    return (c["X"].astype(np.float64) @ R.T + c["pose_t"])[:, 2]


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "far_seed":
        c = _far_seed()
    elif name == "all_outliers_after_round0":
        c = _all_outliers()
    elif name == "behind_camera":
        c = _behind_camera()
    else:
        kind, n = name.split("_")
        c = _slice({"pin": S.PINHOLE, "kb8": S.KB8}[kind], int(n))
        assert len(c["uv"]) == int(n)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ---- the oracle's answer -----------------------------------------------------------------------------------------------------------------
def compared_prefix(rnd, noise=NOISE):
    """the trials of one round that conftest.compare_lm_traces compares: up to the first whose chi2 change is on the noise floor"""
    out = []
    for y in rnd:
        if abs(y["chi"] - y["chi_new"]) <= noise * abs(y["chi"]):
            break
        out.append(y)
    return out


def rejection_run(trials):
    """the longest run of consecutive rejected trials within one iteration"""
    best, cur, it = 0, 0, None
    for y in trials:
        if y["iter"] != it:
            cur, it = 0, y["iter"]
        cur = 0 if y["accepted"] else cur + 1
        best = max(best, cur)
    return best


@functools.lru_cache(maxsize=None)
def oracle(name):
    """dict of O.pose_only_solve on case(name): q, t, inl, rounds (the trace, a list of trials per round that ran), trace (flat, with
    `round`), iterations, compared (trials compare_lm_traces compares), to_the_end (no round's comparison stops early), band (the
    points whose chi2 is within GATE_BAND_REL of the gate at any round's classification)"""
    c = case(name)
    rounds, chis = [], []
    q, t, inl = O.pose_only_solve(c["model"], c["prm"], c["uv"], c["X"], c["pose_q"], c["pose_t"], rounds, chis)
    band = np.zeros(len(inl), bool)
    for ch in chis:
        band |= np.abs(ch.astype(np.float64) - GATE) <= GATE_BAND_REL * GATE
    # a round that starts with no active edge runs no trial and the oracle appends no trace for it: put the empty rounds back, so
    # that rounds[r] is round r (round r > 0 runs when round r - 1's classification left an inlier)
    ran = [len(inl) > 0] + [bool((~(ch > O.TH2_SQ)).any()) for ch in chis[:2]]
    it = iter(rounds)
    rounds = [next(it) if r else [] for r in ran]
    assert next(it, None) is None
    flat = [dict(r, round=i) for i, rnd in enumerate(rounds) for r in rnd]
    pre = [compared_prefix(r) for r in rounds]
    out = dict(q=q, t=t, inl=inl, rounds=rounds, trace=flat, iterations=sum(len({y["iter"] for y in r}) for r in rounds),
               compared=sum(len(p) for p in pre), to_the_end=all(len(p) == len(r) for p, r in zip(pre, rounds)), band=band,
               n_band=int(band.sum()), empty_rounds=[r for r in range(3) if not ran[r]])
    for v in (q, t, inl, band):
        v.setflags(write=False)
    return out


def compare_traces(trials, name):
    """conftest.compare_lm_traces(trials, oracle, 3) on case `name`: every trial of every round up to the oracle's noise floor.  A round
    the oracle starts with no active edge has no trial to compare (compare_lm_traces insists on one): there `trials` has none either.
    Returns the number of trials compared, which is at least what the CPU test found for the case."""
    from conftest import compare_lm_traces
    o = oracle(name)
    n = 0
    for r in range(3):
        mine = [dict(x, round=0) for x in trials if x["round"] == r]
        if r in o["empty_rounds"]:
            assert not mine, "round %d: trials on a round without an active edge" % r
        else:
            n += compare_lm_traces(mine, [o["rounds"][r]], 1)
    assert n >= o["compared"]
    return n

