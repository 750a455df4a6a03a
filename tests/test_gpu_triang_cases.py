"""GPU parity: k_triangulate (csrc/nrs_triang.hip) against oracle/triang_oracle.py on the designed cases of tests/triang_cases.py, which
tests/test_triang_cases_cpu.py vets first: every exit code is reached, the neighbour list is probed at its ties, its limits and its
11th place, tracks of 1, 2 and 21 (gappy) vertices, buffers of 1 and 2 snapshots, and a problem without a single regulariser edge.

Held: statuses identical; a failed candidate's position exactly zero; the regulariser edge count (dbg[:, 3]) equal to the oracle's for
every candidate that got past the seeds -- in the neighbour cases every potential neighbour carries another count, so this is the
neighbour SET; positions of OK candidates within the 2e-3 of tests/test_gpu_triang.py and their pooled median within its 1e-4 (same
scene, same basis: the LM runs on g2o's numeric Jacobian); where no solve of the LM can succeed (no regulariser edge),
the iteration and trial counts equal to the oracle's and the position equal bit for bit (nothing moved: the fp32 twin path alone).
The same buffers through nrs_map_frame (the `close_bits` form of the kernel) give the batch call's statuses and position bits."""
import numpy as np
import pytest

import nrs
import triang_cases as TC
import triang_oracle as T

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _run(ctx, cs):
    tb = cs["tb"]
    cam = nrs.make_camera(tb["model"], tb["prm"])
    return cam, ctx.triangulate_batch(cam, tb, cs["cand"], cs["min_track"], debug=True)


def _held_to_the_oracle(name, cs, st, xyz, dbg):
    """the comparisons of one case; returns the position errors of its OK candidates"""
    ref = cs["ref"]
    rst = np.array([r["status"] for r in ref])
    rxyz = np.array([r["xyz"] for r in ref])
    assert np.array_equal(st, rst), (name, [T.STATUS_TEXT[s] for s in st], [T.STATUS_TEXT[s] for s in rst])
    assert np.all(xyz[st != 0] == 0)
    for k, r in enumerate(ref):
        if r["edges"] is None:                                     # stopped at a gate or a seed: the kernel wrote no debug row
            assert np.all(dbg[k] == 0), (name, k, dbg[k])
            continue
        assert dbg[k, 3] == r["edges"], (name, k, dbg[k], r["edges"])
        if r["all_failed"]:
            assert (dbg[k, 1], dbg[k, 2]) == (r["iters"], r["trials"]), (name, k, dbg[k], r["iters"], r["trials"])
            assert np.array_equal(_bits(xyz[k]), _bits(r["xyz"])), (name, k, xyz[k], r["xyz"])
        else:
            assert 1 <= dbg[k, 1] <= 10 and dbg[k, 1] <= dbg[k, 2] <= 100
    ok = st == 0
    err = np.linalg.norm(xyz[ok].astype(np.float64) - rxyz[ok], axis=1)
    print(name, "positions of OK candidates: disagreement", err)
    assert np.all(err <= 2e-3), (name, err)
    return err


@pytest.mark.parametrize("name", TC.CASES)
def test_case_matches_the_oracle(ctx, name):
    """`no_edges`, `track_1`, `frames_1`: the first Cholesky fails, and the update and the gain ratio of that trial read dx.  The kernel
    zeroes dx before the LM loop (g2o's solution vector starts at zero and a failed solve leaves it).  Without that it read LDS the
    workgroup never wrote; what the LDS holds at launch cannot be set from here, so these cases pin the right answer (1 iteration, 10
    trials, the seed's bits) but cannot be relied on to fail on a kernel without the zeroing."""
    cs = TC.case(name)
    tb = cs["tb"]
    cam, (st, xyz, dbg) = _run(ctx, cs)
    _held_to_the_oracle(name, cs, st, xyz, dbg)
    # the same candidates through frame mapping, every snapshot deforming: the rigid leg refuses all, the deformable leg is voted
    F = tb["n_frames"]
    r = ctx.map_frame(cam, tb, np.full(F, 0.006, np.float32), float(1.0 / tb["prm"][0]), rigidity_th=0.004, min_track=cs["min_track"])
    assert np.array_equal(r["cand"], cs["cand"]) and r["n_rigid"] == 0 and r["mode"] == 2
    assert np.array_equal(r["deform_status"], st), (name, r["deform_status"], st)
    assert np.array_equal(_bits(r["deform_xyz"]), _bits(xyz))
    assert np.array_equal(r["accepted_ids"], cs["cand"][st == 0]) and np.array_equal(_bits(r["accepted_xyz"]), _bits(xyz[st == 0]))


def test_refusals_leave_the_context_usable(ctx):
    cs = TC.case("half_bad_neighbours")
    tb = cs["tb"]
    cam = nrs.make_camera(tb["model"], tb["prm"])
    n = tb["has_kp"].shape[1]
    none = dict(tb, n_frames=0)
    long = dict(tb, n_frames=22)                                   # 22 snapshots: the oldest one repeated in front
    for k in ("poses", "has_kp", "kp_xy", "has_lm", "lm_xyz"):
        none[k] = tb[k][:0]
        long[k] = np.concatenate([tb[k][:1]] * 17 + [tb[k]])
    assert long["has_kp"].shape == (22, n) and none["has_kp"].shape == (0, n)
    with pytest.raises(nrs.NrsError, match="at most 21"):
        ctx.triangulate_batch(cam, none, cs["cand"], 5)
    with pytest.raises(nrs.NrsError, match="at most 21"):
        ctx.triangulate_batch(cam, long, cs["cand"], 5)
    with pytest.raises(nrs.NrsError, match="out of range"):
        ctx.triangulate_batch(cam, tb, [-1], 5)
    with pytest.raises(nrs.NrsError, match="unknown camera model"):
        ctx.triangulate_batch(nrs.make_camera(7, tb["prm"]), tb, cs["cand"], 5)
    st, xyz, dbg = _run(ctx, cs)[1]
    _held_to_the_oracle("half_bad_neighbours", cs, st, xyz, dbg)


def test_pooled_position_error(ctx):
    """every case once more, in one go: the OK candidates' disagreement with the oracle, pooled, has the median of tests/test_gpu_triang.py"""
    err = []
    for name in TC.CASES:
        cs = TC.case(name)
        st, xyz, dbg = _run(ctx, cs)[1]
        err.append(_held_to_the_oracle(name, cs, st, xyz, dbg))
    err = np.concatenate(err)
    print("pooled over", len(err), "OK candidates: max", err.max(), "median", np.median(err))
    assert len(err) >= 20 and err.max() <= 2e-3 and np.median(err) <= 1e-4
