"""The evaluation entry points next to the pattern matcher (include/nrs.h "f7: evaluation") against tests/eval_oracle.py, bit for bit:
nrs_eval_depth_ground_truth, nrs_eval_frame and the LK stereo composition (nrs.stereo_lk)."""
import numpy as np
import pytest

import eval_oracle as E
import lk_oracle as LK
import nrs
import nrs_synth as S

pytestmark = pytest.mark.gpu
F32 = np.float32


def _depth(w, h, seed):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    return (3.0 + 0.8 * np.sin(xs / 17.0 + 0.2) * np.cos(ys / 13.0) + rng.normal(0, 0.01, (h, w))).astype(F32)


@pytest.mark.parametrize("model,wh", [(S.PINHOLE, (320, 240)), (S.KB8, (736, 552))], ids=["pinhole", "kb8"])
def test_depth_ground_truth_matches_the_oracle_bit_for_bit(ctx, model, wh):
    w, h = wh
    prm = S.HAMLYN_PINHOLE if model == S.PINHOLE else S.ENDOMAPPER_KB8
    depth = _depth(w, h, 5)
    depth[40, 50] = np.inf
    rng = np.random.default_rng(6)
    eps_x, eps_y = np.nextafter(F32(w - 1), F32(0)), np.nextafter(F32(h - 1), F32(0))
    xy = np.concatenate([
        np.stack([rng.uniform(0, w - 1, 60), rng.uniform(0, h - 1, 60)], 1),
        np.stack([rng.integers(0, w - 1, 8), rng.integers(0, h - 1, 8)], 1),          # integer positions: weights 1 0 0 0
        [[eps_x, 17.25], [33.5, eps_y], [eps_x, eps_y], [0, 0]],                        # the last cell that is still inside
        [[w - 1, 20], [20, h - 1], [w - 0.5, 3], [-0.25, 10], [10, -1e-3], [np.nan, 5]],  # rejected: last column / row, outside
        [[49.5, 39.5], [50, 40], [50.25, 40]],                                          # the cell with the infinite depth
    ]).astype(F32)
    gt, st = ctx.eval_depth_ground_truth(nrs.make_camera(model, prm), depth, xy)
    o_gt, o_st = E.depth_ground_truth(model, prm, depth, xy)
    assert np.array_equal(st, o_st)
    assert np.array_equal(gt.view(np.uint32)[o_st == 0], o_gt.view(np.uint32)[o_st == 0]) and np.isnan(gt[o_st != 0]).all()
    assert (st[-9:-3] == E.OUT_OF_BOUNDS).all() and (st[-3:] == E.BAD_DEPTH).all() and (st[:72] == E.OK).all()
    # a row-strided view of a wider image gives the same
    wide = np.full((h, w + 7), np.nan, F32)
    wide[:, :w] = depth
    gt2, st2 = ctx.eval_depth_ground_truth(nrs.make_camera(model, prm), wide[:, :w], xy)
    assert np.array_equal(st2, st) and gt2.tobytes() == gt.tobytes()


def _frame(n, seed, w=320, h=240):
    rng = np.random.default_rng(seed)
    prm = S.HAMLYN_PINHOLE
    depth = _depth(w, h, seed + 1)
    xy = np.stack([rng.uniform(5, w - 6, n), rng.uniform(5, h - 6, n)], 1).astype(F32)
    xy[0] = (w - 1, 10)                                             # one keypoint without ground truth
    q = np.array([0.02, -0.03, 0.01, 1.0])
    q = (q / np.linalg.norm(q)).astype(F32)
    t = np.array([0.1, -0.05, 0.2], F32)
    # world points whose camera-frame depth is the image depth / 1.3 plus noise
    z = np.array([depth[int(v), int(u)] for u, v in xy], np.float64) / 1.3 + rng.normal(0, 0.004, n)
    pc = np.stack([(xy[:, 0] - prm[2]) / prm[0] * z, (xy[:, 1] - prm[3]) / prm[1] * z, z], 1)
    x, y, zq, s = q.astype(np.float64)
    R = np.array([[1 - 2 * (y * y + zq * zq), 2 * (x * y - zq * s), 2 * (x * zq + y * s)],
                  [2 * (x * y + zq * s), 1 - 2 * (x * x + zq * zq), 2 * (y * zq - x * s)],
                  [2 * (x * zq - y * s), 2 * (y * zq + x * s), 1 - 2 * (x * x + y * y)]])
    X = ((pc - t.astype(np.float64)) @ R).astype(F32)
    return prm, depth, xy, q, t, X


def test_eval_frame_from_a_depth_image_matches_the_oracle_composition(ctx):
    prm, depth, xy, q, t, X = _frame(30, 11)
    r = ctx.eval_frame(nrs.make_camera(S.PINHOLE, prm), q, t, X, xy, depth=depth)
    gt, st = E.depth_ground_truth(S.PINHOLE, prm, depth, xy)
    rmse, scale, counts, gw = E.eval_frame(np.concatenate([q, t]), X, gt, st, True)
    assert r["rc"] == 0 and np.array_equal(r["gt_status"], st) and st[0] == E.OUT_OF_BOUNDS
    assert r["counts"] == tuple(counts) == (29, 29, 27)
    assert F32(r["rmse"]).tobytes() == F32(rmse).tobytes() and F32(r["scale"]).tobytes() == F32(scale).tobytes()
    assert np.array_equal(np.isnan(r["gt_world"]), np.isnan(gw)) and np.isnan(gw[0]).all()
    assert np.array_equal(r["gt_world"][1:].view(np.uint32), gw[1:].view(np.uint32))
    assert abs(float(scale) - 1.3) < 0.01 and float(rmse) < 0.02
    # the same frame with the ground truth handed in, as a stereo matcher would: the IQR gate is on, 0.9 inliers
    r2 = ctx.eval_frame(nrs.make_camera(S.PINHOLE, prm), q, t, X, xy, gt_xyz=gt, gt_status=st)
    rmse2, scale2, counts2, gw2 = E.eval_frame(np.concatenate([q, t]), X, gt, st, False)
    assert r2["counts"] == tuple(counts2) and counts2[2] == int(F32(counts2[1]) * F32(0.9))
    assert F32(r2["rmse"]).tobytes() == F32(rmse2).tobytes() and F32(r2["scale"]).tobytes() == F32(scale2).tobytes()
    assert np.array_equal(r2["gt_world"][1:].view(np.uint32), gw2[1:].view(np.uint32))
    # too few points with ground truth: no RMSE, NaN, and the statuses are still returned
    r3 = ctx.eval_frame(nrs.make_camera(S.PINHOLE, prm), q, t, X[:1], xy[:1], depth=depth)
    assert r3["rc"] == -1 and np.isnan(r3["rmse"]) and np.isnan(r3["scale"]) and r3["gt_status"][0] == E.OUT_OF_BOUNDS


def test_lk_stereo_composition_matches_the_lk_oracle_and_the_disparity_step():
    p = S.make_stereo_pair((160, 120), 8, (6, 0), 30, repeat=False)
    keep = [i for i, k in enumerate(p["kind"]) if k != "boundary"]
    xy = np.concatenate([p["xy"][keep], [[400.0, 60.0]]]).astype(F32)            # the last one is outside the image
    prm = np.array([383.19, 383.05, 80.0, 60.0], F32)
    c = nrs.Context()
    try:
        c.klt_configure(21, 2, 10, 1e-4, 1e-4)
        xyz, status, rxy, tst = nrs.stereo_lk(c, nrs.make_camera(0, prm), 2000.0, p["left"], p["right"], xy)
    finally:
        c.close()
    lk = LK.LucasKanadeOracle(21, 2, 10, 1e-4, 1e-4)
    lk.set_reference(p["left"], xy)
    oxy, ost, _, _ = lk.track(p["right"], xy.copy(), np.full(len(xy), 1, np.int32), initial_flow=True, min_ssim=0.5)
    o_xyz, o_status = E.stereo_from_tracks(prm, 2000.0, xy, oxy, ost)
    assert np.array_equal(tst, ost) and np.array_equal(status, o_status)
    assert np.array_equal(np.isnan(xyz), np.isnan(o_xyz))
    assert np.array_equal(xyz[o_status == 0].view(np.uint32), o_xyz[o_status == 0].view(np.uint32))
    assert (o_status == E.OK).sum() >= 10 and o_status[-1] == E.NOT_TRACKED
    # and the disparities are the planted ones where the tracker converged
    d = np.abs(xy[:-1, 0] - rxy[:-1, 0])[o_status[:-1] == 0]
    planted = p["disparity"][keep][o_status[:-1] == 0]
    assert np.median(np.abs(d - planted)) < 0.1
