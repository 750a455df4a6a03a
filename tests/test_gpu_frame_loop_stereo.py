"""GPU: System::TrackImageWithStereo in the frame loop (FrameLoop.track_image_with_stereo) on the resident stereo pair, against the host path
it replaces.  The sequence is tests/test_gpu_stereo_init_loop.py's (nrs_synth.make_stereo_init_sequence, 320 x 240, three frames; the
generator makes one right view, which serves every frame: the camera moves 0.35 mm per frame, a fraction of a disparity step).

  resident  front-mode backend: ONE nrs_front_process_stereo per stereo frame, Shi-Tomasi / init_stereo / LK / the pattern matcher of the
            evaluation all on the resident eyes;
  host      front-mode backend fed the raw left frames through nrs_front_process; the grey bytes of both eyes are downloaded (a helper
            context) and go up again into the host-pointer nrs_init_stereo / nrs_stereo_match_pattern; track_image per frame.
The same kernels run on the same bytes, so poses, statuses, positions and the evaluation's records must agree bit for bit."""
import numpy as np
import pytest

import nrs
import nrs_frame_loop as FL
import nrs_synth as S
from map_loop_backend import OPTS, RAD_PER_PIXEL

pytestmark = pytest.mark.gpu
F32 = np.float32
MAX_FEATURES = 250


def _thin(xy):
    xy = np.asarray(xy, F32).reshape(-1, 2)
    return xy[(np.arange(MAX_FEATURES) * len(xy)) // MAX_FEATURES] if len(xy) > MAX_FEATURES else xy


def _loop(b, sq, r):
    proj = lambda pc: FL.project_f32(sq["model"], sq["prm"], pc)
    return FL.FrameLoop.from_stereo_initialization(b, proj, sq["wh"], r, sq["images"][0], mapping=True, rad_per_pixel=RAD_PER_PIXEL,
                                                   camera=(sq["model"], sq["prm"]))


def test_track_image_with_stereo_equals_the_host_path():
    sq = S.make_stereo_init_sequence()
    frames = [1, 2]
    rights = {f: sq["right"].copy() for f in [0] + frames}            # a fresh array per frame, as a grabber hands them out
    opts = dict(bf=sq["bf"], z_min=sq["z_min"], z_max=sq["z_max"], eps=sq["eps"], min_points=sq["min_points"])
    rb = FL.GpuBackend(nrs, sq["model"], sq["prm"], OPTS, dense_graph=True, front=True)
    hb = FL.GpuBackend(nrs, sq["model"], sq["prm"], OPTS, dense_graph=True, front=True)
    aux = nrs.Context()
    try:
        # ---- resident: the pair goes up once, everything else reads it where it lies
        left0 = sq["images"][0]
        rb.front_stereo(left0, rights[0])
        xy = _thin(rb.extract_features(left0, None, None)[0])
        r = rb.init_stereo(left0, rights[0], xy, **opts)
        rl = _loop(rb, sq, r)
        assert rb.n_front_calls == 1                                # extraction, initialisation and SetReferenceImage on one processed pair
        for f in frames:
            assert rl.track_image_with_stereo(sq["images"][f], rights[f], evaluate=True, matcher="pattern", bf=sq["bf"])
        assert rb.n_front_calls == 1 + len(frames)                  # exactly one front-end call per stereo frame
        # ---- host: raw frame -> nrs_front_process, grey bytes down and up again
        gray = lambda im: aux.front_process(im, outputs=("gray",))["gray"]
        hxy = _thin(hb.extract_features(left0, None, None)[0])
        assert np.array_equal(hxy, xy)
        h = hb.ctx.init_stereo(hb.cam, gray(left0), gray(rights[0]), hxy, **opts)
        h["selected_keypoints"] = hxy[h["selected"]].copy()
        assert set(h) == set(r)
        for k in r:
            assert np.array_equal(np.asarray(r[k]), np.asarray(h[k]), equal_nan=True), k
        assert r["verdict"] == 0 and r["n_selected"] >= 100
        hl = _loop(hb, sq, h)
        h_rmse = []
        for f in frames:
            assert hl.track_image(sq["images"][f])
            slots = np.nonzero(hl.status == FL.TRACKED_WITH_3D)[0]
            gt, st, _, _ = hb.ctx.stereo_match_pattern(hb.cam, sq["bf"], gray(sq["images"][f]), gray(rights[f]), hl.kp[slots])
            e = hb.eval_frame(hl.pose[0], hl.pose[1], hl.pos[slots], hl.kp[slots], gt_xyz=gt, gt_status=st)
            h_rmse.append(dict(rmse=e["rmse"], scale=e["scale"], counts=e["counts"], n=len(slots), rc=e["rc"]))
        # ---- the same bits
        assert len(rl.log) == len(hl.log) == len(frames)
        for a, b in zip(rl.log, hl.log):
            for k in ("pose_q", "pose_t", "pos_by_map", "kp_2d"):
                assert a[k].tobytes() == b[k].tobytes(), k
            assert np.array_equal(a["status_by_map"], b["status_by_map"]) and np.array_equal(a["status_after_mapping"], b["status_after_mapping"])
            for k in ("lost", "reused", "n_tracked", "keyframe", "n_2d", "map_size", "mapping"):
                assert a[k] == b[k], k
        assert rl.map_pos.tobytes() == hl.map_pos.tobytes() and rl.kp.tobytes() == hl.kp.tobytes() and np.array_equal(rl.status, hl.status)
        assert len(rl.rmse) == len(h_rmse) == len(frames)
        for a, b in zip(rl.rmse, h_rmse):
            print("rmse", a["rmse"], "scale", a["scale"], "counts", tuple(a["counts"]), "n", a["n"], "rc", a["rc"])
            assert F32(a["rmse"]).tobytes() == F32(b["rmse"]).tobytes() and F32(a["scale"]).tobytes() == F32(b["scale"]).tobytes()
            assert tuple(a["counts"]) == tuple(b["counts"]) and a["n"] == b["n"] and a["rc"] == b["rc"]
        assert rl.rmse[0]["rc"] == 0 and rl.rmse[0]["counts"][0] > 20       # the evaluation did have ground truth to score against
        # evaluate() alone after the frame: the resident pair again, nothing is processed
        n = rb.n_front_calls
        again = rl.evaluate(right=rights[frames[-1]], bf=sq["bf"])
        assert rb.n_front_calls == n and F32(again["rmse"]).tobytes() == F32(rl.rmse[-2]["rmse"]).tobytes()
        # the LK stereo matcher: the backend's stereo context tracks on the pair resident in the main context (nrs_stereo_match_lk_front);
        # host path: nrs.stereo_lk on the downloaded grey bytes in a tracker context of its own.  The main tracker's templates stay
        f = frames[-1]
        n_tpl, tpl = rb.ctx.klt_num_points(), rb.ctx.klt_get_templates(0, 1)[0]
        lk = rl.evaluate(right=rights[f], matcher="lk", bf=sq["bf"])
        assert rb.n_front_calls == n and rb.ctx.klt_num_points() == n_tpl
        for k, v in rb.ctx.klt_get_templates(0, 1)[0].items():
            assert np.array_equal(v, tpl[k], equal_nan=True), k
        cs = nrs.Context()
        try:
            cs.klt_configure(OPTS["win"], OPTS["max_level"], OPTS["max_iters"], OPTS["epsilon"], OPTS["min_eig"])
            slots = np.nonzero(hl.status == FL.TRACKED_WITH_3D)[0]
            gt, st, _, tst = nrs.stereo_lk(cs, hb.cam, sq["bf"], gray(sq["images"][f]), gray(rights[f]), hl.kp[slots])
        finally:
            cs.close()
        e = hb.eval_frame(hl.pose[0], hl.pose[1], hl.pos[slots], hl.kp[slots], gt_xyz=gt, gt_status=st)
        print("lk rmse", lk["rmse"], "counts", tuple(lk["counts"]), "tracked by the matcher", int((tst == 1).sum()), "of", len(slots))
        assert F32(lk["rmse"]).tobytes() == F32(e["rmse"]).tobytes() and F32(lk["scale"]).tobytes() == F32(e["scale"]).tobytes()
        assert tuple(lk["counts"]) == tuple(e["counts"]) and lk["rc"] == e["rc"] and lk["n"] == len(slots)
        assert (tst == 1).any()                                     # the matcher did track: the comparison covers something
    finally:
        rb.close()
        hb.close()
        aux.close()


def test_track_image_with_stereo_needs_the_front_mode():
    p = S.make_stereo_pair((96, 64), 3, (0, 8), 40)
    b = FL.GpuBackend(nrs, 0, np.array([383.19, 383.05, 155.97, 124.34], F32), OPTS)
    try:
        with pytest.raises(ValueError):
            b.front_stereo(p["left"], p["right"])
        r = b.init_stereo(p["left"], p["right"], p["xy"], bf=400.0)              # without it nothing changes: the host-pointer form
        assert r["n_matched"] > 0 and b.n_front_calls == 0
    finally:
        b.close()
