"""GPU: Tracking::PointReuse as ONE call on the tracker's resident frame (include/nrs.h nrs_point_reuse; DESIGN.md 4 "PointReuse (one
call)").  The oracle is tests/point_reuse_oracle.py -- stages 1, 2 and 4 in NumPy, pinned to the oracle loop by
tests/test_point_reuse_oracle_cpu.py -- with OracleBackend.reuse_track (oracle/lk_oracle.py) as its tracker.  Comparisons are exact;
the one tolerance is on the KB8 seeds (double-precision atan2 / sin / cos of two libraries, rounded to float: at most 1 seed in 100 may
differ, none by more than 1 ulp), and the oracle's tracker is therefore fed the device's own seeds."""
import ctypes as C
import functools

import numpy as np
import pytest

import nrs
import nrs_frame_loop as FL
import nrs_synth as S
import point_reuse_oracle as PRO
import front_oracle as FO
from frame_loop_backend import OracleBackend, _get_template
import lk_oracle as LK

pytestmark = pytest.mark.gpu

F32 = np.float32
OPTS = dict(win=21, max_level=4, max_iters=10, epsilon=1e-4, min_eig=1e-4)
INVALID, STATE = -1, -5
OUT_IMAGE_BOUNDARIES = 4


def _oracle_templates(img, pts):
    lk = LK.LucasKanadeOracle(OPTS["win"], OPTS["max_level"], OPTS["max_iters"], OPTS["epsilon"], OPTS["min_eig"])
    lk.set_reference(img, np.asarray(pts, F32))
    return [_get_template(lk, i) for i in range(len(pts))]


def _never_filled():
    L = OPTS["max_level"] + 1
    return dict(xy=np.zeros(2, F32), gray=np.zeros((L, 21, 21), np.int16), grad=np.zeros((L, 21, 21, 2), np.int16), mean=np.zeros((L, 2), F32),
                valid=np.zeros(L, np.uint8))


def _ulps(a, b):
    return np.abs(np.asarray(a, F32).view(np.int32).astype(np.int64) - np.asarray(b, F32).view(np.int32).astype(np.int64))


def _against_oracle(ctx, model, prm, pose, wh, map_pos, frame_slot, slot_status, lost, img, tpl_of, insert_new=True):
    """one device call against the restatement; tpl_of: archive key -> oracle template (absent = never archived).  Returns (device, oracle)."""
    cam = nrs.make_camera(model, prm)
    n0 = ctx.klt_num_points()
    d = ctx.point_reuse(cam, pose[0], pose[1], wh, map_pos, frame_slot, slot_status, lost, 0.75, insert_new)
    pc, uv = PRO.project(pose, model, prm, map_pos)
    cand = PRO.candidates(pc, uv, wh, frame_slot, slot_status, lost)
    assert np.array_equal(d["cand_id"], cand), (d["cand_id"], cand)                 # the candidate set is identical in every case
    ob = OracleBackend(model, prm, OPTS)
    track = lambda c, seed: ob.reuse_track(img, seed, [tpl_of.get(int(mp)) or _never_filled() for mp in c], 0.75)
    o = PRO.point_reuse(pose, model, prm, wh, map_pos, frame_slot, slot_status, lost, track, seeds=d["seed_xy"])
    ul = _ulps(d["seed_xy"], o["own_seed_xy"]).max(1) if len(cand) else np.zeros(0, np.int64)
    print("n_cand %d  n_reused %d/%d  n_new %d/%d  seeds differing %d (max %d ulp)" % (
        d["n_cand"], d["n_reused"], o["n_reused"], d["n_new"], o["n_new"] if insert_new else 0, int((ul > 0).sum()), int(ul.max()) if len(ul) else 0))
    if model == S.PINHOLE:
        assert np.array_equal(d["seed_xy"], o["own_seed_xy"])
    else:
        assert (ul > 0).sum() * 100 <= len(ul) and (ul <= 1).all(), ul
    assert np.array_equal(d["xy"], o["xy"], equal_nan=True)
    assert np.array_equal(d["status"], o["status"]) and np.array_equal(d["accepted"], o["accepted"])
    assert d["n_reused"] == o["n_reused"] and d["n_new"] == (o["n_new"] if insert_new else 0)
    assert ctx.klt_num_points() == n0 + d["n_new"]
    return d, o


# ---- the call against the oracle on a frame-loop scene --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene(model):
    sq = S.make_frame_sequence(200, 3, 9 if model == S.PINHOLE else 12, model)
    n = sq["n_points"]
    held = np.arange(0, n, 2)                                      # the frame holds every other map point, slot j = map point 2 j
    frame_slot = np.full(n, -1, np.int32)
    frame_slot[held] = np.arange(len(held))
    slot_status = np.zeros(len(held), np.int32)
    slot_status[3::7] = FL.TRACKED
    slot_status[5::11] = FL.BAD
    lost = sorted(set(held[1::9].tolist()) | {1, 7})               # held points among them (status 0, 1 or 3), and two the frame lacks
    pose = (np.asarray(sq["pose_q"][2], F32), np.asarray(sq["pose_t"][2], F32))
    return dict(sq=sq, n=n, held=held, frame_slot=frame_slot, slot_status=slot_status, lost=lost, pose=pose)


def _scene_context(sc):
    """klt_set_reference on frame 0, every point archived under its map index, the frame's slots referenced, klt_track on frame 2"""
    sq, n, held = sc["sq"], sc["n"], sc["held"]
    ctx = nrs.Context()
    ctx.klt_configure(**OPTS)
    ctx.klt_set_reference(sq["images"][0], sq["kp0"])
    ctx.klt_archive_templates(np.arange(n), np.arange(n))
    ctx.klt_set_reference(sq["images"][0], sq["kp0"][held])
    ctx.klt_track(sq["images"][2], sq["kp0"][held], np.zeros(len(held), np.int32), initial_flow=True, min_ssim=0.7)
    return ctx


@pytest.mark.parametrize("model", [S.PINHOLE, S.KB8], ids=["pinhole", "kb8"])
def test_call_against_the_oracle(model):
    sc = _scene(model)
    sq = sc["sq"]
    tpl = dict(enumerate(_oracle_templates(sq["images"][0], sq["kp0"])))
    ctx = _scene_context(sc)
    try:
        d, o = _against_oracle(ctx, sq["model"], sq["prm"], sc["pose"], sq["wh"], sq["X0"], sc["frame_slot"], sc["slot_status"], sc["lost"],
                               sq["images"][2], tpl)
        held_lost = [i for i in sc["lost"] if sc["frame_slot"][i] >= 0]
        assert set(held_lost) <= set(d["cand_id"].tolist())        # (unless they left the image, which none does here)
        assert d["n_cand"] > sc["n"] // 2 and 0 < d["n_reused"] < d["n_cand"] and 0 < d["n_new"] < d["n_reused"]
        assert (d["status"] != FL.TRACKED_WITH_3D).any()
    finally:
        ctx.close()


def test_tracker_state_after_insert_new_equals_the_two_context_path():
    """consistency of the append: klt_num_points and the appended slots' templates, byte for byte, against reuse_track_archived +
    insert_archived (a two-level tracker in a second context, the gate on the host) on the same inputs"""
    sc = _scene(S.PINHOLE)
    sq = sc["sq"]
    a, b, b2 = _scene_context(sc), _scene_context(sc), nrs.Context()
    try:
        cam = nrs.make_camera(sq["model"], sq["prm"])
        n0 = a.klt_num_points()
        d = a.point_reuse(cam, sc["pose"][0], sc["pose"][1], sq["wh"], sq["X0"], sc["frame_slot"], sc["slot_status"], sc["lost"], 0.75, True)
        b2.klt_configure(OPTS["win"], 1, OPTS["max_iters"], OPTS["epsilon"], OPTS["min_eig"])
        b2.klt_insert_archived(b, d["cand_id"], d["seed_xy"])
        xy, st, _, _ = b2.klt_track(sq["images"][2], d["seed_xy"], np.zeros(d["n_cand"], np.int32), initial_flow=True, min_ssim=0.75)
        ok = PRO.gate(d["seed_xy"], xy, st)
        new = ok & (sc["frame_slot"][d["cand_id"]] < 0)
        b.klt_insert_archived(b, d["cand_id"][new], xy[new])
        assert np.array_equal(xy, d["xy"], equal_nan=True) and np.array_equal(st, d["status"]) and np.array_equal(ok, d["accepted"])
        assert d["n_new"] == int(new.sum()) > 0
        assert a.klt_num_points() == b.klt_num_points() == n0 + d["n_new"]
        ta, tb = a.klt_get_templates(n0, d["n_new"]), b.klt_get_templates(n0, d["n_new"])
        for x, y in zip(ta, tb):
            for k in ("xy", "gray", "grad", "mean", "valid"):
                assert x[k].tobytes() == y[k].tobytes(), k
        # ... and the slots the frame had are untouched
        for x, y in zip(a.klt_get_templates(0, n0), b.klt_get_templates(0, n0)):
            for k in ("xy", "gray", "grad", "mean", "valid"):
                assert x[k].tobytes() == y[k].tobytes(), k
    finally:
        a.close(); b.close(); b2.close()


# ---- smallest shapes: a hand-made 96 x 80 textured pair, the second image the first moved one pixel to the right -----------------
W, H = 96, 80
PRM = np.array([64, 64, 48, 40, 0, 0, 0, 0], F32)                 # pinhole: uv of (x, y, 2) is (32 x + 48, 32 y + 40), exact
POSE = (np.array([0, 0, 0, 1], F32), np.zeros(3, F32))
P = np.array([[30.25, 30.5], [48, 40], [60.75, 45.25], [40.5, 52], [66, 28.75], [35, 44.5]], F32)      # template positions


def _pair(w, h, seed):
    rng = np.random.default_rng(seed)
    tex = np.clip(np.rint(S._texture(h, w + 1, rng, 0)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(tex[:, 1:]), np.ascontiguousarray(tex[:, :w])


def _X(uv, prm=PRM, z=2.0):
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    return np.stack([(uv[:, 0] - prm[2]) / prm[0] * z, (uv[:, 1] - prm[3]) / prm[1] * z, np.full(len(uv), z)], 1).astype(F32)


class _Small:
    """a context referenced on image A at P and tracked on image B (so the resident pyramid is B's); oracle templates of the same slots"""

    def __init__(self, w=W, h=H, pts=P, seed=5):
        self.a, self.b = _pair(w, h, seed)
        self.wh, self.pts = (w, h), pts
        self.ctx = nrs.Context()
        self.ctx.klt_configure(**OPTS)
        self.ctx.klt_set_reference(self.a, pts)
        self.ctx.klt_track(self.b, pts, np.zeros(len(pts), np.int32), initial_flow=True, min_ssim=0.7)
        self.tpl_slot = _oracle_templates(self.a, pts)
        self.tpl = {}

    def archive(self, keys):
        """key keys[j] <- slot j mod len(pts)"""
        slots = [j % len(self.pts) for j in range(len(keys))]
        self.ctx.klt_archive_templates(slots, keys)
        for s, k in zip(slots, keys):
            self.tpl[int(k)] = self.tpl_slot[s]
        return slots

    def check(self, map_pos, frame_slot, slot_status, lost, model=S.PINHOLE, prm=PRM, insert_new=True):
        return _against_oracle(self.ctx, model, prm, POSE, self.wh, np.asarray(map_pos, F32), np.asarray(frame_slot, np.int32),
                               np.asarray(slot_status, np.int32), lost, self.b, self.tpl, insert_new)[0]


@pytest.fixture(scope="module")
def small():
    s = _Small()
    yield s
    s.ctx.close()


def test_one_point_as_a_candidate_and_one_point_held(small):
    small.archive([0])
    d = small.check(_X(P[0]), [-1], [], [])
    assert d["n_cand"] == 1 and d["accepted"].all() and d["n_new"] == 1
    assert abs(d["xy"][0, 0] - (P[0, 0] + 1)) < 0.2 and abs(d["xy"][0, 1] - P[0, 1]) < 0.2      # it did follow the one-pixel shift
    n0 = small.ctx.klt_num_points()
    d = small.check(_X(P[0]), [0], [FL.TRACKED_WITH_3D], [])
    assert d["n_cand"] == 0 and d["n_reused"] == 0 and small.ctx.klt_num_points() == n0
    d = small.check(_X(P[0]), [0], [FL.JUST_TRIANGULATED], [])    # a held slot that was just triangulated is present as well
    assert d["n_cand"] == 0 and small.ctx.klt_num_points() == n0
    d = small.check(_X(P[0]), [-1], [], [], insert_new=False)      # without insert_new the tracker is left alone
    assert d["n_cand"] == 1 and d["n_reused"] == 1 and d["n_new"] == 0 and small.ctx.klt_num_points() == n0


@pytest.mark.parametrize("n_map,idx", [(257, [0, 64, 256]), (1025, [0, 256, 1024]), (2050, [0, 1024, 2048, 2049])])
def test_candidate_order_across_waves_and_chunks(small, n_map, idx):
    """the compaction walks the map in chunks of 1024 threads = 16 waves: a candidate that is the first element of a later wave (64, 256),
    of a later chunk (1024, 2048), and the last point"""
    slots = small.archive(idx)
    map_pos = np.tile(np.array([[0.05, 0.05, 2]], F32), (n_map, 1))
    frame_slot = np.arange(n_map)
    map_pos[idx] = _X(P[slots])
    frame_slot[idx] = -1
    d = small.check(map_pos, frame_slot, np.zeros(n_map, np.int32), [])
    assert d["cand_id"].tolist() == idx and d["accepted"].all() and d["n_new"] == len(idx)


def test_z_and_lost_rules(small):
    small.archive([0])
    behind = _X(P[0], z=-2.0)                                      # z < 0, projects onto P[0]
    d = small.check(behind, [-1], [], [0])
    assert d["n_cand"] == 1 and np.array_equal(d["seed_xy"][0], P[0])
    d = small.check(behind, [-1], [], [])
    assert d["n_cand"] == 0
    kb8 = np.array([20, 20, 48, 40, 0, 0, 0, 0], F32)              # z = 0: theta = pi / 2, a finite uv inside the image
    d = small.check([[1.0, 0.5, 0.0]], [-1], [], [], model=S.KB8, prm=kb8)
    assert d["n_cand"] == 1 and np.isfinite(d["seed_xy"]).all()


def test_image_border(small):
    small.archive([0, 1, 2, 3])
    map_pos = np.array([[-1.5, 0, 2], [1.5, 0, 2], [0, 1.234375, 2], [np.nan, 0, 2]], F32)      # u = 0, u = w, v = h - 0.5, NaN
    d = small.check(map_pos, [-1, -1, -1, -1], [], [3])
    assert d["cand_id"].tolist() == [0, 2]
    assert d["seed_xy"][0, 0] == 0 and d["seed_xy"][1, 1] == H - 0.5 and not d["accepted"].any()


def test_key_that_was_never_archived(small):
    small.archive([0])
    n_map = 5001                                                   # key 7: inside the archive, nothing under it (no test of this module archives it); key 5000: beyond it
    map_pos = np.tile(np.array([[0.05, 0.05, 2]], F32), (n_map, 1))
    frame_slot = np.arange(n_map)
    map_pos[[7, 5000]] = _X(P[:2])
    frame_slot[[7, 5000]] = -1
    n0 = small.ctx.klt_num_points()
    d = small.check(map_pos, frame_slot, np.zeros(n_map, np.int32), [])
    assert d["cand_id"].tolist() == [7, 5000] and (d["status"] == OUT_IMAGE_BOUNDARIES).all() and not d["accepted"].any()
    assert d["n_new"] == 0 and small.ctx.klt_num_points() == n0


def test_single_level_pyramid():
    """40 x 64: the next level would be 20 wide, so the pyramid has one level and the top level is 0"""
    s = _Small(40, 64, np.array([[20, 32], [18.5, 30.25], [21.25, 34]], F32), seed=8)
    try:
        s.archive([0, 1, 2])
        prm = np.array([64, 64, 20, 32, 0, 0, 0, 0], F32)
        d = s.check(_X(s.pts, prm), [-1, -1, -1], [], [], prm=prm)
        assert d["n_cand"] == 3 and d["accepted"].any()
    finally:
        s.ctx.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _raw(ctx, **over):
    """nrs_point_reuse through ctypes with a valid two-point call's arguments, some replaced; (code, message)"""
    a = dict(cam=nrs.make_camera(S.PINHOLE, PRM), qt=np.array([0, 0, 0, 1, 0, 0, 0], F32), w=W, h=H, n_map=2, map_pos=_X(P[:2]),
             frame_slot=np.array([-1, 0], np.int32), n_slots=1, slot_status=np.zeros(1, np.int32), n_lost=1, lost=np.array([1], np.int32))
    a.update(over)
    cap = max(int(a["n_map"]), 1)
    outs = dict(n_cand=C.c_int32(0), cand=np.zeros(cap, np.int32), seed=np.zeros((cap, 2), F32), xy=np.zeros((cap, 2), F32), st=np.zeros(cap, np.int32),
                acc=np.zeros(cap, np.int32), n_reused=C.c_int32(0), n_new=C.c_int32(0))
    for k in list(outs):
        if k in over:
            outs[k] = over[k]
    ptr = lambda v, t: None if v is None else (C.byref(v) if isinstance(v, C.c_int32) else v.ctypes.data_as(C.POINTER(t)))
    rc = ctx.lib.nrs_point_reuse(
        ctx.h, C.byref(a["cam"]) if a["cam"] is not None else None, ptr(a["qt"], C.c_float), C.c_int32(a["w"]), C.c_int32(a["h"]), C.c_int32(a["n_map"]),
        ptr(a["map_pos"], C.c_float), ptr(a["frame_slot"], C.c_int32), C.c_int32(a["n_slots"]), ptr(a["slot_status"], C.c_int32), C.c_int32(a["n_lost"]),
        ptr(a["lost"], C.c_int32), C.c_float(0.75), C.c_int32(1), ptr(outs["n_cand"], C.c_int32), ptr(outs["cand"], C.c_int32), ptr(outs["seed"], C.c_float),
        ptr(outs["xy"], C.c_float), ptr(outs["st"], C.c_int32), ptr(outs["acc"], C.c_int32), ptr(outs["n_reused"], C.c_int32), ptr(outs["n_new"], C.c_int32))
    return rc, ctx.lib.nrs_last_error(ctx.h).decode()


def test_refusals(small):
    small.archive([0, 1])
    fresh = nrs.Context()
    try:
        rc, msg = _raw(fresh)                                      # no pyramid has been built
        assert rc == STATE and "pyramid" in msg and fresh.klt_num_points() == 0
    finally:
        fresh.close()
    ctx = small.ctx
    n0 = ctx.klt_num_points()
    big = (1 << 20)
    cases = [(dict(w=W + 8), STATE, "size"), (dict(h=H - 1), STATE, "size"),
             (dict(cam=None), INVALID, "null"), (dict(qt=None), INVALID, "null"), (dict(map_pos=None), INVALID, "null"),
             (dict(frame_slot=None), INVALID, "null"), (dict(slot_status=None), INVALID, "null"), (dict(lost=None), INVALID, "null"),
             (dict(n_cand=None), INVALID, "null"), (dict(cand=None), INVALID, "null"), (dict(seed=None), INVALID, "null"), (dict(xy=None), INVALID, "null"),
             (dict(st=None), INVALID, "null"), (dict(acc=None), INVALID, "null"), (dict(n_reused=None), INVALID, "null"), (dict(n_new=None), INVALID, "null"),
             (dict(n_map=-1), INVALID, "negative"), (dict(n_slots=-1), INVALID, "negative"), (dict(n_lost=-1), INVALID, "negative"),
             (dict(frame_slot=np.array([-1, 1], np.int32)), INVALID, "frame_slot[1]"),
             (dict(lost=np.array([2], np.int32)), INVALID, "lost id 2"), (dict(lost=np.array([-1], np.int32)), INVALID, "lost id -1"),
             (dict(n_map=big, map_pos=np.zeros((big, 3), F32), frame_slot=np.full(big, -1, np.int32)), INVALID, "1048576")]
    for over, code, text in cases:
        rc, msg = _raw(ctx, **over)
        assert rc == code and text in msg, (over.keys(), rc, msg)
        assert ctx.klt_num_points() == n0
    rc, msg = _raw(ctx)                                            # the unmodified call is accepted
    assert rc == 0
    one = nrs.Context()                                            # an archive of one level: PointReuse's tracker needs two
    try:
        one.klt_configure(OPTS["win"], 0, OPTS["max_iters"], OPTS["epsilon"], OPTS["min_eig"])
        one.klt_set_reference(small.a, P[:2])
        one.klt_archive_templates([0, 1], [0, 1])
        rc, msg = _raw(one)
        assert rc == INVALID and "level" in msg and one.klt_num_points() == 2
    finally:
        one.close()


# ---- the frame loop with device_reuse=True against the oracle loop -----------------------------------------------------------------
def _run_loop(backend, sq, images, frames):
    proj = lambda pc: FL.project_f32(sq["model"], sq["prm"], pc)
    loop = FL.FrameLoop(backend, proj, sq["wh"], sq["scale"], sq["kp0"], sq["X0"], sq["graph"], sq["pose_q"][0], sq["pose_t"][0], images[0],
                        images_to_insert_keyframe=2)
    for f in range(1, frames):
        assert loop.track_image(images[f])
    return loop.log


@functools.lru_cache(maxsize=None)
def _loop_scene(n, frames, seed, model):
    sq = S.make_frame_sequence(n, frames, seed, model)
    return sq, _run_loop(OracleBackend(sq["model"], sq["prm"], OPTS), sq, sq["images"], frames)


@pytest.mark.parametrize("front", [False, True], ids=["grey", "front"])
@pytest.mark.parametrize("n,frames,seed,model", [(260, 5, 9, S.PINHOLE), (200, 4, 12, S.KB8)], ids=["pinhole", "kb8"])
def test_frame_loop_with_device_reuse_matches_the_oracle_loop(n, frames, seed, model, front):
    """front: the loop is handed RAW frames (three equal channels: their grey image is the sequence's), the oracle loop the grey ones"""
    sq, olog = _loop_scene(n, frames, seed, model)
    images = sq["images"]
    if front:
        images = [np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2)) for g in sq["images"]]
        assert all(np.array_equal(FO.to_gray(r), g) for r, g in zip(images, sq["images"]))
    gb = FL.GpuBackend(nrs, sq["model"], sq["prm"], OPTS, front=front, device_reuse=True)
    try:
        glog = _run_loop(gb, sq, images, frames)
        assert gb.n_device_reuse >= 1 and gb.n_device_reuse == frames - 1
        assert gb._ctx_reuse is None                               # the second context was never created
    finally:
        gb.close()
    assert any(L["keyframe"] for L in glog) and any(L["reused"] > 0 for L in glog)
    for f, (g, o) in enumerate(zip(glog, olog), 1):
        assert np.allclose(g["pose_q"], o["pose_q"], atol=2e-6, rtol=0), f
        assert np.allclose(g["pose_t"], o["pose_t"], atol=2e-5, rtol=0), f
        assert g["lost"] == o["lost"] and g["reused"] == o["reused"] and g["keyframe"] == o["keyframe"], f
        assert np.array_equal(g["status_by_map"], o["status_by_map"]), f
        assert np.allclose(g["pos_by_map"], o["pos_by_map"], atol=2e-4, rtol=0), f
        assert g["n_tracked"] == o["n_tracked"] and g["n_tracked"] > 0.8 * sq["n_points"]
        assert g["n_2d"] == o["n_2d"] and np.array_equal(g["kp_2d"], o["kp_2d"]), f
