"""Cases of tests/test_gpu_pack_golden.py and of tools/pack_hash_golden.py, which writes tests/golden/pack_hashes.json from them: the
smallest nrs_synth windows that reach each branch of the engine's problem construction (csrc/nrs_engine_plan.hpp, nrs_engine_setup.hpp,
nrs_engine_devpack.hpp, nrs_engine_skin.hpp).  record(case) uploads the window and returns what the file pins, as JSON values:
  hash      the 24 words of nrs_dba_pack_hash without word 21 (the path); `device_built` is word 21
  stats     dba_stats; skin_stats = dba_skin_stats on an embedded window
  trials    accepted, and the bit patterns of lambda, chi2 and the trial's chi2, for every trial of optimize(2)
  error     code and text, where the upload is refused
Sharded cases (thread ranks of one process, at most four) hold one such record per rank."""
import struct
import threading

import numpy as np

import nrs
import nrs_synth as S
import embedded_window_cases as W

JOIN_S = 120
# id -> (kind, window (arguments of make_dba_problem), world, switches)
CASES = {
    # device and host pack, one GPU (tests/test_gpu_devpack.py)
    "c2-device": ("plain", (5000, 20, 1), 1, {}),
    "c2-host": ("plain", (5000, 20, 1), 1, {"NRS_HOST_PACK": "1"}),
    "ragged-device": ("plain", (16000, 5, 17, S.PINHOLE, 0.3), 1, {}),
    "ragged-host": ("plain", (16000, 5, 17, S.PINHOLE, 0.3), 1, {"NRS_HOST_PACK": "1"}),
    # the fused path with its tile descriptors (2048 padded rows: the smallest window the device construction takes); host only: two
    # tile classes on the two-kernel path (the window and the path of tests/test_gpu_edge_cases.py test_ba_two_tile_classes_bit_identical)
    "fused-device": ("plain", (300, 4, 3), 1, {}),
    "fused-host": ("plain", (300, 4, 3), 1, {"NRS_HOST_PACK": "1"}),
    "two-classes-host": ("plain", (1500, 8, 75), 1, {"NRS_FUSED_MAX_ROWS": "0", "NRS_TILE_CUT_PCT": "60"}),
    # sharded, every rank recorded (the smallest SHAPES of tests/test_gpu_sharded_devpack.py)
    "shard2-device": ("plain", (600, 8, 47), 2, {}),
    "shard2-host": ("plain", (600, 8, 47), 2, {"NRS_HOST_PACK": "1"}),
    "shard4-device": ("plain", (600, 16, 45), 4, {}),
    "shard4-host": ("plain", (600, 16, 45), 4, {"NRS_HOST_PACK": "1"}),
    "shard4-full-vectors": ("plain", (600, 16, 45), 4, {"NRS_SHARD_FULL_VECTORS": "1"}),
    # the temporal-difference form on a communicator (host only): its boundary tiles are decided from extents widened by the rows' partners
    "shard2-dform-host": ("plain", (600, 8, 47), 2, {"NRS_DFORM": "1"}),
    # embedded window, host-built (the smallest of tests/embedded_window_cases.py): the skinned observations' set-up
    "embedded-host": ("embedded", 0, 1, {}),
    # a refusal: one spring from the first keyframe to the last, so that both ranks' ranges reach beyond the adjacent keyframes
    "far-edge-device": ("far-edge", (600, 8, 47), 2, {}),
    "far-edge-host": ("far-edge", (600, 8, 47), 2, {"NRS_HOST_PACK": "1"}),
}
_windows = {}


def _bits(x):
    return struct.pack("<d", x).hex()


def _window(kind, win):
    """upload arguments of a window; built once, shared and left unchanged"""
    key = (kind, win)
    if key in _windows:
        return _windows[key]
    if kind == "embedded":
        p, flag, nb = W.window(W.CASES[win], "nodes")
        e = nrs.dba_build_edges_embedded(p["kf_points"], flag, nb)
    else:
        n, k, seed = win[:3]
        p = S.make_dba_problem(n, k, seed, *win[3:4], **(dict(dropout=win[4]) if len(win) > 4 else {}))
        e = nrs.dba_build_edges(p["kf_points"], p["nbr"])
        if kind == "far-edge":
            first, last = np.flatnonzero(p["lm_kf"] == 0)[0], np.flatnonzero(p["lm_kf"] == k - 1)[-1]
            e = dict(e, sp_ij=np.concatenate([np.asarray(e["sp_ij"], np.int32).reshape(-1, 2), [[first, last]]]).astype(np.int32),
                     sp_d0=np.concatenate([np.asarray(e["sp_d0"], np.float32), [1.0]]).astype(np.float32))
    cam = nrs.make_camera(p["model"], p["prm"])
    qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
    _windows[key] = (p, e, cam, qt)
    return _windows[key]


def _record(c, kind, p, e, cam, qt):
    try:
        if kind == "embedded":
            c.dba_upload_embedded(cam, qt, S.embedded_window(p, e), e, p["scale"])
        else:
            c.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"])
    except nrs.NrsError as ex:
        return dict(error=dict(code=ex.code, text=str(ex)))
    h = c.dba_pack_hash()
    res = dict(hash=["%016x" % w for i, w in enumerate(h) if i != 21], device_built=int(h[21]), stats=c.dba_stats())
    if kind == "embedded":
        res["skin_stats"] = c.dba_skin_stats()
    tr = nrs.Trace(64)
    c.dba_optimize(2, tr)
    res["trials"] = [[int(t["accepted"]), _bits(t["lam"]), _bits(t["chi"]), _bits(t["chi_new"])] for t in tr.trials]
    return res


def record(name):
    """the record of a case: a dict on one GPU, a list with one dict per rank on a communicator"""
    kind, win, world, switches = CASES[name]
    p, e, cam, qt = _window(kind, win)
    for key, value in switches.items():
        nrs.debug_set(key, value)
    try:
        if world == 1:
            c = nrs.Context()
            try:
                return _record(c, kind, p, e, cam, qt)
            finally:
                c.close()
        group = nrs.LocalGroup(world)
        out, errs = [None] * world, []

        def main(r):
            c = nrs.Context()
            try:
                c.comm_init_local(group, r)
                out[r] = _record(c, kind, p, e, cam, qt)
            except Exception as ex:
                errs.append((r, ex))
                raise
            finally:
                c.close()                            # (also after a failure: the other ranks do not wait for this one)

        th = [threading.Thread(target=main, args=(r,), daemon=True) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(JOIN_S)
        assert not errs, errs
        assert not any(t.is_alive() for t in th) and all(o is not None for o in out), "a rank did not finish"
        group.close()
        return out
    finally:
        for key in switches:
            nrs.debug_set(key, None)
