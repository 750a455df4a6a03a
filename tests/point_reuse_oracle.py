"""NumPy restatement of Tracking::PointReuse (tracking.cc:394-506) as include/nrs.h nrs_point_reuse states it, stage by stage:
1 project (nrs_frame_loop.se3f_act + project_f32), 2 candidates (the flag algebra, ascending map index), 4 the fp32 gate, 5/6 the
outputs and the list of new slots.  Stage 3, the tracking, is a callback -- the tests plug OracleBackend.reuse_track in.
tests/test_point_reuse_oracle_cpu.py pins this file to FrameLoop.point_reuse on the oracle backend, which is the oracle already."""
import numpy as np

import nrs_frame_loop as FL

F32 = np.float32


def project(pose, model, prm, map_pos):
    """stage 1: (pc, uv), float32"""
    map_pos = np.asarray(map_pos, F32).reshape(-1, 3)
    pc = FL.se3f_act((np.asarray(pose[0], F32), np.asarray(pose[1], F32)), map_pos)
    with np.errstate(all="ignore"):
        uv = FL.project_f32(model, prm, pc) if len(pc) else np.zeros((0, 2), F32)
    return pc, uv


def candidates(pc, uv, wh, frame_slot, slot_status, lost):
    """stage 2: the map indices of the candidates, ascending"""
    w, h = wh
    n = len(pc)
    frame_slot, slot_status = np.asarray(frame_slot, np.int64), np.asarray(slot_status, np.int64)
    with np.errstate(invalid="ignore"):
        inside = (uv[:, 0] >= 0) & (uv[:, 0] < w) & (uv[:, 1] >= 0) & (uv[:, 1] < h)      # (a NaN coordinate compares false)
        front = pc[:, 2] >= 0
    present = np.zeros(n, bool)
    held = frame_slot >= 0
    st = slot_status[frame_slot[held]]
    present[held] = (st == FL.TRACKED_WITH_3D) | (st == FL.JUST_TRIANGULATED)
    is_lost = np.zeros(n, bool)
    is_lost[np.asarray(sorted(int(x) for x in lost), np.int64)] = True
    return np.nonzero((is_lost | (~present & front)) & inside)[0]


def gate(seed_xy, xy, status):
    """stage 4: accepted, float32 element by element"""
    seed_xy, xy = np.asarray(seed_xy, F32).reshape(-1, 2), np.asarray(xy, F32).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        ex = seed_xy[:, 0] - xy[:, 0]
        ey = seed_xy[:, 1] - xy[:, 1]
        return (np.asarray(status) == FL.TRACKED_WITH_3D) & ~(ex * ex + ey * ey > F32(5.99))


def point_reuse(pose, model, prm, wh, map_pos, frame_slot, slot_status, lost, track, seeds=None):
    """track(cand, seed_xy) -> (xy, status).  seeds: None = the candidates' own projections; an (n_cand, 2) array = seeds taken from
    elsewhere (the device's), handed to the tracker and the gate in place of them -- the candidate set is this file's either way.
    Returns dict(cand_id, seed_xy, own_seed_xy, xy, status, accepted, n_reused, new_id, new_xy, n_new)."""
    pc, uv = project(pose, model, prm, map_pos)
    cand = candidates(pc, uv, wh, frame_slot, slot_status, lost)
    own = uv[cand].astype(F32)
    seed = own if seeds is None else np.asarray(seeds, F32).reshape(-1, 2)
    assert len(seed) == len(cand)
    if len(cand):
        xy, st = track(cand, seed)
        xy, st = np.asarray(xy, F32).reshape(-1, 2), np.asarray(st, np.int32)
    else:
        xy, st = np.zeros((0, 2), F32), np.zeros(0, np.int32)
    ok = gate(seed, xy, st)
    new = ok & (np.asarray(frame_slot, np.int64)[cand] < 0)
    return dict(cand_id=cand.astype(np.int32), seed_xy=seed, own_seed_xy=own, xy=xy, status=st, accepted=ok, n_reused=int(ok.sum()),
                new_id=cand[new].astype(np.int32), new_xy=xy[new], n_new=int(new.sum()))
