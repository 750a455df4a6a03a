"""The frame-mapping cases of tests/map_cases.py as per-frame inserts of a TemporalBuffer (test infrastructure for the resident buffer,
include/nrs.h nrs_tbuf_*): tests/test_tbuf_cases_cpu.py vets the round trip on the CPU, tests/test_gpu_tbuf.py replays it on the device.

A flat case has rows; a TemporalBuffer has keypoint ids.  A relabelling gives row j the id ids[j] -- ascending in j, so that the
buffer's own order (ascending ids) is the case's row order -- and an order of the entries inside every snapshot:
  identity     id = row, entries in row order
  offset_gaps  ids from 1 000 000 upwards with gaps of 1 .. 130 between neighbours (rows straddle the 64-id words and the 1024-id trips of
               the device's row scan), entries of a snapshot shuffled
  reversed     id = 3 * row + 1, entries of a snapshot in descending row order

What a round trip cannot keep, by the rule of InsertSnapshotFromFrame itself (temporal_buffer.cc:31-34: only TRACKED_WITH_3D and TRACKED
slots enter): an entry of the LAST snapshot whose status is neither.  map_cases makes such entries (count_*, zero_zero turn candidates BAD
but leave their keypoint).  They are handed to insert all the same -- the caller passes its slots unfiltered -- and the filter drops them:
the row then has no keypoint in the last snapshot and its status is BAD either way.  No mapping kernel looks at a keypoint of the last
snapshot whose status is not 0 or 1 (candidates are status 1, their neighbours status 0), so the results are the flat case's; the CPU test
asserts exactly this difference and no other.  Rows that no snapshot holds drop out."""
import numpy as np

import nrs_frame_loop as FL

F32 = np.float32
RELABELS = ["identity", "offset_gaps", "reversed"]
_GAPS = np.array([1, 2, 63, 1, 65, 1, 1, 130, 1, 1, 7, 64, 1, 1, 1, 29], np.int64)


def relabel_ids(relabel, n):
    """the keypoint id of every row, ascending"""
    if relabel == "identity":
        return np.arange(n, dtype=np.int64)
    if relabel == "offset_gaps":
        return 1_000_000 + np.cumsum(_GAPS[np.arange(n) % len(_GAPS)])
    if relabel == "reversed":
        return 3 * np.arange(n, dtype=np.int64) + 1
    raise KeyError(relabel)


def _order(relabel, rows, f):
    if relabel == "identity":
        return rows
    if relabel == "reversed":
        return rows[::-1]
    return np.random.default_rng(1000 + f).permutation(rows)


def snapshots_of(cs, relabel):
    """cs: a case of map_cases (tb, deform_mag).  -> (ids of the rows, [dict(ids, xy, pos, status, has_lm, pose, mag)] oldest first): every
    snapshot holds the rows with a keypoint in it, unfiltered: in the last one the case's statuses, before it TRACKED_WITH_3D where the
    row has a landmark entry and TRACKED where not (the status of an older snapshot is never read)"""
    tb, mag = cs["tb"], np.asarray(cs["deform_mag"], F32)
    F, n = tb["has_kp"].shape
    ids = relabel_ids(relabel, n)
    snaps = []
    for f in range(F):
        rows = _order(relabel, np.nonzero(tb["has_kp"][f])[0], f)
        st = tb["status"][rows] if f == F - 1 else np.where(tb["has_lm"][f, rows], 0, 1)
        snaps.append(dict(ids=ids[rows], xy=np.asarray(tb["kp_xy"][f, rows], F32), pos=np.asarray(tb["lm_xyz"][f, rows], F32),
                          status=np.asarray(st, np.int32), has_lm=np.asarray(tb["has_lm"][f, rows], bool),
                          pose=np.asarray(tb["poses"][f], F32), mag=mag[f]))
    return ids, snaps


def host_flat(snaps, max_buffer_size=20):
    """nrs_frame_loop.TemporalBuffer fed the snapshots and flattened, with the landmark flags the reference does not have applied on top
    (an entry without one: has_lm clear, position zero).  -> (tb, deform_mag, ids) as TemporalBuffer.flat"""
    t = FL.TemporalBuffer(max_buffer_size)
    flags = []
    for s in snaps:
        t.insert(s["ids"], s["xy"], s["pos"], s["status"], s["pose"][:4], s["pose"][4:], s["mag"])
        keep = (s["status"] == 0) | (s["status"] == 1)
        has_lm = s.get("has_lm")
        flags.append((s["ids"][keep], np.ones(int(keep.sum()), bool) if has_lm is None else has_lm[keep]))
    flags = flags[len(flags) - len(t.snaps):]
    tb, mag, ids = t.flat(None, None)
    for f, (fid, fl) in enumerate(flags):
        j = np.searchsorted(ids, fid)
        tb["has_lm"][f, j] = fl
        tb["lm_xyz"][f, j[~fl]] = 0
    return tb, mag, ids


def held_rows(cs):
    """the rows of a case that survive the round trip, and the mask of the last snapshot's entries the filter drops"""
    tb = cs["tb"]
    dropped = tb["has_kp"][-1] & ~np.isin(tb["status"], (0, 1))
    has_kp = tb["has_kp"].copy()
    has_kp[-1] &= ~dropped
    return np.nonzero(has_kp.any(axis=0))[0], dropped
