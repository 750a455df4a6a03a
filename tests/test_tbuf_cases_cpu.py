"""CPU: the precondition tests/test_gpu_tbuf.py rests on.  Every case of tests/map_cases.py, cut into per-frame inserts (tests/tbuf_cases.py)
and flattened again the way nrs_frame_loop.TemporalBuffer flattens, is the case: has_kp, has_lm, the last statuses, and kp_xy / lm_xyz under
set flags -- under every relabelling, with the one difference InsertSnapshotFromFrame's own filter makes (tbuf_cases' docstring): an entry
of the last snapshot whose status is neither TRACKED_WITH_3D nor TRACKED is dropped.  Rows that no snapshot holds drop out.

NO_ROUND_TRIP names the cases that cannot be replayed, with the reason (at most two).  None needs it."""
import inspect

import numpy as np
import pytest

import map_cases as MC
import nrs
import nrs_frame_loop as FL
import tbuf_cases as TC

NO_ROUND_TRIP = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_skip_list_is_short_and_names_cases():
    assert len(NO_ROUND_TRIP) <= 2 and all(k in MC.CASES and v for k, v in NO_ROUND_TRIP.items())


def test_the_binding_lists_the_resident_buffer():
    for s in ("nrs_tbuf_create", "nrs_tbuf_destroy", "nrs_tbuf_clear", "nrs_tbuf_insert", "nrs_tbuf_info", "nrs_tbuf_flat", "nrs_map_frame_tbuf"):
        assert s in nrs.SYMBOLS
    assert all(hasattr(nrs.TBuf, m) for m in ("insert", "clear", "info", "flat", "map_frame", "close"))
    p = inspect.signature(FL.GpuBackend.__init__).parameters
    assert "device_tbuf" in p and p["device_tbuf"].default is False
    assert all(hasattr(FL.GpuBackend, m) for m in ("tbuf_reset", "tbuf_insert", "map_frame_resident"))


@pytest.mark.parametrize("relabel", TC.RELABELS)
@pytest.mark.parametrize("name", [c for c in MC.CASES if c not in NO_ROUND_TRIP])
def test_a_case_survives_the_round_trip(name, relabel):
    cs = MC.case(name)
    tb = cs["tb"]
    F, n = tb["has_kp"].shape
    ids, snaps = TC.snapshots_of(cs, relabel)
    assert len(snaps) == F and np.all(np.diff(ids) > 0) and ids[0] >= 0 and ids[-1] < 2**31
    assert ids[-1] - ids[0] + 1 <= 1 << 22                         # the span limit of nrs_tbuf_insert
    for s in snaps:                                                # the refusals of nrs_tbuf_insert do not apply
        keep = (s["status"] == 0) | (s["status"] == 1)
        assert len(np.unique(s["ids"][keep])) == int(keep.sum())
    flat, mag, fid = TC.host_flat(snaps)
    rows, dropped = TC.held_rows(cs)
    # rows that no snapshot holds drop out, the others keep their order
    assert np.array_equal(fid, ids[rows])
    assert flat["n_frames"] == F and _bits(flat["poses"]).tolist() == _bits(tb["poses"]).tolist()
    assert np.array_equal(_bits(mag), _bits(cs["deform_mag"]))
    want_kp, want_lm = tb["has_kp"][:, rows].copy(), tb["has_lm"][:, rows].copy()
    want_kp[-1] &= ~dropped[rows]
    want_lm[-1] &= ~dropped[rows]
    assert np.array_equal(flat["has_kp"], want_kp) and np.array_equal(flat["has_lm"], want_lm)
    # the dropped entries are BAD in the case already (GetTriangulationCandidatesIds and the neighbour search pass them over)
    assert np.array_equal(flat["status"], tb["status"][rows])
    assert np.all(tb["status"][dropped] == FL.BAD) and np.all(np.isin(tb["status"][tb["has_kp"][-1] & ~dropped], (0, 1)))
    assert np.all(tb["status"][~tb["has_kp"][-1]] == FL.BAD)
    assert np.array_equal(_bits(flat["kp_xy"])[want_kp], _bits(tb["kp_xy"][:, rows])[want_kp])
    assert np.array_equal(_bits(flat["lm_xyz"])[want_lm], _bits(tb["lm_xyz"][:, rows])[want_lm])
    assert np.all(_bits(flat["kp_xy"])[~want_kp] == 0) and np.all(_bits(flat["lm_xyz"])[~want_lm] == 0)
    # the candidates are the case's, row for row
    assert np.array_equal(fid[flat["status"] == 1], ids[np.nonzero(tb["status"] == 1)[0]])
