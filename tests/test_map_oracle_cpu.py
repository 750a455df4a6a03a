"""tests/map_oracle.py (the restatement of Mapping::LandmarkTriangulation) on the cases the device is held to in
tests/test_gpu_map.py: no gate of a committed case is decided by the last bits, and each case holds what it is meant to hold."""
import numpy as np
import pytest

import map_cases as MC
import map_oracle as M


@pytest.mark.parametrize("name", MC.CASES)
def test_no_gate_hangs_on_the_last_bit(name):
    """every gate quantity (reprojection errors against 5.991, parallax against both window ends, depths against 0, deform_mag against
    the rigidity threshold, neighbour distances against 20 and 500) is at least 16 fp32 ulp of itself away from its threshold"""
    cs = MC.case(name)
    exc = M.margin_exceptions(cs["gates"], 16)
    print(name, "gates", len(cs["gates"]), "inside the margin", len(exc), exc[:5])
    assert len(exc) == 0                                           # share of candidates excluded for sitting inside the margin: 0


def _counts(ref):
    return np.bincount(ref["rigid_status"], minlength=9), np.bincount(ref["deform_status"], minlength=12)


def test_rigid_case():
    ref = MC.case("rigid_f4")["ref"]
    r, d = _counts(ref)
    assert d[M.D_SHORT] == len(ref["cand"]) and ref["n_deformable"] == 0          # 4 snapshots: every track is short
    assert r[M.R_OK] >= 10 and r[M.R_PARALLAX] >= 1 and ref["mode"] == M.MODE_RIGID
    assert np.array_equal(ref["accepted_ids"], ref["cand"][ref["rigid_status"] == 0])   # the rigid successes, in id order


def test_all_deforming_case():
    ref = MC.case("all_deforming")["ref"]
    r, _ = _counts(ref)
    assert ref["n_rigid"] == 0 and r[M.R_NOT_RIGID] >= 10 and ref["n_deformable"] >= 10 and ref["mode"] == M.MODE_DEFORMABLE
    assert np.array_equal(ref["accepted_ids"], ref["cand"][ref["deform_status"] == 0])


def test_one_deforming_case():
    cs = MC.case("one_deforming")
    tb, ref, f = cs["tb"], cs["ref"], cs["tb"]["deforming_snapshot"]
    spans = np.array([M.feature_track(tb, int(c))[0] <= f for c in ref["cand"]])   # (every track ends in the last snapshot)
    close = ref["rigid_status"] == M.R_CLOSE
    assert np.array_equal(ref["rigid_status"][~close] == M.R_NOT_RIGID, spans[~close])   # exactly the tracks spanning it
    absent = [c for c in ref["cand"] if M.feature_track(tb, int(c))[0] < f and not tb["has_kp"][f, c]]
    assert absent and all(ref["rigid_status"][list(ref["cand"]).index(c)] == M.R_NOT_RIGID for c in absent)
    assert (ref["rigid_status"] == M.R_NOT_RIGID).sum() >= 10 and (~spans & ~close).sum() >= 5   # (the later, shorter tracks fail on parallax)


def test_kb8_case():
    ref = MC.case("kb8_f21")["ref"]
    r, d = _counts(ref)
    assert MC.case("kb8_f21")["tb"]["n_frames"] == 21 and r[M.R_OK] >= 10 and r[M.R_CLOSE] >= 1 and d[0] >= 10


def test_dead_band_and_zero_zero():
    ref = MC.case("dead_band")["ref"]
    nr, nd = ref["n_rigid"], ref["n_deformable"]
    assert nr > 0 and nd > 0 and not nr > 1.5 * nd and not nd >= 1.5 * nr
    assert ref["mode"] == M.MODE_NONE and len(ref["accepted_ids"]) == 0
    z = MC.case("zero_zero")["ref"]
    assert len(z["cand"]) >= 5 and z["n_rigid"] == 0 and z["n_deformable"] == 0
    assert z["mode"] == M.MODE_DEFORMABLE and len(z["accepted_ids"]) == 0


@pytest.mark.parametrize("count", [0, 1, 64, 65, 1025])
def test_candidate_counts(count):
    ref = MC.case("count_%d" % count)["ref"]
    assert len(ref["cand"]) == count
    if count == 1025:                                              # one above the 1024-thread scan: the compaction's carry is in use
        assert ref["mode"] == M.MODE_RIGID and len(ref["accepted_ids"]) >= 64
        assert (np.nonzero(ref["rigid_status"] == 0)[0] >= 1024 // 2).any()


def test_index_snapshot_drops_after_the_vote():
    a, b = MC.case("rigid_f4")["ref"], MC.case("index_snapshot")["ref"]
    assert (a["n_rigid"], a["n_deformable"], a["mode"]) == (b["n_rigid"], b["n_deformable"], b["mode"])
    assert 0 < len(b["accepted_ids"]) < len(a["accepted_ids"]) and set(b["accepted_ids"]) < set(a["accepted_ids"])


def test_planted_inputs():
    for name, code in (("bent", M.R_REPROJ_PREV), ("current_reproj", M.R_REPROJ_CUR), ("previous_reproj", M.R_REPROJ_PREV),
                       ("previous_depth", M.R_DEPTH_PREV)):
        cs = MC.case(name)
        k = list(cs["ref"]["cand"]).index(cs["tb"]["touched"])
        assert cs["ref"]["rigid_status"][k] == code, (name, cs["ref"]["rigid_status"][k])
    cs = MC.case("nan")
    ref, c = cs["ref"], cs["tb"]["touched"]
    k = list(ref["cand"]).index(c)
    # the reference's comparisons let a NaN through every gate: a rigid "success" that counts in the vote and is dropped at :214
    assert ref["rigid_status"][k] == 0 and np.isnan(ref["rigid_xyz"][k]).all() and c not in ref["accepted_ids"]
    assert ref["n_rigid"] == MC.case("rigid_f4")["ref"]["n_rigid"]
