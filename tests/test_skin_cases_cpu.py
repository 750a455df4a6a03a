"""CPU: the node-selection cases of tests/skin_cases.py, vetted without a device -- the oracle's picks against a literal loop (small
cases) and against a restatement on the full distance matrix (every case), the tie structure the lattice is made for, the properties
that define the sampling, the refusals as the oracle states them; and nrs.skinned_status (pure NumPy) on four small frames."""
import numpy as np
import pytest

import nrs
import skin_cases as SC
import skin_oracle as K


@pytest.mark.parametrize("name", SC.CASES)
def test_oracle_picks_equal_the_restatements(name):
    c = SC.case(name)
    n = len(c["pos"])
    ok = np.ones(n, bool) if c["eligible"] is None else c["eligible"]
    assert c["picks"].dtype == np.int32 and len(c["picks"]) == c["m"] and n <= 2200
    if n <= 130:
        assert np.array_equal(c["picks"], SC.literal(c["pos"], c["m"], ok)), name
    dist = SC.sqdist_matrix(c["pos"])
    assert np.array_equal(c["picks"], SC.restatement(c["pos"], c["m"], c["eligible"], dist)), name
    # the defining properties: distinct, eligible, the lowest eligible row first, a cover radius that never grows (the radius of
    # pick k = its fp32 squared distance to the nearest earlier pick: the same numbers in the same operation order, so exactly)
    p = c["picks"]
    assert len(set(p.tolist())) == c["m"] and ok[p].all() and p[0] == np.nonzero(ok)[0][0]
    rad = np.array([dist[p[k], p[:k]].min() for k in range(1, c["m"])])
    assert not np.isnan(rad).any() and np.all(rad[1:] <= rad[:-1])


def test_sizes_cover_the_strides():
    for n in SC.SIZES:
        ms = [SC.case(nm)["m"] for nm in SC.CASES if nm.startswith("sizes_n%d_" % n)]
        assert ms == sorted({m for m in (1, 2, min(n, 70)) if m <= n}), n
        if n <= 65:
            assert n in ms                                            # every point a node, compared in pick order
    assert set(SC.SIZES) == {1, 2, 63, 64, 65, 1023, 1024, 1025, 2049}


def test_lattice_ties_at_every_reduction_level():
    c = SC.case("lattice")
    assert c["pos"].shape == (2197, 3) and c["m"] == 200 and c["picks"][0] == 0
    counts = SC.lattice_holds(c)
    print("lattice tie rounds:", counts)
    assert counts["rounds"] == 199
    per_thread = np.bincount(np.arange(2197) % SC.FPS_BLK)
    assert set(per_thread) == {2, 3}
    for name in ("lattice_masked", "lattice_one_wave"):
        m = SC.tie_rounds(SC.case(name))
        print(name, "tie rounds:", m)
        assert m["any_tie"] > 0
    el = SC.case("lattice_masked")["eligible"]
    assert 0.55 < el.mean() < 0.65
    el = SC.case("lattice_one_wave")["eligible"]
    rows = np.nonzero(el)[0]
    assert set((rows % SC.FPS_BLK) // SC.WAVE) == {15} and (rows < SC.FPS_BLK).any() and (rows >= SC.FPS_BLK).any()
    assert SC.tie_rounds(SC.case("lattice_one_wave"))["cross_wave"] == 0


def test_designed_picks():
    c = SC.case("coincident")
    assert np.array_equal(c["picks"], np.arange(1500))
    c = SC.case("coincident_masked")
    assert c["m"] == c["eligible"].sum() == 500 and np.array_equal(c["picks"], np.arange(0, 1500, 3))
    c = SC.case("late_first")
    assert len(c["pos"]) == 2049 and not c["eligible"][:1030].any() and c["eligible"][1030:].all() and c["picks"][0] == 1030
    assert c["m"] == c["eligible"].sum() and sorted(c["picks"].tolist()) == list(range(1030, 2049))
    # overflow: row 0 is ordinary; the eight far points lie at +inf from it and from each other, so they follow in ascending order
    c = SC.case("overflow")
    far = np.nonzero(np.abs(c["pos"]).max(1) > 1e19)[0]
    dist = SC.sqdist_matrix(c["pos"])
    assert len(far) == 8 and far[0] > 0 and np.isinf(dist[np.ix_(far, far)][~np.eye(8, dtype=bool)]).all() and np.isinf(dist[0, far]).all()
    assert not np.isnan(dist).any() and c["picks"][0] == 0 and np.array_equal(c["picks"][1:9], far) and c["m"] > 9
    # non-finite rows that are not eligible: they exist in both trips, and the picks are those of the cloud with them zeroed
    for name in ("nonfinite_nan_lost", "nonfinite_inf_lost", "nonfinite_minus_inf_lost"):
        c = SC.case(name)
        rows = np.nonzero(~np.isfinite(c["pos"]).all(1))[0]
        assert len(rows) == 6 and not c["eligible"][rows].any() and (rows < SC.FPS_BLK).any() and (rows >= SC.FPS_BLK).any()
        zeroed = c["pos"].copy()
        zeroed[rows] = 0
        assert np.array_equal(c["picks"], K.select_nodes(zeroed, c["m"], c["eligible"]))
        assert np.array_equal(c["picks"], K.select_nodes(c["pos"], c["m"], c["eligible"]))


@pytest.mark.parametrize("name", SC.REFUSALS)
def test_the_oracle_refuses_what_the_library_must(name):
    r = SC.refusal(name)
    with pytest.raises(ValueError) as e:
        K.select_nodes(r["pos"], r["m"], r["eligible"])
    ok = np.ones(len(r["pos"]), bool) if r["eligible"] is None else r["eligible"]
    bad = np.nonzero(ok & ~np.isfinite(r["pos"]).all(1))[0]
    if len(bad):
        assert "eligible point %d " % bad[0] in str(e.value) and r["words"][0] == "eligible point %d " % bad[0]
        assert np.isfinite(r["pos"][:bad[0]][ok[:bad[0]]]).all()
    else:
        assert ok.sum() < r["m"] <= len(r["pos"]) and "%d eligible" % ok.sum() in r["words"][1]
    SC.case(SC.GOOD_AFTER_REFUSAL)


def test_cases_are_read_only():
    c = SC.case("lattice")
    with pytest.raises(ValueError):
        c["pos"][0, 0] = 1
    with pytest.raises(ValueError):
        c["picks"][0] = 1


# ---- nrs.skinned_status: nodes keep 0, every other status-0 point of the frame becomes 1
def test_skinned_status_skips_entries_without_a_map_point():
    st = np.array([0, 0, 1, 0, 2, 0], np.int32)
    fm = np.array([4, -1, 2, 0, -1, 3], np.int32)
    out = nrs.skinned_status(st, fm, [4, 3])
    assert np.array_equal(out, [0, 0, 1, 1, 2, 0]) and out.dtype == np.int32     # (-1: not in the map, left as it is)
    assert np.array_equal(st, [0, 0, 1, 0, 2, 0])                                # the argument is not written


def test_skinned_status_with_an_empty_node_list():
    st = np.array([0, 1, 0, 3, 0], np.int32)
    fm = np.array([0, 1, 2, 3, 4], np.int32)
    assert np.array_equal(nrs.skinned_status(st, fm, np.zeros(0, np.int32)), [1, 1, 1, 3, 1])
    assert np.array_equal(nrs.skinned_status(st, fm, []), [1, 1, 1, 3, 1])


def test_skinned_status_with_nodes_outside_the_frame():
    st = np.array([0, 0, 0, 1], np.int32)
    fm = np.array([5, 2, 7, 3], np.int32)
    assert np.array_equal(nrs.skinned_status(st, fm, [2, 4, 6]), [1, 0, 1, 1])   # 4 and 6 are no points of this frame


def test_skinned_status_with_node_ids_above_the_frames_largest():
    st = np.array([0, 0, 2, 0], np.int32)
    fm = np.array([1, 3, 0, 2], np.int32)
    assert np.array_equal(nrs.skinned_status(st, fm, [3, 900, 12]), [1, 0, 2, 1])
    assert np.array_equal(nrs.skinned_status(st, fm, [900]), [1, 1, 2, 1])
