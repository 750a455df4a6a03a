"""CPU: the oracle of the stereo map initialisation (tests/stereo_init_oracle.py) against a second statement of the same rules, and the
stand-alone check of the library's host half.

The device is written to the fixed-point definition of the clustering (components of the core points; a border point takes the lowest raw
label among its core neighbours), the oracle is the textbook sequential algorithm (index order, a queue per cluster, a border point is kept
by the first cluster that reaches it).  Here the two are held to each other on every hand-made case, which also shows that "first cluster to
reach" and "lowest raw label" coincide."""
import os
import subprocess

import numpy as np
import pytest

import nrs_synth as S
import stereo_cases as SC
import stereo_init_oracle as SO

F32 = np.float32
CASES = S.make_cluster_cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_sequential_equals_fixed_point(case):
    for nc in (True, False):
        a = SO.dbscan3d(case["xyz"], case["eps"], case["min_points"], nc)
        b = SO.dbscan3d_fixed_point(case["xyz"], case["eps"], case["min_points"], nc)
        for x, y, name in zip(a, b, ("raw_label", "label", "counts")):
            assert np.array_equal(x, y), (case["name"], nc, name)


LARGE = SC.LARGE_CLUSTER_CASES


@pytest.mark.parametrize("case", LARGE, ids=[c["name"] for c in LARGE])
def test_the_large_cases_hold_what_they_are_made_for(case):
    """roots in every compaction chunk, no core point in the first two chunks, relations that exist only through points behind the first
    trip of the word loops, the limit of 16384 points: each case's `holds` (nrs_synth.make_large_cluster_cases) on the oracle's output"""
    exp = SC.cluster_expected(case["name"], check=True)
    raw, lab, counts = exp[True]
    print(case["name"], len(raw), "points, counts", list(counts))
    assert len(raw) == len(case["xyz"]) and counts[0] == raw.max() + 1
    if len(raw) <= SC.BRUTE_FORCE_MAX_POINTS:
        # the brute-force closure sweeps once per hop of a component's longest shortest path (thousands on the long chain) and is a
        # Python loop over the core points: it is held to the sequential oracle on the cases of at most BRUTE_FORCE_MAX_POINTS points
        for nc in (True, False):
            b = SO.dbscan3d_fixed_point(case["xyz"], case["eps"], case["min_points"], nc)
            for x, y, name in zip(exp[nc], b, ("raw_label", "label", "counts")):
                assert np.array_equal(x, y), (case["name"], nc, name)


def test_large_case_names_and_sizes():
    sizes = {c["name"]: len(c["xyz"]) for c in LARGE}
    assert sizes == {"roots_in_three_chunks": 2100, "first_root_late": 2100, "second_trip4097": 4097, "second_trip4160": 4160,
                     "chain4200_shuffled": 4200, "full16384": 16384, "full16321": 16321}
    assert not {c["name"] for c in CASES} & set(sizes)


def _case(name):
    return next(c for c in CASES if c["name"] == name)


def test_the_cases_hold_what_they_are_made_for():
    run = lambda name, nc=True: SO.dbscan3d(_case(name)["xyz"], _case(name)["eps"], _case(name)["min_points"], nc)
    raw, lab, counts = run("min_points")
    assert np.all(raw == -1) and list(counts) == [0, 5, 5]                       # four neighbours each: no core point
    raw, lab, counts = run("min_points+1")
    nb = SO.neighbours(_case("min_points+1")["xyz"], 2.5).sum(1)
    assert list(nb) == [5, 4, 4, 4, 4, 1] and np.all(raw == 0)                   # one core point with exactly min_points neighbours
    raw, lab, counts = run("boundary")
    assert list(raw) == [0, 0, -1, -1]                                           # eps apart: neighbours; one ulp beyond: not
    for name in ("chain300", "chain300_shuffled", "chain300_reversed"):
        raw, lab, counts = run(name)
        assert np.all(raw == 0) and list(counts) == [1, 0, 300]
    raw, lab, counts = run("bridge")
    assert raw[0] == 0 and np.all(raw[1:21] == 0) and np.all(raw[21:] == 1)      # two clusters; the bridge takes the lower raw label
    nb = SO.neighbours(_case("bridge")["xyz"], 2.5)
    assert nb[0].sum() == 2 and nb[0, 1] and nb[0, 40]                           # ... and touches a core point of either chain
    raw, lab, counts = run("coincident")
    assert np.all(raw == 0)
    raw, lab, counts = run("nan_inf")
    assert raw[7] == -1 and raw[21] == -1 and not SO.neighbours(_case("nan_inf")["xyz"], 2.5)[:, [7, 21]].any()


def test_ranking_rules():
    # size descending, ties by ascending raw key; noise is key -1 when it competes and keeps -1 when it does not
    raw = np.array([2, 2, 2, 0, 0, 1, 1, -1, -1, -1, -1], np.int32)
    lab, counts = SO.rank_labels(raw, True)
    assert list(lab) == [1, 1, 1, 2, 2, 3, 3, 0, 0, 0, 0] and list(counts) == [3, 4, 4]
    lab, counts = SO.rank_labels(raw, False)
    assert list(lab) == [0, 0, 0, 1, 1, 2, 2, -1, -1, -1, -1] and list(counts) == [3, 4, 3]
    lab, counts = SO.rank_labels(np.array([0, 0, -1, -1], np.int32), True)       # a tie between noise and a cluster: key -1 first
    assert list(lab) == [1, 1, 0, 0] and list(counts) == [1, 2, 2]
    lab, counts = SO.rank_labels(np.array([-1, -1], np.int32), False)            # nothing but noise, not competing: no rank 0
    assert list(lab) == [-1, -1] and list(counts) == [0, 2, 0]
    lab, counts = SO.rank_labels(np.zeros(0, np.int32), True)
    assert len(lab) == 0 and list(counts) == [0, 0, 0]
    # the hand-made sets: equal sizes go by raw key, a noise majority wins only when it competes
    c = _case("equal_sizes")
    raw, lab, counts = SO.dbscan3d(c["xyz"], c["eps"], c["min_points"], True)
    assert list(raw) == [0] * 8 + [1] * 8 and np.array_equal(lab, raw)
    c = _case("noise_majority")
    raw, lab, counts = SO.dbscan3d(c["xyz"], c["eps"], c["min_points"], True)
    assert list(counts) == [2, 20, 20] and np.all(lab[raw == -1] == 0) and np.all(lab[raw == 0] == 1) and np.all(lab[raw == 1] == 2)
    raw, lab, counts = SO.dbscan3d(c["xyz"], c["eps"], c["min_points"], False)
    assert list(counts) == [2, 20, 8] and np.all(lab[raw == -1] == -1) and np.all(lab[raw == 0] == 0)


def test_verdict_codes_and_the_strict_gate():
    sc = S.make_stereo_pair((96, 64), 5, disparities=(0, 8), n_keypoints=40)
    prm = S.HAMLYN_PINHOLE
    bf = 400.0                                                                   # disparity 8 is depth 50; the fractional keypoints of the 0 band lie far beyond the gate
    r = SO.init_stereo(prm, sc["left"], sc["right"], sc["xy"], bf=bf, z_min=40.0, z_max=60.0, eps=30.0, min_points=2)
    assert r["verdict"] == 0 and r["n_gated"] > 0 and r["n_matched"] > r["n_gated"]
    ok = r["match_status"] == 0
    assert np.all(r["code"][~ok] == 1) and np.all(r["raw_label"][~ok] == -2) and np.all(r["label"][~ok] == -2)
    out = ok & ~((r["xyz"][:, 2] > 40) & (r["xyz"][:, 2] < 60))
    assert out.any() and np.all(r["code"][out] == 2) and np.all(r["label"][out] == -2)
    assert np.array_equal(r["selected"], np.nonzero(r["code"] == 0)[0]) and np.array_equal(r["selected_xyz"], r["xyz"][r["selected"]])
    assert r["median_depth"] == np.sort(r["selected_xyz"][:, 2])[r["n_selected"] // 2]
    # a keypoint exactly on z_min is excluded: the comparison is strict
    z = np.unique(r["xyz"][ok & (r["code"] != 2), 2])
    r2 = SO.init_stereo(prm, sc["left"], sc["right"], sc["xy"], bf=bf, z_min=float(z[0]), z_max=60.0, eps=30.0, min_points=2)
    assert np.all(r2["code"][r["xyz"][:, 2] == z[0]] == 2)
    # nothing passes the gate: verdict 1, nothing selected, no median
    r3 = SO.init_stereo(prm, sc["left"], sc["right"], sc["xy"], bf=bf, z_min=1e5, z_max=2e5)
    assert r3["verdict"] == 1 and r3["n_gated"] == 0 and r3["n_selected"] == 0 and len(r3["selected"]) == 0 and np.isnan(r3["median_depth"])
    assert np.all(r3["code"] >= 1) and np.all(r3["label"] == -2)


def test_host_half_stand_alone():
    """`make sinit_check`: csrc/nrs_sinit_host.hpp under AddressSanitizer + UBSan in a program of its own"""
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "nr-slam_amd"), "sinit_check"], capture_output=True, text=True)
    assert p.returncode == 0 and "sinit_check OK" in p.stdout, p.stdout + p.stderr
