"""The designed cases of tests/triang_cases.py, vetted without a GPU: the restatement (oracle/triang_oracle.py) reaches the code every
case is made for, GetClosestMapPointsToFeature returns the intended list, and no gate the restatement evaluates on the way sits within
1e-3 (relative) of its threshold -- the two reprojection errors, the parallax, the seed depths (against the scene's depth: their
threshold is 0), the bad-edge and the bad-frame ratio, and every neighbour distance against 20 and 500 px.  The only quantities ON a
threshold are the distances the neighbour cases put there with integer pixel coordinates (exactly 20, exactly 500)."""
import numpy as np
import pytest

import triang_cases as TC
import triang_oracle as T


@pytest.mark.parametrize("name", TC.CASES)
def test_case_reaches_its_code_with_margins(name):
    cs = TC.case(name)
    tb = cs["tb"]
    F, n = tb["has_kp"].shape
    assert F == tb["n_frames"] <= 21 and n <= 200 and 1 <= len(cs["cand"]) <= 8
    for c, r in zip(cs["cand"].tolist(), cs["ref"]):
        want = cs["want"][c]
        if want is None:
            assert r["status"] != T.E_CLOSE, (name, c, T.STATUS_TEXT[r["status"]])
        else:
            assert r["status"] == want, (name, c, T.STATUS_TEXT[r["status"]], T.STATUS_TEXT[want])
        assert (r["status"] == T.OK) == bool(np.any(r["xyz"] != 0)) and np.isfinite(r["xyz"]).all()
        if cs["want_nb"] is not None:
            assert T.closest_map_points(tb, c) == cs["want_nb"][c], (name, c, T.closest_map_points(tb, c))
        near = [g for g in r["gates"] if TC.on_threshold(g, cs["exact_px"])]
        assert not near, (name, c, near)
        print(name, c, T.STATUS_TEXT[r["status"]], "edges", r["edges"], {g[0]: round(g[1], 4) for g in r["gates"] if not g[0].startswith("neigh")})


def test_the_exact_distances_are_exact():
    """20 px and 500 px are hit exactly, from integer coordinates, and the pixels next to them fall on the other side"""
    for name, d in (("nb_one", 500.0), ("nb_at_20", 20.0)):
        cs = TC.case(name)
        last = cs["tb"]["kp_xy"][-1]
        assert np.array_equal(last, np.round(last)) and d in TC.neighbour_distances(cs["tb"], int(cs["cand"][0]))
    assert min(TC.neighbour_distances(TC.case("nb_none_far")["tb"], 7)) > 500.0
    assert min(TC.neighbour_distances(TC.case("nb_below_20")["tb"], 7)) < 20.0


def test_neighbour_cases_tell_their_members_apart():
    """every map point within 500 px of a neighbour case's candidate, eligible or not, carries another number of regulariser edges"""
    for name in TC.NB_CASES:
        cs = TC.case(name)
        tb = cs["tb"]
        last = tb["n_frames"] - 1
        for c in cs["cand"].tolist():
            inside = [j for j in np.nonzero(tb["status"] != 1)[0]
                      if np.linalg.norm(tb["kp_xy"][last, j].astype(np.float64) - tb["kp_xy"][last, c]) <= 500.0]
            m = [int(tb["has_lm"][:, j].sum()) for j in inside]
            assert all(tb["has_lm"][0, j] for j in inside) and len(set(m)) == len(m), (name, m)


def test_ties_cross_the_eleventh_place_on_shared_lanes():
    cs = TC.case("nb_ties_lanes")
    nb = T.closest_map_points(cs["tb"], 70)
    d = dict(zip(np.nonzero(cs["tb"]["has_kp"][-1] & (cs["tb"]["status"] == 0))[0].tolist(), TC.neighbour_distances(cs["tb"], 70)))
    tied = sorted(j for j, v in d.items() if v == 50.0)
    assert len(tied) == 16 and nb[2:] == tied[:9] and d[nb[10]] == 50.0 and d[tied[9]] == 50.0           # the tie holds places 3 .. 18
    lanes = [j % 64 for j in tied]
    assert lanes.count(3) == 3 and lanes.count(5) == 3 and len(set(lanes)) > 8                                # j, j + 64, j + 128; and others
    assert nb[10] == 131 and tied[9] == 133                        # in: the third stride of lane 3; out: the third stride of lane 5


def test_first_bad_frame_cases_hold_both_failures():
    """both tracks have a snapshot without a neighbour landmark AND one with a negative seed depth: only their order differs"""
    for name, neg, none in (("first_bad_decides_a", 1, 3), ("first_bad_decides_b", 3, 1)):
        cs = TC.case(name)
        tb = cs["tb"]
        nb = T.closest_map_points(tb, 0)
        P = tb["poses"].astype(np.float32)
        assert not tb["has_lm"][none, nb].any() and tb["has_kp"][:, 0].all()
        z = np.mean([T.se3_mul_point(P[neg], tb["lm_xyz"][neg, j])[2] for j in nb if tb["has_lm"][neg, j]])
        assert z < -1.0
        assert cs["ref"][0]["status"] == (T.E_NEG_DEPTH if neg < none else T.E_NO_NEIGHBOUR)


def test_no_regulariser_edge_means_no_solve():
    """`no_edges` and its control: with no edge the normal matrix is zero, lambda is 0, every Cholesky fails, and the LM gives up after one
    iteration of ten trials with the estimates where the seeds put them (also true of a one-vertex track)"""
    assert TC.case("first_frame_blind")["ref"][0]["status"] == T.E_NO_NEIGHBOUR and TC.case("first_frame_blind")["ref"][0]["edges"] is None
    for name in ("no_edges", "no_edges_kb8", "track_1", "frames_1"):
        r = TC.case(name)["ref"][0]
        assert r["status"] == T.OK and r["edges"] == 0
        assert all(not t["ok"] and not t["accepted"] and t["lam"] == 0.0 for t in r["trace"])
        assert (r["iters"], r["trials"], r["all_failed"]) == (1, 10, True)
    for name in ("track_2", "frames_2"):
        r = TC.case(name)["ref"][0]
        assert r["edges"] > 0 and not r["all_failed"]


def test_track_shapes():
    tb = TC.case("track_21_gappy")["tb"]
    assert np.nonzero(tb["has_kp"][:, 0])[0].tolist() == list(range(0, 21, 2))
    assert [int(TC.case(n)["tb"]["has_kp"][:, 0].sum()) for n in ("track_1", "track_2", "frames_1", "frames_2")] == [1, 2, 1, 2]
    assert [TC.case(n)["tb"]["n_frames"] for n in ("frames_1", "frames_2")] == [1, 2]
    sh = TC.case("short")
    assert sh["tb"]["has_kp"][:, sh["cand"]].sum(0).tolist() == [sh["min_track"] - 1, sh["min_track"]]


def test_every_code_is_reached():
    seen = {r["status"] for name in TC.CASES for r in TC.case(name)["ref"]}
    assert seen == {T.OK, T.E_CLOSE, T.E_REPROJ1, T.E_REPROJ2, T.E_PARALLAX, T.E_NO_NEIGHBOUR, T.E_NEG_DEPTH, T.E_BAD_NEIGHBOURS, T.E_BAD_ERROR,
                    T.E_SHORT}
    models = [TC.case(name)["tb"]["model"] for name in TC.CASES]
    assert models.count(TC.S.KB8) >= 2
