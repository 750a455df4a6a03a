"""CPU: the scenes of tests/stereo_cases.py for the matcher's ties and near-ties and for nrs_init_stereo with three chunks of keypoints hold
what they are made for.  Every condition is asserted on the oracles' output alone (tests/eval_oracle.py's per-position score maps,
tests/stereo_init_oracle.py's result), so a scene that stops holding its property fails here, where no device is asked."""
import numpy as np
import pytest

import eval_oracle as E
import stereo_cases as SC


@pytest.mark.parametrize("second_workgroup", [False, True], ids=["first_position", "second_workgroup"])
def test_lattice_of_exact_ties(second_workgroup):
    sc = SC.lattice_scene(second_workgroup)
    SC.lattice_holds(sc)
    match = sc["oracle"][3]
    if not second_workgroup:
        assert match.max() == 1                                     # the first position of the template's parity
    else:
        assert match[:, 0].min() >= SC.MF_TILE[0] and match[:, 1].min() >= SC.MF_TILE[1]
        Wr, Hr = E.search_dims(*sc["wh"])
        assert Wr > 2 * SC.MF_TILE[0] and Hr > 2 * SC.MF_TILE[1]     # three workgroups a side


@pytest.mark.parametrize("name", list(SC.NEAR_TIES))
def test_near_ties_lie_within_the_screen_margin(name):
    gap = SC.near_tie_holds(SC.near_tie_scene(name))
    print(name, "largest relative gap of the two best distinct scores: %.3e" % gap)
    assert gap < 1e-6                                               # (a grey level in one of 225 pixels: far inside the 1e-5 the screen claims)


def test_init_scene_with_three_chunks_of_keypoints():
    p = SC.init_scene_three_chunks()
    counts = SC.init_three_chunks_holds(p)
    o1, o0 = p["oracle"][1], p["oracle"][0]
    print("n_matched, n_gated, n_selected", counts, "codes", np.bincount(o1["code"]), "clusters", o1["n_clusters"], "noise", o1["n_noise"])
    assert np.array_equal(o1["raw_label"], o0["raw_label"])
    noise = o1["raw_label"] == -1
    assert noise.any() and np.all(o0["label"][noise] == -1) and np.all(o1["label"][noise] >= 1)
