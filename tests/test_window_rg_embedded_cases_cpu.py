"""The windows of tests/window_rg_embedded_cases.py say something (no GPU): on the restatements alone, some walks run off a first prefix
and some do not, skinned walks among them; the window is served by prefixes, not by whole lists; skinned observations with fewer than 11
nodes and with none exist; BAD entries stop walks; and the host builder agrees with the oracle on the full lists."""
import numpy as np
import pytest

import embedded_oracle as E
import nrs
import window_rg_embedded_cases as WE

LISTS = ("lm_obs", "sp_ij", "sp_d0", "dm_idx", "dm_w", "sk_obs", "sk_node", "sk_omega")


@pytest.mark.parametrize("name", WE.CASES)
def test_some_walks_run_off_a_first_prefix_and_some_do_not(name):
    c = WE.case(name)
    for first in (64, 8):
        ran, total, ran_skin = WE.walks_that_run_off(c, first)
        assert 0 < ran < total, (first, ran, total)
        assert ran_skin > 0, first                                   # a skinned walk runs off in round 1
        cap, rounds = WE.final_cap(c, first, c["n"])
        assert rounds >= 2
        assert cap < c["n"] - 1                                      # served by prefixes, not by the whole lists


@pytest.mark.parametrize("name", WE.CASES)
def test_the_full_walks_cover_the_cases(name):
    c = WE.case(name)
    w = WE.walks(c)
    n_obs = sum(len(k) for k in c["p"]["kf_points"])
    assert n_obs > 256                                               # more than one workgroup of the thread-per-observation kernels
    assert not any(x[5] for x in w)                                  # a complete list never runs off
    skin = [x for x in w if x[0] == "skin"]
    assert any(0 < x[3] < 11 for x in skin)                          # a skinned observation with fewer than 11 nodes
    assert any(x[3] == 0 for x in skin)                              # ... and one bound to nothing
    assert any(x[4] == "bad" for x in w) and any(x[4] == "bad" for x in skin)      # walks stopped by a BAD entry
    assert any(x[4] == "count" for x in w)                           # ... and by the count
    assert any(x[0] == "spring" and x[3] > 0 for x in w) and any(x[0] == "damper" and x[3] > 0 for x in w)


@pytest.mark.parametrize("name", WE.CASES)
def test_host_builder_is_the_oracle_on_the_full_lists(name):
    c = WE.case(name)
    p, nb = c["p"], c["nbr"]
    host = nrs.dba_build_edges_embedded(p["kf_points"], c["flag"], nb)
    ora = E.dba_build_embedded(p["kf_points"], c["flag"], nb["rowptr"], nb["col"], nb["w"], nb["d0"], nb["status"])
    for key in LISTS:
        assert np.array_equal(host[key], ora[key]), key
    assert len(host["sp_d0"]) > 0 and len(host["dm_w"]) > 0 and len(host["sk_obs"]) > 0
    # the restated walks describe these lists: node copies, skinned observations and their node counts
    w = WE.walks(c)
    assert len(host["lm_obs"]) == sum(x[0] == "spring" for x in w)
    skin = [x for x in w if x[0] == "skin" and x[3] > 0]
    assert np.array_equal(host["sk_obs"], [x[1] for x in skin])
    assert np.array_equal((host["sk_node"] >= 0).sum(1), [x[3] for x in skin])


def test_the_small_window_runs_off_a_limit_of_16():
    """the 120-point window of the run-off-at-the-limit test: walks run off a prefix of 16, and its 120-point graph is served whole"""
    c = WE.case(WE.SMALL)
    ran, total, _ = WE.walks_that_run_off(c, 16)
    assert 0 < ran < total
    assert WE.final_cap(c, 8, c["n"])[1] >= 2
