"""GPU: nrs_skin_select_nodes (k_fps, csrc/nrs_skin.hip) on the designed cases of tests/skin_cases.py, which tests/test_skin_cases_cpu.py
vets without a device: every case equals the oracle's picks IN PICK ORDER, bit for bit; every refusal is checked by code and message and
leaves the context usable."""
import numpy as np
import pytest

import nrs
import skin_cases as SC

pytestmark = pytest.mark.gpu
NRS_ERR_INVALID = -1


def _run(ctx, c):
    return ctx.skin_select_nodes(c["pos"], c["m"], c["eligible"])


@pytest.mark.parametrize("name", SC.CASES)
def test_picks_equal_the_oracle_in_pick_order(ctx, name):
    c = SC.case(name)
    ids = _run(ctx, c)
    assert ids.dtype == np.int32 and np.array_equal(ids, c["picks"]), (name, np.nonzero(ids != c["picks"])[0][:4])


def test_lattice_twice_on_one_context(ctx):
    """nothing of a call survives in the running minima or the LDS scratch: a masked lattice in between, then the same picks again"""
    c = SC.case("lattice")
    first = _run(ctx, c)
    assert np.array_equal(_run(ctx, SC.case("lattice_one_wave")), SC.case("lattice_one_wave")["picks"])
    second = _run(ctx, c)
    assert np.array_equal(first, second) and np.array_equal(second, c["picks"])


@pytest.mark.parametrize("name", SC.REFUSALS)
def test_refusals_by_code_and_message(ctx, name):
    r = SC.refusal(name)
    with pytest.raises(nrs.NrsError) as e:
        ctx.skin_select_nodes(r["pos"], r["m"], r["eligible"])
    assert e.value.code == NRS_ERR_INVALID
    for w in r["words"]:
        assert w in str(e.value), (w, str(e.value))
    good = SC.case(SC.GOOD_AFTER_REFUSAL)                          # the context stays usable
    assert np.array_equal(_run(ctx, good), good["picks"])
