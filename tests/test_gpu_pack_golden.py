"""GPU: the problem construction against the bits recorded in tests/golden/pack_hashes.json (tools/pack_hash_golden.py).  The other
pack tests hold the device construction to the host construction and would still pass if both changed together; this one holds both
to a recorded commit -- checksums of every packed array, sizes, the first LM trials to the last bit, and a refusal's code and text.
Nothing here has a tolerance."""
import json
import os

import pytest

import pack_golden_cases as G

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_hashes.json")) as fh:
    GOLDEN = json.load(fh)


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(G.CASES)


@pytest.mark.parametrize("name", list(G.CASES))
def test_pack_is_the_recorded_pack(name):
    got = json.loads(json.dumps(G.record(name)))     # (tuples and numpy integers as the file holds them)
    want = GOLDEN[name]
    if isinstance(want, list):
        assert len(got) == len(want)
        for r, (a, b) in enumerate(zip(got, want)):
            assert a == b, (name, r, {k: (a.get(k), b.get(k)) for k in set(a) | set(b) if a.get(k) != b.get(k)})
    else:
        assert got == want, (name, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)})
