"""CPU: the node-selection restatement (oracle/skin_oracle.py) against a literal farthest-point loop and the properties
that define the sampling (distinct picks, non-increasing cover radius, eligibility)."""
import numpy as np

import skin_oracle as K
from skin_cases import literal as _literal                          # (shared with tests/test_skin_cases_cpu.py)


def test_matches_a_literal_loop_and_the_defining_properties():
    rng = np.random.default_rng(4)
    pos = rng.uniform(-10, 10, (120, 3)).astype(np.float32)
    pos[60] = pos[20]
    ok = rng.uniform(size=120) < 0.7
    assert np.array_equal(K.select_nodes(pos, 25, ok), _literal(pos, 25, ok))
    assert np.array_equal(K.select_nodes(pos, 25), _literal(pos, 25, np.ones(120, bool)))
    big = rng.uniform(-20, 20, (3000, 3)).astype(np.float32)
    ids = K.select_nodes(big, 300)
    assert len(set(ids.tolist())) == 300 and ids[0] == 0
    # cover radius (distance of pick k to the picks before it) never grows
    rad = [np.min(np.linalg.norm(big[ids[:k]] - big[ids[k]], axis=1)) for k in range(1, 300)]
    assert all(rad[i + 1] <= rad[i] * (1 + 1e-6) for i in range(len(rad) - 1))
    try:
        K.select_nodes(pos, int(ok.sum()) + 1, ok)
        assert False
    except ValueError:
        pass
