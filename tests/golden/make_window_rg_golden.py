"""Goldens of tests/test_gpu_window_rg.py: nrs_oracle.dba_solve (the dense restatement of optimize(5), OPT:1140-1143) on the two larger
windows of tests/window_rg_cases.py, whose solve takes the oracle one to ten minutes -- not a test's work.  Stored per case: the final
poses and points (fp64), the accept / reject sequence of the LM trials, and a checksum of the problem it was run on (observations and the
oracle's edge lists), which the test compares with its own inputs before it uses the numbers.
    python tests/golden/make_window_rg_golden.py [case ...]
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "nr-slam_amd", "py"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)
import nrs_oracle as O  # noqa: E402
import window_rg_cases as W  # noqa: E402

GOLDEN_CASES = ("900x6_kb8", "2000x5")


def problem_checksum(p, edges):
    h = hashlib.sha256()
    for a, t in ((p["poses_q"], np.float64), (p["poses_t"], np.float64), (p["lm_xyz"], np.float32), (p["lm_uv"], np.float32), (p["lm_kf"], np.int32),
                 (edges["sp_ij"], np.int32), (edges["sp_d0"], np.float32), (edges["dm_idx"], np.int32), (edges["dm_w"], np.float32)):
        h.update(np.ascontiguousarray(a, t).tobytes())
    return h.hexdigest()


def path(name):
    return os.path.join(HERE, "window_rg_%s.npz" % name)


if __name__ == "__main__":
    for name in sys.argv[1:] or GOLDEN_CASES:
        c = W.case(name)
        p, nbr = c["p"], c["nbr"]
        e = O.dba_build(p["kf_points"], nbr["rowptr"], nbr["col"], nbr["w"], nbr["d0"], nbr["status"])
        tr = []
        q, t, pts, _ = O.dba_solve(p["model"], p["prm"], p["poses_q"], p["poses_t"], p["lm_xyz"], p["lm_kf"], p["lm_uv"], e["sp_ij"], e["sp_d0"], e["dm_idx"],
                                   e["dm_w"], p["scale"], 5, tr)
        np.savez_compressed(path(name), q=q, t=t, pts=pts, accepted=np.array([x["accepted"] for x in tr], np.uint8),
                            checksum=np.array(problem_checksum(p, e)))
        print(name, "trials", len(tr), "->", path(name), flush=True)
