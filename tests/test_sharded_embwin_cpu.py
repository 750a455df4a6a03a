"""The sharded one-call embedded window (include/nrs.h nrs_dba_solve_window_embedded on a communicator) without a GPU: the new entry points
are declared, exported and bound; the keyframe range a rank derives from the per-keyframe node-copy counts (nrs_shard_plan_counts: what
the device builder feeds the set-up's shard_plan) is nrs_shard_plan's on the windows of tests/test_gpu_sharded_embwin.py; and those
windows are not vacuous."""
import os
import re

import numpy as np
import pytest

import embedded_window_cases as W
import nrs_synth as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE8 = (300, 8, 40, 61, S.PINHOLE, {})                              # (as tests/test_gpu_sharded_embwin.py)
CASE4 = (300, 4, 40, 53, S.PINHOLE, {})


def test_entry_points_are_declared_exported_and_bound(lib_built):
    nrs = lib_built
    text = open(os.path.join(ROOT, "include", "nrs.h")).read()
    assert re.search(r"^int nrs_dba_window_slice_embedded\(nrs_ctx\* ctx,", text, re.M)
    assert re.search(r"^int nrs_shard_plan_counts\(int32_t n_kf,", text, re.M)
    lib = nrs.load_library()
    for name in ("nrs_dba_window_slice_embedded", "nrs_shard_plan_counts"):
        assert name in nrs.SYMBOLS and hasattr(lib, name), name
    assert lib.nrs_dba_window_slice_embedded(None, None) == -1       # a null context fails cleanly, no device needed
    assert callable(getattr(nrs.Context, "dba_window_slice_embedded")) and callable(nrs.shard_plan_counts)


@pytest.mark.parametrize("case", [CASE8, CASE4], ids=["8kf", "4kf"])
@pytest.mark.parametrize("form", W.FORMS)
def test_range_from_per_keyframe_counts_is_shard_plan(lib_built, case, form):
    nrs = lib_built
    p, flag, nb = W.window(case, form)
    e = nrs.dba_build_edges_embedded(p["kf_points"], flag, nb)
    n_kf = len(p["kf_points"])
    obs_kf = np.concatenate([np.full(len(x), k, np.int32) for k, x in enumerate(p["kf_points"])])
    lm_kf = obs_kf[e["lm_obs"]]
    counts = np.bincount(lm_kf, minlength=n_kf)
    assert (counts > 0).all() and len(set(counts.tolist())) > 1      # (uneven keyframes: the split is not trivially even)
    for world in range(1, min(n_kf, 8) + 1):
        kb = nrs.shard_plan_counts(counts, world)
        assert kb.tolist() == nrs.shard_plan(n_kf, lm_kf, world).tolist()
        assert kb[0] == 0 and kb[-1] == n_kf and (np.diff(kb) >= 1).all()


def test_counts_that_cross_the_row_padding(lib_built):
    """shard_plan balances rows padded to 256 per keyframe: counts either side of a multiple of 256, and an empty keyframe (one group)"""
    nrs = lib_built
    counts = np.array([256, 257, 1, 0, 600, 255, 512, 513], np.int32)
    lm_kf = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    for world in (1, 2, 3, 5, 8):
        assert nrs.shard_plan_counts(counts, world).tolist() == nrs.shard_plan(len(counts), lm_kf, world).tolist()
    with pytest.raises(nrs.NrsError):
        nrs.shard_plan_counts(counts, 9)                             # more ranks than keyframes


def test_the_gpu_windows_are_not_vacuous(lib_built):
    nrs = lib_built
    for case in (CASE8, CASE4):
        for form in W.FORMS:
            p, flag, nb = W.window(case, form)
            W.check_not_vacuous(case, form, p, flag, nb, nrs.dba_build_edges_embedded(p["kf_points"], flag, nb))
    p, flag, nb = W.window(CASE8, "full")
    assert ((np.asarray(flag)[p["kf_points"][5]]) != 0).sum() >= 2   # (the duplicate-node case needs two nodes in keyframe 5)
