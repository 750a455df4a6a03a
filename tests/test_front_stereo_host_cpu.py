"""CPU: the host side of the resident stereo pair (include/nrs.h nrs_front_process_stereo and "the resident stereo pair") -- the new entry
points are declared, listed and exported, the binding and the frame loop expose what drives them, and the scene the GPU test of
nrs_init_stereo_front uses is one on which that comparison covers something (checked with the oracle alone)."""
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["nrs_front_process_stereo", "nrs_stereo_match_pattern_front", "nrs_init_stereo_front", "nrs_stereo_match_lk_front"]


def test_new_symbols_are_declared_listed_and_exported(lib_built):
    nrs = lib_built
    lib = nrs.load_library()
    hdr = open(os.path.join(ROOT, "include", "nrs.h")).read()
    declared = set(re.findall(r"\b(nrs_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in nrs.SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name                   # the binding gives each of them its argument types
    # every entry point cites the reference lines it restates
    for cite in ("system.cc:134-160", "stereo_pattern_matching.cc:33-94", "tracking.cc:216-263", "stereo_lucas_kanade.cc:38-75"):
        assert cite in hdr, cite
    for name in ("front_process_stereo", "stereo_match_pattern_front", "init_stereo_front"):
        assert callable(getattr(nrs.Context, name)), name
    assert callable(nrs.stereo_lk_front)
    assert list(inspect.signature(nrs.stereo_lk_front).parameters)[:2] == ["ctx_stereo", "ctx_front"]


def test_backend_and_loop_expose_the_stereo_steps(lib_built):
    import nrs_frame_loop as FL
    for name in ("front_stereo", "init_stereo", "stereo_pattern", "stereo_lk"):
        assert callable(getattr(FL.GpuBackend, name)), name
    p = inspect.signature(FL.FrameLoop.track_image_with_stereo).parameters
    assert list(p)[:3] == ["self", "left", "right"]
    assert p["evaluate"].default is False and p["matcher"].default == "pattern" and "bf" in p      # (compiled out in the reference: off)


def test_the_init_scene_of_the_gpu_test_has_a_cluster_and_noise():
    """tests/test_gpu_front_stereo.py compares nrs_init_stereo_front with the oracle on this scene: the comparison covers the gate, the
    clustering and the selection only if the oracle finds a verdict 0, at least one cluster and some noise on it"""
    import stereo_cases as SC
    sc = SC.init_scene()
    o = sc["oracle"]
    assert o["verdict"] == 0 and o["n_clusters"] >= 1 and o["n_noise"] > 0 and o["n_selected"] >= 3
    assert all((o["code"] == k).any() for k in range(4))
    import eval_oracle as E
    st = SC.pattern_scene()["oracle17"][1]                            # the matcher's scene: matched and unmatched keypoints, the two rejections
    assert (st == E.OK).sum() >= 4 and (st == E.LOW_CORRELATION).sum() >= 4 and (st == E.OUT_OF_BOUNDS).sum() == 1 and (st == E.SATURATED).sum() == 1
    assert SC.pattern_scene()["oracle1"][1].tolist() == [E.OK]
    assert sc["left"].shape == (64, 96) and np.array_equal(sc["left"], sc["raw_left"][:, :, 0])
