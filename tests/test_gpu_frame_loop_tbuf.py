"""GPU: the frame loop with the resident TemporalBuffer (GpuBackend(device_tbuf=True): nrs_tbuf_insert per frame, nrs_map_frame_tbuf for
frame mapping) against the same loop on the host buffer (the default: TemporalBuffer.flat + nrs_map_frame).  Both run the same kernels
on the same tables, so every logged field is EQUAL -- poses and positions as bytes, not within a tolerance."""
import numpy as np
import pytest

import map_loop_backend as B
import nrs
import nrs_frame_loop as FL
import nrs_synth as S
import test_gpu_frame_loop_stereo as ST

pytestmark = pytest.mark.gpu


def _same_logs(a_log, b_log):
    assert len(a_log) == len(b_log)
    for f, (a, b) in enumerate(zip(a_log, b_log), 1):
        assert set(a) == set(b), f
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (f, k)
            else:
                assert a[k] == b[k], (f, k)


def _same_state(a, b):
    for k in ("map_pos", "kp", "pos", "status", "map_index", "kp_id"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


def test_mapping_loop_is_the_host_buffer_loop():
    sq = B.sequence()
    loops = {}
    for dev in (False, True):
        gb = FL.GpuBackend(nrs, sq["model"], sq["prm"], B.OPTS, dense_graph=True, device_tbuf=dev)
        try:
            loops[dev] = B.run(gb, True)
            if dev:
                assert loops[dev].tbuf is None and gb.tb.info()[0] == min(21, B.N_FRAMES - 1)
        finally:
            gb.close()
    host, res = loops[False], loops[True]
    assert len(res.log) == B.N_FRAMES - 1
    _same_logs(res.log, host.log)
    _same_state(res, host)
    assert any(e["mapping"]["skipped"] is None and e["mapping"]["n_candidates"] > 0 for e in res.log)      # frame mapping did run
    assert res.log[-1]["map_size"] - sq["n_points"] >= 5


def test_stereo_start_with_mapping_is_the_host_buffer_loop():
    """the sequence of tests/test_gpu_frame_loop_stereo.py (its helpers, unedited): a stereo start, whose first frame takes FrameMapping"""
    sq = S.make_stereo_init_sequence()
    opts = dict(bf=sq["bf"], z_min=sq["z_min"], z_max=sq["z_max"], eps=sq["eps"], min_points=sq["min_points"])
    loops = {}
    for dev in (False, True):
        gb = FL.GpuBackend(nrs, sq["model"], sq["prm"], B.OPTS, dense_graph=True, front=True, device_tbuf=dev)
        try:
            left0, right = sq["images"][0], sq["right"]
            gb.front_stereo(left0, right)
            xy = ST._thin(gb.extract_features(left0, None, None)[0])
            loop = ST._loop(gb, sq, gb.init_stereo(left0, right, xy, **opts))
            for f in (1, 2):
                assert loop.track_image_with_stereo(sq["images"][f], right.copy())
            loops[dev] = loop
        finally:
            gb.close()
    _same_logs(loops[True].log, loops[False].log)
    _same_state(loops[True], loops[False])
    assert all("mapping" in e for e in loops[True].log) and loops[True].log[0]["mapping"]["skipped"] is None
