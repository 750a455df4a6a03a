"""CPU: the flow-track clustering's oracle (tests/flow_cluster_oracle.py) pinned to the stereo start's, every case of
tests/flow_cluster_cases.py holding what it is made for, the new symbols, the stand-alone check of the host half (`make flowc_check`) and
MonoInitializer(cluster_tracks=True) over a backend that is the oracle."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import flow_cluster_cases as FC
import flow_cluster_oracle as FO
import nrs_frame_loop as FL
import nrs_synth as S
import stereo_init_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nr-slam_amd")
F32 = np.float32
NEW = ["nrs_dbscan_nd", "nrs_flow_tracks_cluster"]


def test_new_symbols_are_declared_listed_and_exported(lib_built):
    nrs = lib_built
    lib = nrs.load_library()
    hdr = open(os.path.join(ROOT, "include", "nrs.h")).read()
    declared = set(re.findall(r"\b(nrs_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in nrs.SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name                   # the binding gives each of them its argument types
    assert "#define NRS_DBSCAN_MAX_DIM 64" in hdr and nrs.DBSCAN_MAX_DIM == 64
    assert (nrs.FLOW_MIN_LENGTH, nrs.FLOW_MAX_LENGTH, nrs.FLOW_MIN_POINTS) == (2, 33, 10)
    for cite in ("monocular_map_initializer.cc:185-219", "dbscan.cc:106-131", "NRS_DBND_NO_TILE"):
        assert cite in hdr, cite
    assert "the DBSCAN labels of FeatureTracksClustering (visualiser only" not in hdr      # the "Not built" sentence is gone
    for name in ("dbscan_nd", "flow_tracks_cluster"):
        assert callable(getattr(nrs.Context, name)), name
    assert callable(FL.GpuBackend.flow_cluster)
    assert inspect.signature(FL.MonoInitializer.__init__).parameters["cluster_tracks"].default is False


def test_the_oracle_equals_the_stereo_starts_at_three_dimensions():
    """dim = 3: the neighbour matrix and the raw labels of tests/stereo_init_oracle.py on its own hand-made cases"""
    seen = 0
    for case in S.make_cluster_cases():
        if len(case["xyz"]) == 0:
            continue
        nb3 = SO.neighbours(case["xyz"], case["eps"])
        assert np.array_equal(FO.neighbours_nd(case["xyz"], case["eps"]), nb3), case["name"]
        raw, _ = SO.dbscan3d_raw(case["xyz"], case["eps"], case["min_points"], nb=nb3)
        label, counts = FO.dbscan_nd(case["xyz"], case["eps"], case["min_points"])
        assert np.array_equal(label, raw) and counts[1] == (raw < 0).sum() and counts[0] == len(set(raw[raw >= 0])), case["name"]
        seen += 1
    assert seen >= 15
    assert FO.dbscan_nd(np.zeros((0, 3), F32), 1.0)[1].tolist() == [0, 0]


def test_the_eps_rule_is_the_floats():
    assert FO.flow_eps(10) == 1.0 and FO.flow_eps(60) == 6.0
    assert FO.flow_eps(2) == float(F32(0.2)) != 0.2                 # the reference keeps 0.1 * dim in a float


@pytest.mark.parametrize("dim", FC.EDGE_DIM)
def test_word_and_tile_edges_hold(dim):
    for n in FC.EDGE_N:
        c = FC.edge_case(n, dim)
        assert c["data"].shape == (n, dim)
        FC.edge_holds(c)


def test_structure_holds():
    FC.structure_holds(FC.structure_case())


def test_exact_and_near_ties_hold():
    FC.tie_holds(FC.tie_case(False), FC.tie_case(True))


def test_order_sensitive_pairs_hold():
    FC.order_holds(FC.order_case())


def test_nonfinite_chunk_and_wide_hold():
    FC.nonfinite_holds(FC.nonfinite_case())
    FC.chunk_holds(FC.chunk_case())
    FC.wide_holds(FC.wide_case())
    FC.big_then_tiny_holds(FC.big60_case(), FC.tiny_case())


@pytest.mark.parametrize("length,quantised", [(2, True), (31, True), (5, False)])
def test_track_cases_hold(length, quantised):
    FC.track_holds(FC.track_case(length, quantised))


def test_the_sequential_pass_is_the_fixed_point_definition():
    """the rule the device is written to (components of the core points, a border point to its lowest core neighbour's label) against the
    sequential pass, on the cases where the two could part: a border point of two clusters, ties, the order-sensitive pairs"""
    for name in ("structure", "exact_ties", "order_sensitive", "nonfinite"):
        c = FC.point_case(name)
        nb, core = c["nb"], c["core"]
        n = len(nb)
        lab = np.where(core, np.arange(n), n)
        while True:
            new = lab.copy()
            for i in np.nonzero(core)[0]:
                m = nb[i] & core
                if m.any():
                    new[i] = min(lab[i], lab[m].min())
            if np.array_equal(new, lab):
                break
            lab = new
        rid = {r: k for k, r in enumerate(sorted({int(v) for v in lab[core]}))}
        want = np.array([rid[int(lab[i])] if core[i] else min([rid[int(v)] for v in lab[nb[i] & core]], default=-1) for i in range(n)], np.int32)
        assert np.array_equal(want, c["label"]), name


def test_flowc_check_runs_clean_and_its_texts_are_the_librarys(lib_built):
    """`make flowc_check`: csrc/nrs_flowc_host.hpp under AddressSanitizer + UBSan in a program of its own; the refusals' formats it prints
    are the strings the library holds"""
    p = subprocess.run(["make", "-C", PKG, "flowc_check"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "flowc_check OK" in p.stdout, p.stdout + p.stderr
    exe = os.path.join(PKG, "flowc_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "flowc_check OK" and not r.stderr, r.stdout + r.stderr
    texts = subprocess.run([exe, "--texts"], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert len(texts) == 6 and all(t.startswith("%s: ") for t in texts)
    for word in ("n = %d (0 .. %d)", "dim = %d (1 .. %d)", "length = %d keypoints (2 .. %d)", "null pointer", "eps = %g is not a positive finite number",
                 "min_points = %d (at least 1)"):
        assert sum(word in t for t in texts) == 1, word
    blob = open(lib_built.LIB_PATH, "rb").read()
    for t in texts:
        assert t.encode() + b"\0" in blob, t
    for name in NEW:
        assert name.encode() + b"\0" in blob                       # ... and the names the formats are filled with


# ---- MonoInitializer over a backend that is the oracle
class FakeBackend:
    """120 features on a grid; per image the first 60 move by (0.8, 0.1), the next 50 by (-0.5, 0.6), the last 10 by (3 k, -2 k) px for
    feature k (no two alike).  Feature `lose` fails on image `lose_at` and stays lost, as with the tracker.  init_essential: verdict 2 until
    image `start_at`, then every feature with an even index triangulated."""

    def __init__(self, lose=7, lose_at=2, start_at=3):
        self.lose, self.lose_at, self.start_at, self.image = lose, lose_at, start_at, 0
        self.cluster_calls = []
        n = 120
        self.step = np.zeros((n, 2), F32)
        self.step[:60] = (0.8, 0.1)
        self.step[60:110] = (-0.5, 0.6)
        self.step[110:] = np.stack([3.0 * np.arange(1, 11), -2.0 * np.arange(1, 11)], 1)
        self.xy0 = np.stack([20.0 + 25 * (np.arange(n) % 12), 20.0 + 20 * (np.arange(n) // 12)], 1).astype(F32)

    def extract_features(self, im, held_xy, mask=None):
        return self.xy0.copy(), np.arange(len(self.xy0))

    def klt_set_reference(self, im, kp):
        self.image = 0

    def klt_track(self, im, kp, status, min_ssim):
        self.image += 1
        st = np.asarray(status, np.int32).copy()
        if self.image >= self.lose_at:
            st[self.lose] = FL.BAD
        xy = np.asarray(kp, F32).copy()
        xy[st == FL.TRACKED] += self.step[st == FL.TRACKED]
        return xy, st

    def init_essential(self, ref_xy, cur_xy, status, n_matches, **options):
        n = len(status)
        ok = self.image >= self.start_at
        code = np.where(np.arange(n) % 2 == 0, 0, 1).astype(np.int32)
        return dict(verdict=0 if ok else 2, code=code, xyz=np.ones((n, 3), F32), pose_q=np.array([0, 0, 0, 1], F32), pose_t=np.array([1, 0, 0], F32))

    def flow_cluster(self, tracks):
        self.cluster_calls.append(np.array(tracks, F32))
        return FO.flow_tracks_cluster(tracks)[0]


def _run(cluster_tracks):
    b = FakeBackend()
    mo = FL.MonoInitializer(b, min_tracks=100, cluster_tracks=cluster_tracks)
    results = [mo.process_new_image(None) for _ in range(4)]        # the reset image and three more
    return b, mo, results


def test_mono_initializer_clusters_the_full_length_tracks():
    b, mo, results = _run(True)
    assert [e["reset"] for e in mo.log] == [True, False, False, False] and [r is None for r in results] == [True, True, True, False]
    assert "full_tracks" not in mo.log[0] and len(b.cluster_calls) == 3       # not on the "just reset" image; before the solve on every other
    for f, e in enumerate(mo.log[1:], 1):
        full, labels = e["full_tracks"], e["feature_labels"]
        want = np.arange(120) if f < b.lose_at else np.delete(np.arange(120), b.lose)
        assert full.dtype == np.int32 and np.array_equal(full, want) and len(labels) == len(full)            # ascending; the lost feature is out
        tr = b.cluster_calls[f - 1]
        assert tr.shape == (len(full), f + 1, 2)                    # f + 1 keypoints: the reset image's and one per image since
        assert np.array_equal(tr[:, 0], b.xy0[full]) and np.array_equal(tr[:, -1], e["cur_xy"][full])
        assert np.array_equal(labels, FO.flow_tracks_cluster(tr)[0])
        by_feature = dict(zip(full.tolist(), labels.tolist()))
        a, c = by_feature[0], by_feature[60]
        assert a >= 0 and c >= 0 and a != c                          # the two motions are two clusters, the ten others noise
        assert all(by_feature[k] == a for k in range(60) if k in by_feature) and all(by_feature[k] == c for k in range(60, 110))
        assert all(by_feature[k] == -1 for k in range(110, 120))
    res, last = results[3], mo.log[3]
    assert np.array_equal(res["index"], np.array([k for k in range(0, 120, 2)]))            # even features; 7 is odd, so none of them is the lost one
    by_feature = dict(zip(last["full_tracks"].tolist(), last["feature_labels"].tolist()))
    assert res["track_labels"].dtype == np.int32 and res["track_labels"].tolist() == [by_feature[int(k)] for k in res["index"]]
    assert set(res["track_labels"].tolist()) == {by_feature[0], by_feature[60], -1}


def test_mono_initializer_drops_a_lost_feature_from_the_result_and_the_tracks():
    """the lost feature has an even index here: it is triangulated by the fake solve but its track is short, so it is in neither list"""
    b = FakeBackend(lose=8)
    mo = FL.MonoInitializer(b, min_tracks=100, cluster_tracks=True)
    res = [mo.process_new_image(None) for _ in range(4)][3]
    assert 8 not in res["index"] and 8 not in mo.log[3]["full_tracks"] and len(res["track_labels"]) == len(res["index"]) == 59


def test_mono_initializer_without_clustering_logs_what_it_always_did():
    b, mo, results = _run(False)
    assert b.cluster_calls == [] and mo.history == []
    assert set(mo.log[0]) == {"reset", "n_features", "n_tracks", "verdict"}
    for e in mo.log[1:3]:
        assert set(e) == {"reset", "n_features", "n_tracks", "verdict", "ref_xy", "cur_xy", "status"}
    assert set(mo.log[3]) == {"reset", "n_features", "n_tracks", "verdict", "ref_xy", "cur_xy", "status", "n_map_points"}
    assert set(results[3]) == {"index", "reference_keypoints", "current_keypoints", "reference_landmark_positions", "current_landmark_positions",
                               "pose_q", "pose_t"}
    # and the clustering changes nothing else: the same entries and the same result next to the new keys
    _, mo2, results2 = _run(True)
    for e, e2 in zip(mo.log, mo2.log):
        assert set(e2) - set(e) <= {"full_tracks", "feature_labels"}
        for k, v in e.items():
            assert np.array_equal(v, e2[k]), k
    for k, v in results[3].items():
        assert np.array_equal(v, results2[3][k]), k
    assert set(results2[3]) - set(results[3]) == {"track_labels"}


def test_mono_initializer_with_no_full_length_track_logs_empty_arrays():
    class LosesAll(FakeBackend):
        def klt_track(self, im, kp, status, min_ssim):
            xy, st = super().klt_track(im, kp, status, min_ssim)
            if self.image == 2:
                st[:] = FL.BAD                                       # every feature fails on the second image
            return xy, st
    b = LosesAll()
    mo = FL.MonoInitializer(b, min_tracks=0, cluster_tracks=True)   # (no renewal of the reference for too few tracks)
    for _ in range(3):
        assert mo.process_new_image(None) is None
    assert [e["reset"] for e in mo.log] == [True, False, False] and len(mo.log[1]["full_tracks"]) == 120
    full, labels = mo.log[2]["full_tracks"], mo.log[2]["feature_labels"]
    assert full.dtype == np.int32 and labels.dtype == np.int32 and len(full) == 0 and len(labels) == 0
    assert len(b.cluster_calls) == 1                                # the backend is not asked about nothing
