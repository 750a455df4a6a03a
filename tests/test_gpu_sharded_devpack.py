"""GPU: the device-side problem construction (csrc/nrs_engine_devpack.hpp) on a communicator -- every rank of a sharded plain BA
window builds its own share on the device: the window's row layout, then the incidence records, halo lists and chi2 edge lists of
its own keyframe range only, and the shard fields from the device-built halo lists.

Held against the host construction of the same rank (NRS_HOST_PACK=1, csrc/nrs_engine_setup.hpp), which it must reproduce BIT FOR
BIT: the checksums of every packed array (nrs_dba_pack_hash; a row-limited rank hashes the rows it holds) and the solves on top of
the two.  Nothing here has a tolerance: the two constructions feed the same kernels the same bytes.

The ranks are threads of this process on the one GPU of the test box (nrs.LocalGroup), as in tests/test_gpu_sharded.py; the runner
here also returns the pack hashes and can take the one-call window entry point.  Shapes: 600 x 8 (6144 padded rows: T = 8, the
two-kernel form the device packer never produced before), 400 x 7 with the KB8 camera and three ranks (uneven split), 600 x 16
over four ranks (interior ranks with two ghost keyframes: row-limited arrays), a communicator of one, and 1100 x 26 = 33 280
padded rows, the T = 2 layout (every point observed in every keyframe it projects into, dropout = 0: with the generator's default
5 % a keyframe of 1100 points keeps fewer than 1024 and the window stays below the 32768 rows where T changes)."""
import threading

import numpy as np
import pytest

import nrs
import nrs_synth as S

gpu = pytest.mark.gpu

NAMES = ["vrow", "ss_ptr", "sd_ptr", "s_om", "s_d0", "d_hdr", "d_w", "halo_ptr", "halo_rows", "halo_ns", "tile_list", "ec_sp", "ec_dm", "ec_w",
         "rflag", "uv", "xl_init", "pose_init", "grp_pose", "pose_grp_ptr", "scalars", "(path)", "tile_desc", "halo_fix"]
JOIN_S = 120

_problems, _runs = {}, {}


def _setup(n, k, seed, model=S.PINHOLE, dropout=None):
    key = (n, k, seed, model, dropout)
    if key not in _problems:
        p = S.make_dba_problem(n, k, seed, model) if dropout is None else S.make_dba_problem(n, k, seed, model, dropout=dropout)
        e = nrs.dba_build_edges(p["kf_points"], p["nbr"])
        cam = nrs.make_camera(p["model"], p["prm"])
        qt = np.concatenate([p["poses_q"], p["poses_t"]], 1)
        _problems[key] = (p, e, cam, qt)
    return _problems[key]


def _run_ranks(world, rank_main):
    """rank_main(r, ctx) -> result of rank r; every thread is joined with a time limit and a rank that did not finish fails the test"""
    group = nrs.LocalGroup(world)
    out, errs = [None] * world, []

    def main(r):
        try:
            c = nrs.Context()
            c.comm_init_local(group, r)
            out[r] = rank_main(r, c)
            c.close()
        except Exception as ex:                      # (a failed rank would leave the others in the barrier)
            errs.append((r, ex))
            raise

    th = [threading.Thread(target=main, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(JOIN_S)
    assert not errs, errs
    assert not any(t.is_alive() for t in th) and all(o is not None for o in out), "a rank did not finish"
    group.close()
    return out


def _trials(tr):
    return [(t["accepted"], t["lam"], t["chi"], t["chi_new"]) for t in tr]


def _run(world, shape, host, solve=False, switches=(), edges=None):
    """One sharded window, device-packed or under NRS_HOST_PACK=1; per rank: pack hash, stats and -- solve=True -- optimize(5), a
    reset and optimize(5) again, download, residual taps.  Computed once per argument set and shared by the tests (never modified)."""
    key = (world, shape, host, solve, tuple(switches), edges is not None)
    if key in _runs:
        return _runs[key]
    p, e, cam, qt = _setup(*shape)
    e = edges if edges is not None else e
    nrs.debug_set("NRS_HOST_PACK", "1" if host else None)
    for name in switches:
        nrs.debug_set(name, "1")

    def rank_main(r, c):
        assert c.comm_rank() == (r, world)
        c.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"])
        res = dict(hash=c.dba_pack_hash(), stats=c.dba_stats())
        if solve:
            tr = nrs.Trace(64)
            c.dba_optimize(5, tr)
            c.dba_reset()
            tr = nrs.Trace(64)
            c.dba_optimize(5, tr)
            res["trials"] = _trials(tr.trials)
            res["pq"], res["xyz"] = c.dba_download()
            res["taps"] = c.dba_residuals()
        return res

    try:
        out = _run_ranks(world, rank_main)
    finally:
        nrs.debug_set("NRS_HOST_PACK", None)
        for name in switches:
            nrs.debug_set(name, None)
    _runs[key] = out
    return out


def _same_solve(a, b):
    assert a["trials"] == b["trials"]
    assert all(np.isfinite(t[2]) and np.isfinite(t[3]) for t in a["trials"])
    assert np.array_equal(a["pq"], b["pq"]) and np.array_equal(a["xyz"], b["xyz"])
    for x, y in zip(a["taps"], b["taps"]):
        assert np.array_equal(x, y)


BASE = (600, 8, 47, S.PINHOLE)
SHAPES = [(2, (600, 8, 47, S.PINHOLE)), (3, (400, 7, 42, S.KB8)), (4, (600, 16, 45, S.PINHOLE)), (1, (600, 8, 47, S.PINHOLE)),
          (2, (1100, 26, 49, S.PINHOLE, 0.0))]
SOLVED = [(2, (600, 8, 47, S.PINHOLE)), (4, (600, 16, 45, S.PINHOLE))]


@gpu
def test_every_rank_builds_its_share_on_the_device():
    out = _run(4, BASE, host=False, solve=True)
    assert [o["hash"][21] for o in out] == [1, 1, 1, 1]


@gpu
@pytest.mark.parametrize("world,shape", SHAPES)
def test_rank_device_pack_is_the_rank_host_pack(world, shape):
    solve = (world, shape) in SOLVED or (world, shape) == (4, BASE)
    dev = _run(world, shape, host=False, solve=solve)
    hst = _run(world, shape, host=True, solve=solve)
    if shape[0] == 1100:
        assert dev[0]["stats"]["rows"] == 33280, "this shape is the T = 2 layout at 33 280 padded rows"
    for r in range(world):
        assert dev[r]["hash"][21] == 1 and hst[r]["hash"][21] == 0, "the two runs must take the two constructions"
        bad = [nm for i, nm in enumerate(NAMES) if i != 21 and dev[r]["hash"][i] != hst[r]["hash"][i]]
        assert not bad, (r, bad)
        assert dev[r]["stats"] == hst[r]["stats"]


@gpu
@pytest.mark.parametrize("world,shape,full", [(2, SOLVED[0][1], False), (4, SOLVED[1][1], False), (4, SOLVED[1][1], True)])
def test_rank_device_pack_solves_as_the_rank_host_pack(world, shape, full):
    sw = ("NRS_SHARD_FULL_VECTORS",) if full else ()
    dev = _run(world, shape, host=False, solve=True, switches=sw)
    hst = _run(world, shape, host=True, solve=True, switches=sw)
    for r in range(world):
        assert dev[r]["hash"][21] == 1 and hst[r]["hash"][21] == 0
        _same_solve(dev[r], hst[r])
        _same_solve(dev[r], dev[0])                  # ... and every rank holds the same complete result
    if full:                                         # (the switch took: full-length per-row arrays are larger than the row-limited ones)
        own = _run(world, shape, host=False, solve=True)
        assert min(o["stats"]["device_bytes"] for o in dev) > max(o["stats"]["device_bytes"] for o in own)


@gpu
def test_a_device_packed_rank_holds_only_its_keyframe_range(ctx):
    p, e, cam, qt = _setup(*BASE)
    nrs.debug_set("NRS_HOST_PACK", None)
    ctx.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"])
    whole = ctx.dba_stats()
    assert whole["packed_rows"] == whole["rows"]
    world = 4
    out = _run(world, BASE, host=False, solve=True)
    st = [o["stats"] for o in out]
    assert all(o["hash"][21] == 1 for o in out)
    kb = nrs.shard_plan(8, p["lm_kf"], world)
    assert sum(x["packed_rows"] for x in st) == whole["rows"]                      # the ranges tile the window
    assert sum(x["spring_slots"] for x in st) <= whole["spring_slots"] + 64 * 4 * world
    assert sum(x["damper_slots"] for x in st) <= whole["damper_slots"] + 64 * 4 * world
    for r in range(world):
        own_kf = np.isin(p["lm_kf"], np.arange(kb[r], kb[r + 1]))
        assert st[r]["rows"] == whole["rows"] and own_kf.sum() <= st[r]["packed_rows"] < own_kf.sum() + 256 * (kb[r + 1] - kb[r])
        assert st[r]["spring_slots"] < 0.45 * whole["spring_slots"] and st[r]["damper_slots"] < 0.45 * whole["damper_slots"]
        assert st[r]["device_bytes"] < 0.6 * whole["device_bytes"]


@gpu
def test_solve_window_on_a_communicator_is_the_step_by_step_solve():
    p, e, cam, qt = _setup(*BASE)
    nrs.debug_set("NRS_HOST_PACK", None)

    def rank_main(r, c):
        tr = nrs.Trace(64)
        pq, xyz = c.dba_solve_window(cam, qt, p["kf_points"], p["lm_xyz"], p["lm_uv"], p["nbr"], p["scale"], 5, tr)
        h = c.dba_pack_hash()
        ed = c.dba_window_edges()
        c.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"])
        h2 = c.dba_pack_hash()
        tr2 = nrs.Trace(64)
        c.dba_optimize(5, tr2)
        pq2, xyz2 = c.dba_download()
        return dict(pq=pq, xyz=xyz, hash=h, edges=ed, trials=_trials(tr.trials), pq2=pq2, xyz2=xyz2, hash2=h2, trials2=_trials(tr2.trials))

    out = _run_ranks(2, rank_main)
    for o in out:
        assert o["hash"][21] == 1 and o["hash2"][21] == 1
        assert o["edges"] is not None, "the one call should have built its edge lists on the device"
        for key in ("sp_ij", "sp_d0", "dm_idx", "dm_w"):
            assert np.array_equal(o["edges"][key], e[key]), key
        assert [h for i, h in enumerate(o["hash"]) if i != 21] == [h for i, h in enumerate(o["hash2"]) if i != 21]
        assert o["trials"] == o["trials2"]
        assert np.array_equal(o["pq"], o["pq2"]) and np.array_equal(o["xyz"], o["xyz2"].astype(np.float32))   # (OPT:1158: the one call returns floats)
        assert np.array_equal(o["pq"], out[0]["pq"]) and np.array_equal(o["xyz"], out[0]["xyz"])


SMALL = (150, 4, 50, S.PINHOLE)


def test_the_small_window_of_the_fallback_test_is_below_the_row_threshold(lib_built):
    """(CPU form of the fallback case: the window the GPU test expects on the host path has 4 x 256 = 1024 padded rows, below the
    2048 the device construction asks for, and its two ranks get two keyframes each)"""
    p = S.make_dba_problem(*SMALL)
    cnt = np.bincount(p["lm_kf"], minlength=4)
    assert sum(max(1, -(-int(n) // 256)) * 256 for n in cnt) == 1024
    assert list(nrs.shard_plan(4, p["lm_kf"], 2)) == [0, 2, 4]


@gpu
def test_small_sharded_windows_keep_the_host_path():
    dev = _run(2, SMALL, host=False, solve=True)
    hst = _run(2, SMALL, host=True, solve=True)
    for r in range(2):
        assert dev[r]["hash"][21] == 0 and hst[r]["hash"][21] == 0
        assert dev[r]["hash"] == hst[r]["hash"]
        _same_solve(dev[r], hst[r])
        assert any(t[0] for t in dev[r]["trials"])                   # it still solves: steps are accepted


@gpu
@pytest.mark.parametrize("host", [False, True])
def test_an_incomplete_damper_never_reaches_the_device_pack(host):
    """A damper with an absent vertex (-1) is valid for the engine's host construction only.  The window upload refuses such a list
    on every rank alike, before either construction and without a collective (NRS_ERR_INVALID, as under NRS_HOST_PACK=1): no rank is
    left waiting, and the same ranks then take the intact window -- device-packed unless the switch is set."""
    p, e, cam, qt = _setup(*BASE)
    bad = dict(e, dm_idx=np.array(e["dm_idx"], np.int32).copy())
    bad["dm_idx"].reshape(-1, 4)[len(bad["dm_idx"].reshape(-1, 4)) // 2, 3] = -1
    nrs.debug_set("NRS_HOST_PACK", "1" if host else None)

    def rank_main(r, c):
        with pytest.raises(nrs.NrsError) as ei:
            c.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], bad, p["scale"])
        c.dba_upload(cam, qt, p["lm_xyz"], p["lm_kf"], p["lm_uv"], e, p["scale"])
        return dict(code=ei.value.code, text=str(ei.value), hash=c.dba_pack_hash())

    out = _run_ranks(2, rank_main)
    ref = _run(2, BASE, host=host)
    for r in range(2):
        assert out[r]["code"] == -1 and "damper index out of range" in out[r]["text"]
        assert out[r]["hash"][21] == (0 if host else 1)
        assert out[r]["hash"] == ref[r]["hash"]


@gpu
def test_no_stray_write_under_poison():
    """NRS_POISON=1 fills a fresh arena with 0xFF (a read of memory nobody wrote shows up as NaN), NRS_CHECK_EVAL=1 evaluates every
    trial state twice and compares the bits: the device-packed ranks -- row-limited arrays, bounded launches -- run as without them."""
    plain = _run(4, BASE, host=False, solve=True)
    pois = _run(4, BASE, host=False, solve=True, switches=("NRS_POISON", "NRS_CHECK_EVAL"))
    for r in range(4):
        assert pois[r]["hash"][21] == 1
        assert all(np.isfinite(t[2]) and np.isfinite(t[3]) for t in pois[r]["trials"])
        _same_solve(pois[r], plain[r])
