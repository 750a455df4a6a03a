"""GPU: the Lucas-Kanade case table (tests/lk_cases.py, vetted on the CPU by tests/test_lk_cases_cpu.py) through the C ABI against
oracle/lk_oracle.py -- short pyramids, odd level sizes, dead windows, the three border gates, bad numbers, configurations other than
the default, all six input statuses -- and the paths of nrs_klt_* the other files do not compare: a row stride, one context across
image sizes, template growth across a capacity step and the resident hand-over on short-pyramid frames.

Bars (tests/test_gpu_klt.py states them): templates, derivative templates, means, validity, status, n_good and positions exact (NaN
positions included); SSIM 1e-5 absolute where the oracle's value is finite.  The window contents of a (point, level) that holds no
template are not defined (the buffer keeps what it held); its means are -1 and its flag 0, and those are compared."""
import ctypes as C

import numpy as np
import pytest

import lk_cases as LC
import nrs

pytestmark = pytest.mark.gpu

KEYS = ("max_level", "max_iters", "epsilon", "min_eig")


def _configure(c, cfg):
    c.klt_clear()
    c.klt_configure(21, *[cfg[k] for k in KEYS])


def _stack(ts):
    return {k: np.stack([t[k] for t in ts]) for k in ("gray", "grad", "mean", "valid")}


def _run(c, case, **cfg):
    """set-reference, every template in ONE read, track"""
    _configure(c, dict(case["cfg"], **cfg))
    c.klt_set_reference(case["im0"], case["pts"], case["mask"])
    n = len(case["pts"])
    assert c.klt_num_points() == n
    t = _stack(c.klt_get_templates(0, n))
    return t, c.klt_track(case["im1"], case["guess"], case["status"], case["initial_flow"], case["min_ssim"])


def _same_templates(t, ref, tag=""):
    assert np.array_equal(t["valid"], ref["valid"]), tag
    assert np.array_equal(t["mean"], ref["mean"]), tag
    ok = ref["valid"] != 0
    assert np.array_equal(t["gray"][ok], ref["gray"][ok]), tag
    assert np.array_equal(t["grad"][ok], ref["grad"][ok]), tag


def _same_track(r, ref, ssim_atol, tag=""):
    xy, st, good, ssim = r
    oxy, ost, ogood, ossim = ref
    assert np.array_equal(st, ost), (tag, st.tolist(), ost.tolist())
    assert good == ogood, tag
    assert np.array_equal(xy, oxy, equal_nan=True), (tag, np.argwhere(~((xy == oxy) | (np.isnan(xy) & np.isnan(oxy))))[:4].tolist())
    m = np.isfinite(ossim)                                                          # (a point that did not reach the gate: not written)
    if ssim_atol == 0.0:                                                            # against another device run: the points that passed it
        m &= np.isin(ost, LC.USABLE)
    assert np.allclose(ssim[m], ossim[m], atol=ssim_atol, rtol=0), tag


def _restore(c):
    c.klt_clear()
    c.klt_configure()


@pytest.mark.parametrize("name", LC.NAMES)
def test_case_matches_oracle(ctx, name):
    case = LC.case(name)
    ot, oref = LC.oracle(name)
    try:
        t, r = _run(ctx, case)
        _same_templates(t, ot, name)
        _same_track(r, oref, 1e-5, name)
        un = ~np.isin(case["status"], LC.USABLE)                                    # unusable points: the guess's bits, the input status
        assert np.array_equal(r[0][un].view(np.uint32), case["guess"][un].view(np.uint32)) and np.array_equal(r[1][un], case["status"][un])
    finally:
        _restore(ctx)


@pytest.mark.parametrize("name", LC.SHORT)
def test_short_pyramid_is_the_tracker_of_its_top_level(ctx, name):
    """on a pyramid of k levels, max_level >= k returns bit for bit the xy, status, n_good and SSIM of max_level = k - 1"""
    case = LC.case(name)
    h, w = case["im0"].shape
    k = LC.n_levels(w, h, case["cfg"]["max_level"])
    try:
        t, r = _run(ctx, case)
        t2, r2 = _run(ctx, case, max_level=k - 1)
        assert np.all(t["valid"][:, k:] == 0) and np.all(t["mean"][:, k:] == -1)    # levels that were not built: invalid, means -1
        _same_templates({x: v[:, :k] for x, v in t.items()}, t2, name)
        _same_track(r, r2, 0.0, name)
    finally:
        _restore(ctx)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def test_row_stride(ctx):
    """image rows w + 37 bytes apart, the slack filled with 255, through the raw entry points: the packed image's templates and tracks"""
    case = LC.case("short_161x123")
    h, w = case["im0"].shape
    n = len(case["pts"])
    try:
        t_ref, r_ref = _run(ctx, case)
        pad0, pad1 = np.full((h, w + 37), 255, np.uint8), np.full((h, w + 37), 255, np.uint8)
        pad0[:, :w], pad1[:, :w] = case["im0"], case["im1"]
        _configure(ctx, case["cfg"])
        pts = np.ascontiguousarray(case["pts"])
        rc = ctx.lib.nrs_klt_set_reference(ctx.h, _p(pad0, C.c_uint8), C.c_int32(w), C.c_int32(h), C.c_int32(w + 37), None, C.c_int32(n), _p(pts, C.c_float))
        assert rc == 0
        _same_templates(_stack(ctx.klt_get_templates(0, n)), t_ref)
        xy, st, good, ssim = case["guess"].copy(), case["status"].copy(), C.c_int32(0), np.full(n, np.nan, np.float32)
        rc = ctx.lib.nrs_klt_track(ctx.h, _p(pad1, C.c_uint8), C.c_int32(w), C.c_int32(h), C.c_int32(w + 37), C.c_int32(n), _p(xy, C.c_float),
                                   _p(st, C.c_int32), C.c_int32(1), C.c_float(case["min_ssim"]), C.byref(good), _p(ssim, C.c_float))
        assert rc == 0
        _same_track((xy, st, good.value, ssim), r_ref, 0.0)
        assert good.value > 10
    finally:
        _restore(ctx)


def test_one_context_across_sizes():
    """640 x 480 (5 levels) -> 97 x 45 (max_level 3, 2 levels built) -> 161 x 123 (max_level 2): the pyramid buffers shrink and regrow and
    klt_configure changes the template layout in between; every step equals a fresh context's"""
    import nrs_synth as S
    sq = S.make_lk_sequence(60, 3)
    big = LC._case(sq["im0"], sq["im1"], sq["pts"])
    steps = [(big, {}), (LC.case("short_97x45"), dict(max_level=3)), (LC.case("odd_161x123_l2"), {})]
    one = nrs.Context()
    try:
        for i, (case, cfg) in enumerate(steps):
            t, r = _run(one, case, **cfg)
            fresh = nrs.Context()
            try:
                t2, r2 = _run(fresh, case, **cfg)
            finally:
                fresh.close()
            _same_templates(t, t2, i)
            _same_track(r, r2, 0.0, i)
            assert r[2] > 10
    finally:
        one.close()


def test_template_growth_keeps_the_stored_templates():
    """200 hand-placed points at max_level 0, then nrs_klt_insert_templates of 100 more.  In a context whose first reference held 100
    points the template buffers hold 256 slots (reserve_points: max(n + n / 2, 256)); 200 fit, 300 do not: the buffers are reallocated
    with the stored templates copied.  The first 200 are unchanged bit for bit and tracking all 300 equals the oracle."""
    import lk_oracle as LK
    sq = LC.pair(161, 123, 5)
    first = LC._grid(np.linspace(14, 146, 20), np.linspace(14, 108, 10), 21)
    more = LC._grid(np.linspace(17, 143, 10), np.linspace(19, 103, 10), 22)
    allp = np.concatenate([first, more])
    c = nrs.Context()
    try:
        c.klt_configure(21, 0)
        c.klt_set_reference(sq["im0"], more)
        extra = c.klt_get_templates(0, 100)
        c.klt_set_reference(sq["im0"], first)
        before = _stack(c.klt_get_templates(0, 200))
        c.klt_insert_templates(extra)
        assert c.klt_num_points() == 300
        after = c.klt_get_templates(0, 300)
        assert np.array_equal(np.stack([t["xy"] for t in after]), allp)
        after = _stack(after)
        for k in ("gray", "grad", "mean", "valid"):
            assert np.array_equal(after[k][:200], before[k]), k
        lk = LK.LucasKanadeOracle(max_level=0)
        lk.set_reference(sq["im0"], allp)
        _same_templates(after, LC.oracle_templates(lk))
        assert after["valid"].all()
        st = np.zeros(300, np.int32)
        guess = allp + np.float32(0.7)
        r = c.klt_track(sq["im1"], guess, st)
        _same_track(r, lk.track(sq["im1"], guess.copy(), st), 1e-5)
        assert r[2] > 200
    finally:
        c.close()


@pytest.mark.parametrize("wh", [(161, 123), (97, 45)], ids=lambda s: "%dx%d" % s)
def test_resident_track_on_a_short_pyramid(wh):
    """nrs_klt_set_reference_front / nrs_klt_track_front on frames whose pyramid is shorter than the default configuration's five
    levels: the bits of the host-pointer calls, and of the oracle (an RGB frame of three equal channels has itself as its grey image)"""
    name = "short_%dx%d" % wh
    case = LC.case(name)
    ot, oref = LC.oracle(name)
    n = len(case["pts"])
    dev, host = nrs.Context(), nrs.Context()
    try:
        th, rh = _run(host, case)
        _configure(dev, case["cfg"])
        dev.front_configure([])
        o0 = dev.front_process(np.ascontiguousarray(np.repeat(case["im0"][:, :, None], 3, 2)), outputs=("gray",))
        assert np.array_equal(o0["gray"], case["im0"])
        dev.klt_set_reference_front(case["pts"], nrs.FRONT_GRAY, False)
        td = _stack(dev.klt_get_templates(0, n))
        assert dev.front_process(np.ascontiguousarray(np.repeat(case["im1"][:, :, None], 3, 2)), outputs=False) == {}
        rd = dev.klt_track_front(case["guess"], case["status"], nrs.FRONT_GRAY, initial_flow=True, min_ssim=case["min_ssim"])
        _same_templates(td, th, name)
        _same_track(rd, rh, 0.0, name)
        _same_templates(td, ot, name)
        _same_track(rd, oref, 1e-5, name)
    finally:
        dev.close()
        host.close()
