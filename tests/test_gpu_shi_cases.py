"""GPU: the Shi-Tomasi case table (tests/shi_cases.py, vetted on the CPU by tests/test_shi_cases_cpu.py) through nrs_shi_extract and
nrs_shi_extract_front against oracle/shi_oracle.py -- ties, rows denser than a wave and than a 256-column chunk, marks in cells the score
pass never writes, 3000 held points, a size change inside one extractor, the last-row pass at w == h, w == h + 1 and h == 5, scores either
side of the threshold, saturated gradients and a NaN score -- and the refusal of a held point that rounds outside the image.

Bars: n, xy and ids equal after every call, and the extractor's three buffers equal to the oracle's bit for bit.  The one cell of the table
whose score is NaN is compared as NaN: the sign and payload of the NaN of an invalid square root are not defined, and nothing reads them."""
import numpy as np
import pytest

import nrs
import shi_cases as SC
import shi_oracle as SH

pytestmark = pytest.mark.gpu

INVALID = -1


def _same_bits(sc, xg, yg, ex, tag):
    assert xg.tobytes() == ex.Xg.tobytes() and yg.tobytes() == ex.Yg.tobytes(), tag
    nan = np.isnan(ex.scores)
    assert np.array_equal(np.isnan(sc), nan), tag
    bad = np.argwhere((sc.view(np.uint32) != ex.scores.view(np.uint32)) & ~nan)
    assert len(bad) == 0, (tag, len(bad), bad[:4].tolist(), sc[tuple(bad[0])], ex.scores[tuple(bad[0])])


def _same_keypoints(got, oxy, oids, cap, tag):
    xy, ids, n = got
    assert n == len(oxy), (tag, n, len(oxy))
    assert len(xy) == len(ids) == min(n, cap), tag
    assert np.array_equal(xy, oxy[:cap]) and np.array_equal(ids, oids[:cap]), tag


def _through(ctx, ex, calls, capacity=None):
    for k, (im, held, mask) in enumerate(calls):
        cap = (capacity or {}).get(k, im.size)
        got = ctx.shi_extract(im, held, mask, capacity=cap)
        oxy, oids = ex.extract(im, held, mask)
        _same_keypoints(got, oxy, oids, cap, k)
        _same_bits(*ctx.shi_buffers(), ex, k)


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_matches_oracle(ctx, name):
    case = SC.BY_NAME[name]
    ctx.shi_configure(case["nms"])
    _through(ctx, SH.ShiTomasi(case["nms"]), case["calls"], case["capacity"])


@pytest.mark.parametrize("tag,held", SC.REFUSALS, ids=[r[0] for r in SC.REFUSALS])
def test_refusal_changes_nothing(ctx, tag, held):
    """a held point that rounds outside the image, or is not finite, behind a good one: INVALID, the buffers as they were, and the next
    call numbered as if the refused one had not been made"""
    ctx.shi_configure(3)
    ex = SH.ShiTomasi(3)
    other = SC.noise(SC.W, SC.H, 32)
    _through(ctx, ex, [(SC.REFUSAL_IMAGE, held[:1], None)])
    before = [b.tobytes() for b in ctx.shi_buffers()]
    for im in (other, SC.noise(50, 30, 33)):                        # at the extractor's size, and at one that would resize it
        with pytest.raises(nrs.NrsError) as ei:
            ctx.shi_extract(im, held)
        assert ei.value.code == INVALID
        assert [b.tobytes() for b in ctx.shi_buffers()] == before
    first = ex.next_id
    assert first > 0
    _through(ctx, ex, [(other, held[:1], None)])
    xy, ids, n = ctx.shi_extract(other, held[:1])
    assert n > 0 and ids[0] == ex.next_id > first                    # (and once more, past the oracle: the counter only ever grew by n)


def _partial(im):
    """the image with its values capped below the bright threshold outside columns 90..189: the Global mask is zero around that band only"""
    out = np.minimum(im, 199).astype(np.uint8)
    out[:, 90:190] = im[:, 90:190]
    return out


@pytest.mark.parametrize("name,edit", [("ties_checker2", None), ("dense_rows_300x8", None), ("dense_rows_300x8", _partial)],
                         ids=["ties_checker2", "dense_rows_300x8", "dense_rows_300x8_partial"])
def test_resident_entry_equals_host_entry_and_oracle(name, edit):
    """nrs_shi_extract_front on the resident grey image under the resident Global mask of a BrightFilter at 200: the bits of nrs_shi_extract
    given the downloaded image and mask, and of the oracle.  On the table's own images the filter's eroded, blurred mask is zero everywhere
    (every keypoint, thousands over the calls, is dropped by front_mask_at and the ids still advance); the `partial` edit keeps the bright
    pixels to a band of columns, so that some keypoints are dropped and some are kept."""
    case = SC.BY_NAME[name]
    dev, host = nrs.Context(), nrs.Context()
    try:
        for c in (dev, host):
            c.shi_configure(case["nms"])
        dev.front_configure([("bright", 200)])
        ex = SH.ShiTomasi(case["nms"])
        dropped = kept = 0
        for k, (im, held, _) in enumerate(case["calls"]):
            im = im if edit is None else edit(im)
            o = dev.front_process(im, outputs=("gray", "global"))
            assert np.array_equal(o["gray"], im) and (o["global"] == 0).any()
            d = dev.shi_extract_front(held, nrs.FRONT_GRAY, True, capacity=im.size)
            first = ex.next_id
            oxy, oids = ex.extract(o["gray"], held, o["global"])
            _same_keypoints(d, oxy, oids, im.size, k)
            _same_keypoints(host.shi_extract(o["gray"], held, o["global"], capacity=im.size), oxy, oids, im.size, k)
            _same_bits(*dev.shi_buffers(), ex, k)
            _same_bits(*host.shi_buffers(), ex, k)
            dropped += ex.next_id - first - d[2]
            kept += d[2]
        print(name, "dropped by the mask:", dropped, "kept:", kept)
        assert dropped >= 1000 and (kept > 100 if edit is not None else kept == 0)
    finally:
        dev.close()
        host.close()


def test_fresh_extractor_keeps_nothing(ctx):
    """marks_unwritten leaves eight marks that last for the life of the extractor; shi_configure ends that life"""
    case = SC.BY_NAME["marks_unwritten"]
    ctx.shi_configure(case["nms"])
    _through(ctx, SH.ShiTomasi(case["nms"]), case["calls"])
    assert (ctx.shi_buffers()[0] == -1).sum() == len(SC.UNWRITTEN_MARKS)
    ctx.shi_configure(case["nms"])
    ex = SH.ShiTomasi(case["nms"])
    _through(ctx, ex, case["calls"][-1:])
    h, w = case["calls"][-1][0].shape
    assert ex.next_id == (h - 3) * (w - 2) and not (ctx.shi_buffers()[0] == -1).any()
