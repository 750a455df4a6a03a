"""CPU: the Shi-Tomasi case table (tests/shi_cases.py) on the oracle (oracle/shi_oracle.py).  For every case the literal single pass and the
closed form go through all calls of the case and leave the same gradients, scores, keypoints and ids; and every entry of the case's `claims`
is asserted, so that the GPU test (tests/test_gpu_shi_cases.py) is known to reach what the case is named after.  A count the kernel must also
meet is computed here from the case's construction (the written rectangle, 31 x 31 boxes around marks, hand-written rounding), never
read off the oracle's window code.

The literal form is Python loops, and still takes about a second on the slowest case (three dense 64 x 40 calls): it runs on every call of
every case, the 300-wide ones included."""
import numpy as np
import pytest

import shi_cases as SC
import shi_oracle as SH

F32 = np.float32


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _run(case, literal=False, calls=None):
    """[(xy, ids, scores, Xg, Yg)] after every call of the case through one extractor"""
    ex = SH.ShiTomasi(case["nms"])
    out = []
    for im, held, mask in case["calls"][:calls]:
        xy, ids = ex.extract(im, held, mask, literal=literal)
        out.append((xy, ids, ex.scores.copy(), ex.Xg.copy(), ex.Yg.copy()))
    return out


_CLOSED = {}


def closed(name):
    if name not in _CLOSED:
        _CLOSED[name] = _run(SC.BY_NAME[name])
    return _CLOSED[name]


@pytest.mark.parametrize("name", SC.NAMES)
def test_literal_pass_equals_closed_form(name):
    case = SC.BY_NAME[name]
    lit, clo = _run(case, literal=True), closed(name)
    assert len(lit) == len(clo) == len(case["calls"])
    for k, (a, b) in enumerate(zip(lit, clo)):
        assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]), k
        assert _same(a[2], b[2]), k
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), k


# ---- the claims, one checker per key ---------------------------------------------------------------------------------------------------------
def _row_major(cells_map):
    rr, cc = np.nonzero(cells_map)
    return np.stack([cc, rr], 1).astype(F32)


def _boxes(w, h, marks, half=15):
    """cells within `half` of a mark in both axes: the 31 x 31 neighbourhoods, from their geometry"""
    m = np.zeros((h, w), bool)
    for x, y in marks:
        m[max(0, y - half):y + half + 1, max(0, x - half):x + half + 1] = True
    return m


def _expect_exact(case, res, keep_per_call):
    """the keypoints of every call are exactly the cells of keep_per_call[k] in row-major order, numbered before the mask filter"""
    first = 0
    for k, ((im, held, mask), r, keep) in enumerate(zip(case["calls"], res, keep_per_call)):
        xy = _row_major(keep)
        ids = first + np.arange(len(xy))
        first += len(xy)
        if mask is not None:
            sel = mask[xy[:, 1].astype(int), xy[:, 0].astype(int)] != 0
            assert 0 < sel.sum() < len(sel)
            xy, ids = xy[sel], ids[sel]
        assert np.array_equal(r[0], xy) and np.array_equal(r[1], ids), k


def _all_written_pass(im_shape, scores):
    """the condition on the input behind every `dense` claim: no written cell scores below 80 (marked cells aside)"""
    h, w = im_shape
    s = scores[SC.written(w, h)]
    assert np.all((s >= 80) | (s == -1)) and not np.isnan(s).any()


def check_cells_ge80_min(case, res, v):
    n = int((res[0][2] >= 80).sum())
    print(case["name"], "cells >= 80:", n)
    assert n >= v


def check_distinct_scores_max(case, res, v):
    s = res[0][2]
    d = np.unique(s[s >= 80])
    print(case["name"], "distinct scores >= 80:", len(d))
    assert 1 <= len(d) <= v


def check_keypoints_min(case, res, v):
    print(case["name"], "keypoints:", len(res[0][0]))
    assert len(res[0][0]) >= v


def check_adjacent_equal_pair(case, res, v):
    xy, sc = res[0][0].astype(int), res[0][2]
    kp = np.zeros(sc.shape, bool)
    kp[xy[:, 1], xy[:, 0]] = True
    pairs = 0
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        a = kp[:sc.shape[0] - dy, max(0, -dx):sc.shape[1] - max(0, dx)]
        b = kp[dy:, max(0, dx):sc.shape[1] - max(0, -dx)]
        sa = sc[:sc.shape[0] - dy, max(0, -dx):sc.shape[1] - max(0, dx)]
        sb = sc[dy:, max(0, dx):sc.shape[1] - max(0, -dx)]
        pairs += int((a & b & (sa == sb)).sum())
    print(case["name"], "8-adjacent keypoint pairs of equal score:", pairs)
    assert pairs >= 1


def check_dense(case, res, v):
    keep = []
    for (im, _, _), r in zip(case["calls"], res):
        h, w = im.shape
        _all_written_pass(im.shape, r[2])
        keep.append(SC.written(w, h))
        assert keep[-1].sum() == (h - 3) * (w - 2) and np.all(keep[-1][:h - 3].sum(1) == w - 2)
    _expect_exact(case, res, keep)
    for k, cap in case["capacity"].items():
        assert 0 < cap < len(res[k][0])


def check_dense_minus_boxes(case, res, marks_per_call):
    keep = []
    for (im, _, _), r, marks in zip(case["calls"], res, marks_per_call):
        h, w = im.shape
        _all_written_pass(im.shape, r[2])
        keep.append(SC.written(w, h) & ~_boxes(w, h, marks))
        print(case["name"], "keypoints outside the boxes:", int(keep[-1].sum()), "of", (h - 3) * (w - 2))
    # the unwritten marks leave part of the dense set and take part of it; the interior mark takes more on the call that sets it, only
    assert 0 < keep[1].sum() < SC.written(*res[1][2].shape[::-1]).sum() and keep[0].sum() < keep[1].sum() == keep[2].sum()
    _expect_exact(case, res, keep)
    x, y = SC.INTERIOR_MARK
    assert res[0][2][y, x] == -1 and res[1][2][y, x] >= 80 and np.array_equal(res[1][0], res[2][0])
    for x, y in SC.UNWRITTEN_MARKS:
        assert not SC.written(*res[0][2].shape[::-1])[y, x] and all(r[2][y, x] == -1 for r in res)


def check_marked_cells(case, res, cells):
    rr, cc = np.nonzero(res[0][2] == -1)
    assert sorted(zip(cc.tolist(), rr.tolist())) == [tuple(c) for c in cells]
    h, w = res[0][2].shape
    wr = SC.written(w, h)
    left = sorted(c for c in cells if not wr[c[1], c[0]])          # the next call rewrites the others
    rr, cc = np.nonzero(res[1][2] == -1)
    assert sorted(zip(cc.tolist(), rr.tolist())) == [tuple(c) for c in left] and 0 < len(left) < len(cells)


def check_held_min(case, res, v):
    assert len(case["calls"][0][1]) >= v and (len(case["calls"][0][1]) + 255) // 256 > 1


def check_duplicates_min(case, res, v):
    assert len(case["calls"][0][1]) - len(case["claims"]["marked_cells"]) >= v


def check_fresh_at_every_size(case, res, v):
    first = 0
    shapes = [c[0].shape for c in case["calls"]]
    assert all(a != b for a, b in zip(shapes, shapes[1:])) and (res[0][2] == -1).sum() == len(case["calls"][0][1])
    for k, ((im, held, mask), r) in enumerate(zip(case["calls"], res)):
        fresh = SH.ShiTomasi(case["nms"])
        xy, ids = fresh.extract(im, held, mask)
        assert _same(r[2], fresh.scores) and np.array_equal(r[3], fresh.Xg) and np.array_equal(r[4], fresh.Yg), k
        assert np.array_equal(r[0], xy) and np.array_equal(r[1], ids + first) and len(xy) > 0, k
        assert k == 0 or not (r[2] == -1).any()
        first += len(xy)


def check_last_row_memory(case, res, v):
    """the second call's last-row pass reads a non-zero memory: its score row h-4 differs from a fresh extractor's on the same image"""
    im = case["calls"][1][0]
    h, w = im.shape
    assert np.any(res[0][3][h - 1, 2:h - 1] != 0)
    fresh = SH.ShiTomasi(case["nms"])
    fresh.extract(im)
    assert not _same(res[1][2][h - 4, 1:h - 1], fresh.scores[h - 4, 1:h - 1])
    assert _same(res[1][2][h - 4, h - 1:], fresh.scores[h - 4, h - 1:]) and _same(res[1][2][:h - 4], fresh.scores[:h - 4])


def check_near_threshold(case, res, v):
    s = res[0][2]
    h, w = s.shape
    below, above = int(((s >= 70) & (s < 80)).sum()), int(((s >= 80) & (s < 90)).sum())
    print(case["name"], "cells in [70, 80):", below, " in [80, 90):", above)
    assert below >= v[0] and above >= v[1] and case["nms"] == 0
    assert np.array_equal(res[0][0], _row_major(SC.written(w, h) & (s >= 80)))


def check_nan_cells(case, res, cells_per_call):
    """the NaN cells of every call, and each of them a keypoint: `< 80` is false for it, and no comparison with it is true"""
    for k, (r, cells) in enumerate(zip(res, cells_per_call)):
        rr, cc = np.nonzero(np.isnan(r[2]))
        assert sorted(zip(cc.tolist(), rr.tolist())) == sorted(cells), k
        for c in cells:
            assert (r[0] == np.array(c, F32)).all(1).any(), (k, c)
    assert any(cells_per_call)


def check_gradient_1020(case, res, v):
    top = max(max(int(np.abs(r[3].astype(int)).max()), int(np.abs(r[4].astype(int)).max())) for r in res)
    assert top == 1020


def check_tensor_below_2_24(case, res, v):
    top = 0
    for r in res:
        x, y = r[3].astype(np.int64), r[4].astype(np.int64)
        for a in (x * x, np.abs(x * y), y * y):
            box = sum(np.roll(np.roll(np.pad(a, 2), dy, 0), dx, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
            top = max(top, int(box.max()))
    print(case["name"], "largest 3 x 3 tensor sum:", top)
    assert 1020 * 1020 <= top < 2 ** 24


CHECKERS = {k[len("check_"):]: f for k, f in list(globals().items()) if k.startswith("check_")}


@pytest.mark.parametrize("name", SC.NAMES)
def test_claims(name):
    case = SC.BY_NAME[name]
    assert case["claims"]
    for key, v in case["claims"].items():
        CHECKERS[key](case, closed(name), v)                        # (a claim without a checker is a KeyError)


def test_table_holds_what_the_issue_lists():
    n = SC.NAMES
    for want in ("ties_checker2", "ties_checker2_nms0", "ties_checker2_nms15", "ties_checker4", "ties_checker8", "marks_unwritten", "marks_many",
                 "size_change", "threshold", "saturated", "nan_score_nms0", "nan_score_nms2"):
        assert want in n
    assert {"dense_rows_%dx%d" % (w, h) for w in (255, 256, 257, 258, 300) for h in (6, 8)} <= set(n)
    assert {"geometry_%dx%d_%s_nms%d" % (w, h, k, m) for w, h in ((5, 5), (6, 5), (300, 5), (41, 41), (42, 41), (7, 7)) for k in ("dense", "smooth")
            for m in (0, 2)} <= set(n)
    assert {c["nms"] for c in SC.CASES} >= {0, 2, 3, 5, 15}
    assert all(max(im.shape) <= 300 for c in SC.CASES for im, _, _ in c["calls"])


# ---- the oracle refuses what the C ABI refuses -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,held", SC.REFUSALS, ids=[r[0] for r in SC.REFUSALS])
def test_oracle_refuses_a_held_point_outside_the_image(tag, held):
    ex = SH.ShiTomasi(3)
    ex.extract(SC.REFUSAL_IMAGE, held[:1])
    before = (ex.scores.copy(), ex.Xg.copy(), ex.Yg.copy(), ex.next_id)
    other = SC.noise(SC.W, SC.H, 32)
    with pytest.raises(ValueError):
        ex.extract(other, held)
    assert _same(before[0], ex.scores) and np.array_equal(before[1], ex.Xg) and np.array_equal(before[2], ex.Yg) and before[3] == ex.next_id
    with pytest.raises(ValueError):                                # before a resize, too: the extractor keeps its size and buffers
        ex.extract(SC.noise(50, 30, 33), held)
    assert ex.shape == SC.REFUSAL_IMAGE.shape and _same(before[0], ex.scores)
    fresh = SH.ShiTomasi(3)
    with pytest.raises(ValueError):
        fresh.extract(other, held)
    assert fresh.shape is None and fresh.next_id == 0


def test_oracle_accepts_the_cells_next_to_the_refused_ones():
    """-0.49 and w - 1 + 0.49 are cells 0 and w - 1 (half away from zero): accepted, and marked where they round to"""
    ex = SH.ShiTomasi(3)
    w, h = SC.W, SC.H
    ex.extract(SC.REFUSAL_IMAGE, np.array([[-0.49, h - 1 + 0.49], [w - 1 + 0.49, -0.4]], F32))
    assert ex.scores[h - 1, 0] == -1 and ex.scores[0, w - 1] == -1 and (ex.scores == -1).sum() == 2
