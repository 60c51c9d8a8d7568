"""Pins tests/golden/poly_np.py, the restatement of COCO's polygon fill (rleFrPoly + merge) that tests/test_gpu_poly.py holds
the device to: integer-corner rectangles, a literal mask, the published sort / difference / merge ending against the parity
fill, an even-odd point-in-polygon test at pixel centres as a loose outside check, and the special cases and refusals."""
import numpy as np
import pytest

import poly_cases
import poly_np as pn
import segm_eval_np as sen

N_RANDOM = 320
H, W = 23, 31


@pytest.fixture(scope="module")
def random_polygons():
    rs = np.random.RandomState(20)
    return [poly_cases.random_polygon(rs, H, W) for _ in range(N_RANDOM)]


@pytest.mark.parametrize("x0,y0,x1,y1", [(2, 3, 7, 6), (0, 0, 9, 11), (0, 0, 1, 1), (8, 10, 9, 11), (0, 4, 9, 5), (3, 0, 4, 11)])
def test_integer_corner_rectangles(x0, y0, x1, y1):
    """(a) [x0,y0, x1,y0, x1,y1, x0,y1] fills exactly columns x0..x1-1, rows y0..y1-1: either winding, any starting vertex."""
    h, w = 11, 9
    want = np.zeros((h, w), np.uint8)
    want[y0:y1, x0:x1] = 1
    corners = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    for winding in (corners, corners[::-1]):
        for start in range(4):
            xy = [float(c) for p in winding[start:] + winding[:start] for c in p]
            assert np.array_equal(pn.polygon_mask(xy, h, w), want), (winding, start)


def test_literal_mask():
    """(b) [2,3, 7,3, 7,6, 2,6] on a 9 x 11 image."""
    want = np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0],
                     [0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0],
                     [0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]], np.uint8)
    got = pn.annotation_masks([[[2, 3, 7, 3, 7, 6, 2, 6]]], 9, 11)
    assert got.shape == (1, 9, 11) and np.array_equal(got[0], want)
    assert list(sen.encode_counts(got[0])) == [21, 3, 6, 3, 6, 3, 6, 3, 6, 3, 39]


def test_array_forms_equal_the_literal_loops(random_polygons):
    for xy in random_polygons:
        u, v = pn.dense_points(xy)
        ul, vl = pn.dense_points_loop(xy)
        assert u.tolist() == ul and v.tolist() == vl
        assert len(ul) == pn.n_points(xy)
        assert pn.crossings(u, v, H, W).tolist() == pn.crossings_loop(ul, vl, H, W)


def test_parity_fill_equals_published_ending(random_polygons):
    """(c) the parity fill against sort / differences / merge of zero-length runs."""
    outside = 0
    for xy in random_polygons:
        a = pn.crossings(*pn.dense_points(xy), H, W)
        counts = pn.published_counts(a, H, W)
        assert all(c > 0 for c in counts[1:-1]) or len(counts) <= 2
        assert np.array_equal(pn.fill(a, H, W).reshape(W, H).T, sen.decode_counts(counts, H, W))
        c = np.asarray(xy).reshape(-1, 2)
        outside += bool((c < 0).any() or (c[:, 0] > W).any() or (c[:, 1] > H).any())
    assert outside >= 50                                                # some reach outside the image


def _even_odd(xy, px, py):
    """Crossing-number test of the points (px, py) against the polygon's outline."""
    c = np.asarray(xy, np.float64).reshape(-1, 2)
    x0, y0 = c[:, 0][:, None], c[:, 1][:, None]
    x1, y1 = np.roll(c[:, 0], -1)[:, None], np.roll(c[:, 1], -1)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        xi = x0 + (py[None, :] - y0) * (x1 - x0) / (y1 - y0)
    cross = ((y0 > py[None, :]) != (y1 > py[None, :])) & (px[None, :] < xi)
    return (cross.sum(0) & 1).astype(np.uint8)


def _boundary_distance(xy, px, py):
    c = np.asarray(xy, np.float64).reshape(-1, 2)
    a, b = c[:, None, :], np.roll(c, -1, axis=0)[:, None, :]
    p = np.stack([px, py], 1)[None, :, :]
    ab = b - a
    den = (ab * ab).sum(-1)
    t = np.clip(((p - a) * ab).sum(-1) / np.where(den == 0, 1.0, den), 0.0, 1.0)
    return np.sqrt((((a + t[..., None] * ab) - p) ** 2).sum(-1)).min(0)


def test_loose_outside_check(random_polygons):
    """(d) every pixel where the fill disagrees with an even-odd test at the pixel centre (x + .5, y + .5) lies within 0.5 px
    of the outline.  A cap, not a tolerance.  Measured on these seeds: 0.1849 px over 1295 differing pixels (recorded in DESIGN.md 4.12)."""
    ys, xs = np.mgrid[0:H, 0:W]
    px, py = xs.ravel() + .5, ys.ravel() + .5
    worst, differing = 0.0, 0
    for xy in random_polygons:
        got = pn.polygon_mask(xy, H, W).ravel()
        bad = got != _even_odd(xy, px, py)
        if bad.any():
            differing += int(bad.sum())
            worst = max(worst, float(_boundary_distance(xy, px[bad], py[bad]).max()))
    print("farthest disagreeing pixel centre: %.4f px from the outline (%d pixels differ)" % (worst, differing))
    assert worst < 0.5


def test_polygon_wholly_outside_is_empty():
    h, w = 9, 11
    for dx, dy in ((-30, 0), (30, 0), (0, -30), (0, 30), (-30, -30), (30, 30)):
        xy = [2.5 + dx, 3 + dy, 7 + dx, 3.2 + dy, 6 + dx, 8 + dy]
        assert not pn.polygon_mask(xy, h, w).any(), (dx, dy)


def test_repeated_and_closing_vertices_change_nothing(random_polygons):
    for xy in random_polygons[:60]:
        want = pn.polygon_mask(xy, H, W)
        assert np.array_equal(pn.polygon_mask(list(xy) + list(xy[:2]), H, W), want)           # closed by its first vertex
        assert np.array_equal(pn.polygon_mask(list(xy[:4]) + list(xy[2:]), H, W), want)       # second vertex twice


def test_overlapping_polygons_give_their_union():
    h, w = 12, 14
    a, b = [1, 1, 8, 1, 8, 7, 1, 7], [5, 4, 12, 4, 12, 10, 5, 10]
    want = np.zeros((h, w), np.uint8)
    want[1:7, 1:8] = 1
    want[4:10, 5:12] = 1
    got = pn.annotation_masks([[a, b], [a], []], h, w)
    assert np.array_equal(got[0], want) and got[0, 4:7, 5:8].all()        # the overlap does not cancel
    assert np.array_equal(got[1], pn.polygon_mask(a, h, w)) and not got[2].any()


def test_refusals():
    tri = [0.0, 0.0, 4.0, 0.0, 4.0, 4.0]
    for bad in ([0, 0, 4, 0, 4, 4, 1], [0, 0, 4, 4], [], [0, 0, 4, 0, float("nan"), 4], [0, 0, 4, 0, float("inf"), 4],
                [0, 0, 4, 0, 2.0 ** 20 + 1, 4], [0, 0, 4, 0, 4, -2.0 ** 20 - 1]):
        with pytest.raises(ValueError):
            pn.annotation_masks([[tri], [bad]], 8, 8)
    pn.check([[[0, 0, 2.0 ** 20, 0, 4, -2.0 ** 20]]], 8, 8)              # the bounds themselves are accepted
    with pytest.raises(ValueError):
        pn.check([[tri]], 2048, 2049)                                    # h w > 2^22
    with pytest.raises(ValueError):
        pn.check([[tri]], 0, 8)
    big = 2.0 ** 20
    zigzag = [c for j in range(8) for c in ((-big if j % 2 else big), float(j))]     # 8 edges of 10 * 2^20 points each
    assert pn.n_points(zigzag) > pn.MAX_POINTS
    with pytest.raises(ValueError, match="dense points"):
        pn.check([[zigzag]], 8, 8)


def test_host_arrays_and_c_abi_refusals(random_polygons):
    """The host side of cim_amd.segm_eval.poly_masks (no device work): the edge-length prefix agrees with the restatement's
    dense points, and the library refuses what it cannot size."""
    from cim_amd import _lib, segm_eval
    anns = [random_polygons[0:2], [], random_polygons[2:5]]
    xy, poly_off, poly_ann, edge_off, total = segm_eval._polygon_arrays(anns, H, W)
    polys = random_polygons[0:5]
    assert poly_ann.tolist() == [0, 0, 2, 2, 2] and poly_off.tolist() == np.cumsum([0] + [len(p) // 2 for p in polys]).tolist()
    assert total == sum(pn.n_points(p) for p in polys) == edge_off[-1] == pn.check(anns, H, W)
    assert np.array_equal(xy, np.concatenate([np.asarray(p, np.float64) for p in polys]))
    assert [int(edge_off[o]) for o in poly_off[1:]] == np.cumsum([pn.n_points(p) for p in polys]).tolist()
    tri = [0.0, 0.0, 4.0, 0.0, 4.0, 4.0]
    for bad in ([0, 0, 4, 0, 4, 4, 1], [0, 0, 4, 4], [0, 0, 4, 0, float("nan"), 4], [0, 0, 4, 0, float("-inf"), 4],
                [0, 0, 4, 0, 2.0 ** 20 + 1, 4]):
        with pytest.raises(ValueError):
            segm_eval._polygon_arrays([[tri], [bad]], 8, 8)
    with pytest.raises(ValueError):
        segm_eval._polygon_arrays([[tri]], 2048, 2049)
    big = 2.0 ** 20
    zigzag = [c for j in range(8) for c in ((-big if j % 2 else big), float(j))]
    with pytest.raises(ValueError, match="CIM_POLY_MAX_POINTS"):
        segm_eval._polygon_arrays([[zigzag]], 8, 8)
    assert segm_eval.MAX_POLY_POINTS == pn.MAX_POINTS
    words = (H * W + 63) // 64
    assert _lib.call("cim_poly_ws_bytes", 5, H, W) >= 5 * words * 8
    assert _lib.call("cim_poly_ws_bytes", 0, H, W) > 0
    for args in ((-1, H, W), (1, 0, W), (1, 2048, 2049)):
        assert _lib.call("cim_poly_ws_bytes", *args) == -1
    assert "cim_poly_ws_bytes" in _lib.load().cim_last_error().decode()
    for n_poly, n_vert, n_points, h, w, msg in ((1, 3, pn.MAX_POINTS + 1, 8, 8, "dense points"), (1, 3, 10, 2048, 2049, "H \\* W"),
                                                (2, 5, 10, 8, 8, "vertices"), (1, 3, 2, 8, 8, "vertices")):
        with pytest.raises(_lib.CimHipError, match=msg):                 # refused before anything is launched or read
            _lib.call("cim_poly_fill", None, None, None, None, n_poly, n_vert, n_points, 1, h, w, None, None, None)
