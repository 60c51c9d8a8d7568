"""tests/golden/pil_resample_np.py - the arithmetic csrc/resample.hip repeats on the device - against Pillow
itself, bit for bit, and the header entries of the device path.  No GPU."""
import zlib

import numpy as np
import pytest
from PIL import Image

import pil_resample_np as prn


def pillow(img, out_w, out_h):
    return np.asarray(Image.fromarray(img).resize((out_w, out_h), Image.BILINEAR))


def check(hw, size):
    (h, w), (ow, oh) = hw, size
    for kind in prn.CONTENTS:
        img = prn.content(kind, h, w, zlib.crc32(repr((hw, size)).encode()) % (1 << 31))
        got = prn.resize(img, ow, oh)
        assert got.shape == (oh, ow, 3) and got.dtype == np.uint8
        np.testing.assert_array_equal(got, pillow(img, ow, oh), err_msg="%s -> %s, %s" % (hw, size, kind))


@pytest.mark.parametrize("hw,size", prn.CASES, ids=["%dx%d_to_%dx%d" % (c[0] + c[1]) for c in prn.CASES])
def test_restatement_equals_pillow_on_the_fixed_cases(hw, size):
    check(hw, size)


def test_restatement_equals_pillow_on_100_seeded_shapes():
    shapes = prn.seeded_shapes()
    assert len(shapes) == 100 and all(h <= 100 * w for (h, w), _ in shapes)
    assert sum(1 for _, s in shapes if s == (448, 448)) >= 20 and sum(1 for _, s in shapes if s != (448, 448)) >= 20
    for hw, size in shapes:
        check(hw, size)


def test_table_rows_hold_n_entries_then_zeros_and_sum_to_one():
    for n_in, n_out in prn.TABLE_CASES:
        bounds, kk = prn.coeffs(n_in, n_out)
        assert bounds.dtype == np.int32 and kk.dtype == np.int32 and kk.shape == (n_out, prn.ksize(n_in, n_out))
        assert np.all(bounds[:, 0] >= 0) and np.all(bounds[:, 1] >= 1) and np.all(bounds.sum(1) <= n_in)
        assert np.all(bounds[:, 1] <= kk.shape[1])
        tail = np.arange(kk.shape[1])[None, :] >= bounds[:, 1:2]
        assert not kk[tail].any()
        assert np.all(np.abs(kk.sum(1) - (1 << prn.PRECISION_BITS)) <= kk.shape[1])      # each entry rounds by at most 1/2


def test_an_unchanged_axis_has_the_identity_table():
    """scale 1: one tap of weight 2^22 on the sample itself - the device path runs such an axis through its table."""
    bounds, kk = prn.coeffs(448, 448)
    np.testing.assert_array_equal(bounds[:, 0], np.arange(448))
    assert np.all(kk[:, 0] == 1 << prn.PRECISION_BITS) and not kk[:, 1:].any()


def test_the_vertical_first_shapes_are_refused():
    prn.resize(np.zeros((300, 3, 3), dtype=np.uint8), 4, 4)
    with pytest.raises(ValueError, match="vertical pass first"):
        prn.resize(np.zeros((301, 3, 3), dtype=np.uint8), 4, 4)


def test_header_entries_parse_into_the_binding():
    import ctypes

    from cim_amd import _lib
    v, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert _lib.FUNCTIONS["cim_resample_ws_bytes"] == (ll, [i, v, i, i])
    assert _lib.SIGNATURES["cim_resample_tables"] == [v, v, i, i, i, v, v]
    assert _lib.SIGNATURES["cim_resample_rgb"] == [v, v, v, i, i, i, v, v, v, v, v]
    assert "cim_resample_ws_bytes" in _lib.VALUE_RETURNING
    assert _lib.CONSTANTS["CIM_RESAMPLE_MAX_SRC"] == 16384 and _lib.CONSTANTS["CIM_RESAMPLE_MAX_DST"] == 4096
    assert _lib.CONSTANTS["CIM_RESAMPLE_MAX_ASPECT"] == 100 and _lib.CONSTANTS["CIM_RESAMPLE_PRECISION_BITS"] == 22
    assert _lib.ABI_VERSION == 16                                                      # additive
