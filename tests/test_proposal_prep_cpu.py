"""Training inputs from proposal masks (cim_amd.proposal_prep, csrc/proposal_prep.hip): the C ABI and its
refusals, the host helpers, and the NumPy restatement (tests/golden/proposal_prep_np.py) against every golden captured from
the reference (make_golden_proposal_prep.py), against Pillow's nearest resize, and against the integer form of the
coverage threshold the kernels use.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

import proposal_prep_np as ppn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
FILES = ("voc", "coco", "nopoints")


def load_golden(name):
    d = np.load(os.path.join(GOLDEN, "proposal_prep_%s.npz" % name))
    g = {k: d[k] for k in d.files}
    g["masks_full"] = ppn.unpack_bits(g["mask_bits"], g["mask_shape"])
    return g


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_prop_entries():
    from cim_amd import _lib, build, proposal_prep
    header = open(os.path.join(REPO, "include", "cim_hip.h")).read()
    declared = set(re.findall(r"\b(cim_prop_[a-z0-9_]+)\s*\(", header))
    assert declared == {"cim_prop_ws_bytes", "cim_prop_prepare", "cim_prop_assign"}
    assert declared <= set(_lib.SIGNATURES)
    assert "#define CIM_PROP_MAX_POINTS 256" in header and "#define CIM_PROP_MAX_S 16" in header
    assert proposal_prep.MAX_POINTS == 256 and proposal_prep.MAX_S == 16
    assert "#define CIM_SEGM_MAX_HW (1 << 22)" in header and proposal_prep.MAX_HW == 1 << 22
    build.build()
    lib = _lib.load()
    assert lib.cim_abi_version() == _lib.ABI_VERSION == 16              # additive: the header's rule for new entry points
    for name in declared:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]


def test_workspace_query_and_refusals_of_the_c_entries():
    """Item 6 of the contract at the C level: -1 before any launch (no device is touched: this runs without one)."""
    import ctypes
    from cim_amd import _lib, build
    build.build()
    lib = _lib.load()
    n, h, w = 1000, 375, 500
    words = (h * w + 63) // 64
    assert _lib.call("cim_prop_ws_bytes", n, h * w, 0) >= 5 * n * 4
    assert _lib.call("cim_prop_ws_bytes", n, h * w, 6) >= words * 6 * 8 + 6 * 4 + n * 6 * 4
    for bad in ((0, h * w, 0), (n, 0, 0), (n, (1 << 22) + 1, 0), (n, h * w, -1), (n, h * w, 257)):
        assert _lib.call("cim_prop_ws_bytes", *bad) == -1
    p = ctypes.c_void_p(64)                                             # never dereferenced: every call below is refused first
    prep = lambda N, H, W, S: lib.cim_prop_prepare(p, N, H, W, S, p, p, p, p, p, p, None)
    for args in ((0, h, w, 7), (n, 0, w, 7), (n, h, 0, 7), (n, 65536, 1, 7), (n, 1, 65536, 7), (n, 2049, 2048, 7), (n, h, w, 0),
                 (n, h, w, 17)):
        assert prep(*args) == -1, args
        assert b"cim_prop_prepare: bad argument" in lib.cim_last_error()
    arr = lambda *v: (ctypes.c_int32 * len(v))(*v)

    def assign(rows, cols, classes, C=20, P=None, N=n, H=h, W=w):
        r, c, k = arr(*rows), arr(*cols), arr(*classes)
        return lib.cim_prop_assign(p, p, N, H, W, ctypes.cast(r, ctypes.c_void_p), ctypes.cast(c, ctypes.c_void_p),
                                   ctypes.cast(k, ctypes.c_void_p), len(rows) if P is None else P, C, p, p, None)
    for kw in (dict(rows=[h], cols=[0], classes=[0]), dict(rows=[-1], cols=[0], classes=[0]), dict(rows=[0], cols=[w], classes=[0]),
               dict(rows=[0], cols=[-1], classes=[0]), dict(rows=[0], cols=[0], classes=[20]), dict(rows=[0], cols=[0], classes=[-1]),
               dict(rows=[0, 1], cols=[0, 1], classes=[0, 80], C=80), dict(rows=[0], cols=[0], classes=[0], P=257),
               dict(rows=[0], cols=[0], classes=[0], N=0), dict(rows=[0], cols=[0], classes=[0], H=65536, W=1)):
        assert assign(**kw) == -1, kw
        assert b"cim_prop_assign: bad argument" in lib.cim_last_error()


def test_python_refusals_decided_on_the_host():
    from cim_amd import _lib, proposal_prep as pp
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        pp.prepare(torch.ones(3, 8, 8, dtype=torch.bool))
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        pp.prepare(np.ones((3, 8, 8), dtype=bool))
    with pytest.raises(TypeError):
        pp.assign_clusters(object(), [0], [0], [0], 20)
    # the checks on the points come before any launch, so a Prepared that holds no device data reaches them
    fake = pp.Prepared(None, None, None, torch.empty((2, 5), dtype=torch.int64), 10, 12)
    for rows, cols, classes, c, msg in (([10], [0], [0], 20, "outside the 10 x 12 image"), ([0], [12], [0], 20, "outside the 10 x 12 image"),
                                        ([-1], [0], [0], 20, "outside"), ([0], [-1], [0], 20, "outside"),
                                        ([0], [0], [20], 20, "class 20"), ([0], [0], [-1], 20, "class -1"),
                                        ([0] * 257, [0] * 257, [0] * 257, 20, "at most 256"), ([0, 1], [0], [0], 20, "differ in length"),
                                        ([0.5], [0], [0], 20, "integers"), ([0], [0], [0], 0, "num_classes")):
        with pytest.raises(ValueError, match=msg):
            pp.assign_clusters(fake, rows, cols, classes, c)
    for n, h, w in ((0, 4, 4), (3, 65536, 1), (3, 1, 65536), (3, 2049, 2048)):
        with pytest.raises(ValueError):
            pp._check_shape(n, h, w)
    pp._check_shape(1, 2048, 2048)


# ---- host helpers ------------------------------------------------------------------------------------------------------------
def test_peaks_and_points_follow_the_reference_coordinate_conventions():
    from cim_amd import proposal_prep as pp
    # AGPL_label_assign.py:156-161: x = int(peak[2] * shape[1] / 112) indexes ROWS (shape[1] = H), y = int(peak[3] * shape[2] / 112)
    peaks = np.array([[0, 5, 111, 0], [0, 19, 56, 57], [0, 0, 1, 111]], dtype=np.int64)
    rows, cols, classes = pp.peaks_to_pixels(peaks, 375, 500)
    assert rows == [int(111 * 375 / 112), int(56 * 375 / 112), int(1 * 375 / 112)] == [371, 187, 3]
    assert cols == [0, int(57 * 500 / 112), int(111 * 500 / 112)] == [0, 254, 495]
    assert classes == [5, 19, 0]
    assert max(rows) < 375 and max(cols) < 500
    assert pp.peaks_to_pixels(np.zeros((0, 4)), 375, 500) == ([], [], [])
    # point_level_label_assign.py:56, 72-73: (x, y, class, conf), x = int(points[j][0]) indexes COLUMNS
    rows, cols, classes = pp.points_to_pixels([[25.5, 65.2, 3, 0.9], [12.0, 70.9, 7, 0.8]])
    assert (rows, cols, classes) == ([65, 70], [25, 12], [3, 7])
    assert pp.points_to_pixels([]) == ([], [], [])


# ---- the restatement against the reference's own output ----------------------------------------------------------------------
@pytest.mark.parametrize("name", FILES)
def test_restatement_equals_the_reference_goldens(name):
    from cim_amd import proposal_prep as pp
    g = load_golden(name)
    boxes, small, area = ppn.boxes_and_small(g["masks_full"], 7)
    assert g["boxes"].dtype == np.uint16 and g["small"].dtype == bool and g["mat"].dtype == np.float32
    np.testing.assert_array_equal(boxes, g["boxes"].astype(np.int32))
    np.testing.assert_array_equal(small, g["small"])
    np.testing.assert_array_equal(area, g["masks_full"].reshape(len(area), -1).sum(1))
    rows, cols, classes = pp.points_to_pixels(g["points"])
    mat = ppn.assign_clusters(g["masks_full"], rows, cols, classes, 20)
    assert mat.dtype == np.float32
    np.testing.assert_array_equal(mat, g["mat"])


def test_goldens_hold_the_cases_the_contract_names():
    voc, coco, nop = (load_golden(n) for n in FILES)
    wh = lambda g: (set((g["boxes"][:, 2].astype(int) - g["boxes"][:, 0]).tolist()), set((g["boxes"][:, 3].astype(int) - g["boxes"][:, 1]).tolist()))
    vw, vh = wh(voc)
    assert {2, 4, 8, 16, 32, 64, 128, 1, 3, 5, 7, 13} <= vw and {1, 2, 4, 8, 16, 32, 3, 5, 7} <= vh
    cw, ch = wh(coco)
    assert {256, 512, 1024, 1400, 1, 7} <= cw and {1, 2, 4, 8, 16, 32, 40} <= ch
    hh, ww = (int(v) for v in voc["mask_shape"][1:])
    assert (hh * ww) % 64 != 0 and (hh * ww) % 4 != 0
    assert len(voc["points"]) == 4 and len(nop["points"]) == 0
    assert np.all(nop["mat"][:, 0] == 1) and np.all(nop["mat"][:, 1:] == 0)                  # P = 0
    assert set(np.unique(voc["mat"]).tolist()) == {0.0, 2.0, 4.0, 5.0}                       # cluster 1 overwritten, 3 assigns nothing
    # the closed form of cim_amd.synthetic.masks_7x7 is NOT the reference's arithmetic: it fails these goldens
    from cim_amd import synthetic
    closed = synthetic.masks_7x7(voc["masks_full"], voc["boxes"].astype(np.int64)).astype(bool)
    assert np.any(closed != voc["small"])


# ---- item 2: the fp64 walk is Pillow's nearest resize ------------------------------------------------------------------------
def test_nearest_walk_equals_pillow_for_every_length():
    Image = pytest.importorskip("PIL.Image")
    lengths = list(range(1, 4097)) + sorted(np.random.RandomState(7).randint(4097, 65536, size=300).tolist()) + [65535]
    wrong_closed = 0
    for size in (1, 3, 7, 16):
        for e in lengths:
            src = np.arange(e, dtype=np.int32).reshape(1, e)                                # index-valued one-row image
            got = np.asarray(Image.fromarray(src).resize((size, 1), 0)).reshape(-1)
            want = ppn.nearest_index(e, size)
            assert np.array_equal(got, want), (size, e, got, want)
            if size == 7 and e < 1400:
                closed = np.minimum(((np.arange(size) + 0.5) * e / size).astype(np.int64), e - 1)
                wrong_closed += int(not np.array_equal(closed, want))
    assert wrong_closed == 26                                                               # 2, 4, 8, 16, 32, ...
    # and along the other axis (rows), as the reference's 2-D resize walks it
    for e in (1, 2, 4, 8, 16, 32, 64, 100, 375, 4096):
        src = np.arange(e, dtype=np.int32).reshape(e, 1)
        got = np.asarray(Image.fromarray(src).resize((1, 7), 0)).reshape(-1)
        assert np.array_equal(got, ppn.nearest_index(e, 7))


# ---- item 3: the integer form of mean(0) > 0.7 -------------------------------------------------------------------------------
def test_integer_and_fp64_coverage_thresholds_agree():
    for n in range(1, 2041):
        cnt = np.arange(0, n + 1, dtype=np.int64)
        assert np.array_equal(ppn.covered(cnt, n), ppn.covered_int(cnt, n)), n
    assert not ppn.covered(np.int64(7), 10) and ppn.covered(np.int64(8), 10)
    assert not np.any(ppn.covered(np.zeros(4, dtype=np.int64), 0))                           # NaN > 0.7


def test_restatement_sequential_rule_on_a_hand_case():
    """Item 5 on masks small enough to follow by hand: 1 x 8 image."""
    m = np.array([[1, 1, 1, 1, 0, 0, 0, 0],        # 0: covers the point at col 0
                  [1, 1, 1, 0, 0, 0, 0, 0],        # 1: covers it too -> avg = cols 0..2 (cnt 2 of 2), col 3 has 1/2: out
                  [0, 0, 1, 1, 1, 1, 0, 0],        # 2: IoU with avg = 1 / 6: background
                  [0, 0, 0, 0, 0, 0, 1, 1]],       # 3: IoU 0: untouched
                 dtype=bool).reshape(4, 1, 8)
    mat = ppn.assign_clusters(m, [0], [0], [2], 3)
    want = np.zeros((4, 4), np.float32)
    want[0, 3] = want[1, 3] = 1                    # IoU 3/4 and 1
    want[2, 0] = 2
    np.testing.assert_array_equal(mat, want)
    mat = ppn.assign_clusters(m, [0, 0, 0], [0, 7, 1], [2, 1, 0], 3)       # the third point selects the same two: last wins
    want = np.zeros((4, 4), np.float32)
    want[0, 1] = want[1, 1] = 3
    want[3, 2] = 2                                 # the second point: avg = cols 6..7 = mask 3
    want[2, 0] = 4
    np.testing.assert_array_equal(mat, want)
