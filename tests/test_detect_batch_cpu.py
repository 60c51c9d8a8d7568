"""Batched detection post-processing (cim_amd.detect.nms_limit_batch, cim_amd/datasets/results.py, csrc/detect.hip's ragged
batch form): the C ABI and its refusals, the Python layer's refusals, and the NumPy restatement
(tests/golden/detect_batch_np.py) against every golden captured from the reference.  No GPU needed.  The filter and class-mask
cases built here are run on the device by tests/test_gpu_detect_batch.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import detect_batch_np
import detect_np
from test_detect_cpu import GOLDEN_CASES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cim_batch_detect_ws_bytes", "cim_batch_detect_nms_limit"}


def _row_off(ns):
    return np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)


def grid_boxes(n, pitch=20.0, side=9.0):
    """Disjoint boxes: NMS keeps every candidate."""
    k = np.arange(n)
    return np.stack([(k % 8) * pitch, (k // 8) * pitch, (k % 8) * pitch + side, (k // 8) * pitch + side], 1).astype(np.float32)


def filter_case():
    """A 200 x 250 image: lo = float32(0.00002 * 50000) = 1, hi = float32(0.85 * 50000) = 42500.  Proposal 0 has area exactly
    lo and proposal 2 exactly hi (both stay: the compares are strict); 1 is below lo and 3 above hi (both dropped).  3 contains
    2 (IoU 170 / 171 with the + 1 widths) and scores higher: WITHOUT the filter 3 suppresses 2, with it 2 is kept and 3 gone."""
    h, w = 200, 250
    boxes = np.array([[10, 10, 11, 11], [20, 20, 21, 20.5], [0, 0, 170, 250], [0, 0, 171, 250], [100, 100, 140, 130]], np.float32)
    scores = np.array([[0.5, 0.1], [0.6, 0.2], [0.7, 0.3], [0.8, 0.4], [0.9, 0.05]], np.float32)
    bounds = np.array(detect_batch_np.area_bounds(h, w), np.float32)
    return dict(scores=scores, boxes=boxes, bounds=bounds, height=h, width=w)


def class_mask_case():
    """Two classes on three disjoint boxes, limit 2: the two best of ALL classes are both of class 0, so class 1 - the only
    present one - has nothing left after the limit.  Masking BEFORE the limit would keep class 1's two best instead."""
    scores = np.array([[0.9, 0.6], [0.8, 0.5], [0.7, 0.4]], np.float32)
    return dict(scores=scores, boxes=grid_boxes(3), present=np.array([0, 1], np.uint8), max_det=2)


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_restatement_with_one_image_matches_reference_goldens(name):
    g = GOLDEN_CASES[name]
    thr, nms_thr, D = g["params"]
    image, idx, cls, sc, count = detect_batch_np.nms_limit_batch([g["scores"]], [g["boxes"]], thr, nms_thr, int(D))
    assert count.shape == (1, g["scores"].shape[1]) and np.array_equal(count[0], g["index_counts"])
    assert np.array_equal(idx, g["index_inds"]) and not image.any()
    dets = np.hstack((g["boxes"][idx], sc[:, None])).astype(np.float32)
    assert np.array_equal(dets.view(np.uint32), g["index_cls_boxes"].view(np.uint32))


def test_header_declares_and_lib_binds_batch_entries():
    from cim_amd import _lib, build, detect
    header = open(os.path.join(REPO, "include", "cim_hip.h")).read()
    declared = set(re.findall(r"\b(cim_batch_detect_[a-z0-9_]+)\s*\(", header))
    assert declared == NEW and declared <= set(_lib.SIGNATURES)
    m = re.search(r"#define CIM_BATCH_DETECT_MAX_IMAGES (\d+)", header)
    assert m and int(m.group(1)) == detect.MAX_IMAGES >= 1024
    build.build()
    lib = _lib.load()
    assert lib.cim_abi_version() == _lib.ABI_VERSION == 16
    for name in declared:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    assert lib.cim_batch_detect_ws_bytes.restype == ctypes.c_longlong


def _ws(row_off, C, B=None):
    from cim_amd import _lib
    ro = np.ascontiguousarray(row_off, dtype=np.int32)
    return _lib.call("cim_batch_detect_ws_bytes", ro.ctypes.data, len(ro) - 1 if B is None else B, C)


def test_workspace_size_and_refusals_before_any_launch():
    from cim_amd import _lib, build, detect
    build.build()
    err = lambda: _lib.load().cim_last_error().decode()
    small = _ws(_row_off([1]), 1)
    assert small > 0
    ns = [1, 64, 65, 130, 300]
    big = _ws(_row_off(ns), 3)
    words = [(n + 63) // 64 for n in ns]
    assert big >= sum(n * w * 8 for n, w in zip(ns, words)) + 3 * sum(words) * 8 + 6 * 3 * sum(ns) * 4
    assert _ws(_row_off([8] * detect.MAX_IMAGES), 2) > 0 and _ws(_row_off([8192]), 80) > 8192 * 128 * 8
    refused = {
        "no image": (_row_off([]), 20),
        "too many images": (_row_off([1] * (detect.MAX_IMAGES + 1)), 20),
        "an empty image": (_row_off([5, 0, 5]), 20),
        "too many proposals": (_row_off([10, 8193]), 20),
        "row_off not from 0": (_row_off([5, 5]) + 1, 20),
        "row_off decreasing": (np.array([0, 10, 4], np.int32), 20),
        "no class": (_row_off([5]), 0),
        "3 C sum N >= 2^31": (_row_off([8192] * 100), 1000),
    }
    for what, (ro, C) in refused.items():
        assert _ws(ro if len(ro) else np.zeros(1, np.int32), C, B=len(ro) - 1) == -1, what
        msg = err()
        assert "B <= %d" % detect.MAX_IMAGES in msg and "N_b <= 8192" in msg and "2^31" in msg and "row_off" in msg, (what, msg)
    # the launch entry refuses the same shapes, and ld < C, before it touches a pointer or the device
    ro = _row_off([4, 4])
    args = lambda ld, C: (None, ld, None, None, ro.ctypes.data, 2, C, 1e-5, 0.3, 100, None, None, None, None, None, None, None)
    with pytest.raises(_lib.CimHipError, match="leading dimension must be >= C"):
        _lib.call("cim_batch_detect_nms_limit", *args(2, 3))
    bad = _row_off([4, 9000])
    with pytest.raises(_lib.CimHipError, match="N_b <= 8192"):
        _lib.call("cim_batch_detect_nms_limit", None, 3, None, None, bad.ctypes.data, 2, 3, 1e-5, 0.3, 100, None, None, None,
                  None, None, None, None)
    with pytest.raises(_lib.CimHipError, match="bad argument"):          # in-range shapes, null pointers: still no launch
        _lib.call("cim_batch_detect_nms_limit", *args(3, 3))


def test_batch_and_drivers_reject_cpu_tensors():
    from cim_amd import _lib, detect
    from cim_amd.datasets import results
    s, b = torch.rand(10, 3), torch.rand(10, 4)
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        detect.nms_limit_batch([s], [b])
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        detect.nms_limit_batch((s, np.array([0, 10])), b)
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        detect.nms_limit_batch([s.numpy()], [b])
    roidb = [dict(image="a.jpg", id=1, height=4, width=5, gt_classes=np.ones((1, 3)))]
    all_boxes = {"a.jpg": dict(scores=s, boxes=b)}
    masks_of = lambda e: np.zeros((10, 4, 5), np.uint8)
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        results.instance_predictions(all_boxes, roidb, masks_of, 3)
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        results.pseudo_labels(all_boxes, roidb, masks_of, 3, [])


def test_batch_argument_checks():
    from cim_amd import detect
    s, b = np.zeros((10, 3), np.float32), np.zeros((10, 4), np.float32)
    with pytest.raises(TypeError, match="float32"):
        detect.nms_limit_batch([s.astype(np.float64)], [b])
    with pytest.raises(ValueError, match="disagree"):
        detect.nms_limit_batch([s, s], [b])


def test_chunks_follow_the_budget_and_the_library_limits():
    from cim_amd import detect
    ro = np.concatenate([[0], np.cumsum([300, 65, 130, 1, 300, 64, 200])])
    one = detect._image_bytes(300, 3)
    assert detect._chunks(ro, 3, 1 << 30) == [(0, 7)]
    assert detect._chunks(ro, 3, one + 4096) == [(0, 1), (1, 4), (4, 5), (5, 7)]
    assert detect._chunks(ro, 3, 2 * one + 4096) == [(0, 4), (4, 7)]
    with pytest.raises(ValueError, match="does not hold one image"):
        detect._chunks(ro, 3, one + 4095)
    many = np.arange(detect.MAX_IMAGES + 6) * 8
    assert detect._chunks(many, 2, 1 << 30) == [(0, detect.MAX_IMAGES), (detect.MAX_IMAGES, detect.MAX_IMAGES + 5)]
    big = np.arange(4) * 8192                                          # 3 * C * sum N < 2^31 splits too
    assert detect._chunks(big, 50000, 1 << 40) == [(0, 1), (1, 2), (2, 3)]


def _restated_batch(scores, boxes, score_thr=1e-5, nms_thr=0.3, max_det=100, num_classes=None, area_bounds=None,
                    class_mask=None, ws_budget_bytes=None):
    """The restatement behind nms_limit_batch's signature: the drivers' host logic runs here without a device."""
    return detect_batch_np.nms_limit_batch([np.asarray(s)[:, :num_classes] for s in scores], boxes, score_thr, nms_thr, max_det,
                                           area_bounds, class_mask)


def test_drivers_refuse_a_mis_sized_mask(monkeypatch):
    from cim_amd import detect
    from cim_amd.datasets import results
    monkeypatch.setattr(detect, "nms_limit_batch", _restated_batch)
    rng = np.random.RandomState(3)
    roidb = [dict(image="a.jpg", id=1, height=6, width=5, gt_classes=np.ones((1, 2)))]
    all_boxes = {"a.jpg": dict(scores=rng.rand(8, 2).astype(np.float32), boxes=grid_boxes(8))}
    for bad in ((8, 5, 6), (8, 6, 4), (8, 12, 10)):
        masks_of = lambda e, bad=bad: np.ones(bad, np.uint8)
        with pytest.raises(NotImplementedError, match="resizing masks is not supported"):
            results.instance_predictions(all_boxes, roidb, masks_of, 2)
        with pytest.raises(NotImplementedError, match="resizing masks is not supported"):
            results.pseudo_labels(all_boxes, roidb, masks_of, 2, [])


def test_filter_compares_are_strict_at_both_bounds():
    c = filter_case()
    lo, hi = c["bounds"]
    area = (c["boxes"][:, 2] - c["boxes"][:, 0]) * (c["boxes"][:, 3] - c["boxes"][:, 1])
    assert lo == np.float32(1) and hi == np.float32(42500) and area[0] == lo and area[2] == hi and area[1] < lo and area[3] > hi
    on = detect_batch_np.nms_limit_image(c["scores"], c["boxes"], 1e-5, 0.3, 100, bounds=c["bounds"])
    off = detect_batch_np.nms_limit_image(c["scores"], c["boxes"], 1e-5, 0.3, 100)
    assert list(on[0]) == [0, 2, 4, 0, 2, 4] and list(on[1]) == [0, 0, 0, 1, 1, 1]      # both equal-to-bound proposals stay
    assert list(off[0]) == [0, 1, 3, 4, 0, 1, 3, 4]                                      # unfiltered: 3 suppresses 2
    assert np.array_equal(on[2].view(np.uint32), c["scores"][on[0], on[1]].view(np.uint32))   # survivors keep their input score


def test_class_mask_after_the_limit_differs_from_before():
    c = class_mask_case()
    after = detect_batch_np.nms_limit_image(c["scores"], c["boxes"], 1e-5, 0.3, c["max_det"], class_mask=c["present"])
    before = detect_batch_np.nms_limit_image(c["scores"], c["boxes"], 1e-5, 0.3, c["max_det"], class_mask=c["present"],
                                             mask_first=True)
    assert len(after[0]) == 0 and list(after[3]) == [0, 0]
    assert list(before[0]) == [0, 1] and list(before[1]) == [1, 1]
    assert np.array_equal(detect_np.nms_limit(c["scores"], c["boxes"], 1e-5, 0.3, c["max_det"])[3], [2, 0])


def test_restated_builders_on_hand_made_masks(monkeypatch):
    """run_lengths / bbox_of against hand-derived values, and the product's host arithmetic on run counts
    (results.rle_area_bbox) against them: pixel (0, 0) set, a run across a column boundary, empty, full."""
    from cim_amd.datasets import results
    from cim_amd.utils import rle
    m = np.zeros((3, 4), np.uint8)
    m[0, 0] = 1
    m[2, 1] = m[0, 2] = m[1, 2] = 1                                      # column 1's last pixel runs into column 2
    assert detect_batch_np.run_lengths(m) == [0, 1, 4, 3, 4]
    assert detect_batch_np.bbox_of(m) == [0, 0, 3, 3]
    assert results.rle_area_bbox([0, 1, 4, 3, 4], 3) == (4, [0, 0, 3, 3])
    assert detect_batch_np.run_lengths(np.zeros((3, 4))) == [12] and results.rle_area_bbox([12], 3) == (0, [0, 0, 0, 0])
    assert detect_batch_np.run_lengths(np.ones((3, 4))) == [0, 12] and results.rle_area_bbox([0, 12], 3) == (12, [0, 0, 4, 3])
    rng = np.random.RandomState(5)
    for h, w in ((7, 9), (16, 5), (33, 64), (65, 3)):
        for _ in range(5):
            m = (rng.rand(h, w) < rng.choice([0.05, 0.5, 0.9])).astype(np.uint8)
            if not m.any():
                continue
            runs = detect_batch_np.run_lengths(m)
            assert np.array_equal(rle.counts_to_mask(runs, h, w), m)
            assert results.rle_area_bbox(runs, h) == (int(m.sum()), detect_batch_np.bbox_of(m))
