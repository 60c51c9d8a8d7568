"""-m gpu: the ragged batch form of the detection post-processing (cim_amd.detect.nms_limit_batch, csrc/detect.hip) and the
two dataset-level drivers on it (cim_amd/datasets/results.py) - bit for bit against cim_amd.detect.nms_limit image by image
and against the NumPy restatement (tests/golden/detect_batch_np.py).  DESIGN.md 4.15."""
import numpy as np
import pytest
import torch

import detect_batch_np
from test_detect_batch_cpu import class_mask_case, filter_case, grid_boxes
from test_detect_cpu import GOLDEN_CASES
from test_gpu_detect import _sweep_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(got, ref):
    for g, r, what in zip(got, ref, ("image", "idx", "cls", "score", "count")):
        if what == "score":
            g, r = _bits(g), _bits(r)
        assert g.shape == r.shape and np.array_equal(g, r), what


def _per_image(scores, boxes, thr, nms, D):
    """The single-image device path, image by image, in the batched call's output form."""
    from cim_amd import detect
    out = [detect.to_host(detect.nms_limit(torch.from_numpy(s).to(DEV), torch.from_numpy(b).to(DEV), thr, nms, D))
           for s, b in zip(scores, boxes)]
    return (np.concatenate([np.full(len(o[0]), k, np.int64) for k, o in enumerate(out)]), np.concatenate([o[0] for o in out]),
            np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out]), np.stack([o[3] for o in out]))


def _check(scores, boxes, thr=1e-5, nms=0.3, D=100, **kw):
    from cim_amd import detect
    got = detect.nms_limit_batch(scores, boxes, thr, nms, D, **kw)
    _assert_same(got, detect_batch_np.nms_limit_batch(scores, boxes, thr, nms, D))
    _assert_same(got, _per_image(scores, boxes, thr, nms, D))
    return got


def _images(ns, c, seed, kind="plain"):
    pairs = [_sweep_inputs(n, c, seed + 17 * k, kind) for k, n in enumerate(ns)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


@pytest.mark.parametrize("name", ["limit_exact", "limit_plus1", "limit_tie", "empty", "degenerate", "nolimit", "detect_n1000_c20"])
def test_one_image_matches_goldens(name):
    g = GOLDEN_CASES[name]
    thr, nms, D = g["params"]
    image, idx, cls, sc, count = _check([g["scores"]], [g["boxes"]], thr, nms, int(D))
    assert np.array_equal(idx, g["index_inds"]) and np.array_equal(count[0], g["index_counts"])
    assert np.array_equal(_bits(np.hstack((g["boxes"][idx], sc[:, None]))), _bits(g["index_cls_boxes"]))


def test_ragged_images_and_their_permutation():
    """A one-proposal image, the 64-lane word boundary on both sides, a different W per image; then the same images in
    another order (every tile offset changes)."""
    scores, boxes = _images([1, 64, 65, 130, 300], 3, 1)
    a = _check(scores, boxes)
    assert a[4].sum() > 0
    perm = [3, 0, 4, 2, 1]
    b = _check([scores[k] for k in perm], [boxes[k] for k in perm])
    for new, old in enumerate(perm):
        assert np.array_equal(b[1][b[0] == new], a[1][a[0] == old]) and np.array_equal(b[4][new], a[4][old])
    # the (concatenated, row_off) form, device tensors
    from cim_amd import detect
    row_off = np.concatenate([[0], np.cumsum([len(s) for s in scores])])
    c = detect.nms_limit_batch((torch.from_numpy(np.concatenate(scores)).to(DEV), row_off), torch.from_numpy(np.concatenate(boxes)).to(DEV))
    _assert_same(c, a)


def test_second_mask_register_between_small_images():
    scores, boxes = _images([40, 4160, 7], 1, 2)
    got = _check(scores, boxes)
    assert got[1][got[0] == 1].max() >= 4096                           # a kept proposal in the second register's range


def test_many_small_images():
    scores, boxes = _images([8] * 300, 2, 3)
    got = _check(scores, boxes, D=5)
    assert got[4].shape == (300, 2) and got[4].sum(1).max() >= 5


@pytest.mark.parametrize("D", [60, 0])
def test_mixed_cases_in_one_batch(D):
    """Nothing above the threshold in the middle, ties at the limit (the golden's 60th score twice), duplicate boxes with
    equal scores (the tie rule); max_det = 0 switches the limit off for all."""
    tie = GOLDEN_CASES["limit_tie"]
    plain = _sweep_inputs(65, 3, 5, "plain")
    none = _sweep_inputs(30, 3, 6, "none")
    ties = _sweep_inputs(130, 3, 7, "ties")
    scores = [plain[0], none[0], tie["scores"], ties[0]]
    boxes = [plain[1], none[1], tie["boxes"], ties[1]]
    got = _check(scores, boxes, D=D)
    assert got[4][1].sum() == 0
    if D == 60:
        assert got[4][2].sum() == int(tie["index_counts"].sum()) == 61  # ties at the threshold all stay
    else:
        assert got[4][2].sum() == 120


def test_chunks_and_a_side_stream_give_the_same_records(monkeypatch):
    from cim_amd import _lib, detect
    scores, boxes = _images([300, 65, 130, 1, 300, 64, 200], 3, 4)
    one = _check(scores, boxes)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    budget = detect._image_bytes(300, 3) + 4096                        # a 300-proposal image fills a chunk: 4 chunks
    _assert_same(detect.nms_limit_batch(scores, boxes, ws_budget_bytes=budget), one)
    assert calls.count("cim_batch_detect_nms_limit") >= 3
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        _assert_same(detect.nms_limit_batch(scores, boxes, ws_budget_bytes=budget), one)
        _assert_same(detect.nms_limit_batch(scores, boxes), one)
    with pytest.raises(ValueError, match="does not hold one image"):
        detect.nms_limit_batch(scores, boxes, ws_budget_bytes=1000)
    torch.cuda.synchronize()


def test_filter_and_class_mask_on_the_device():
    from cim_amd import detect
    f = filter_case()
    other = _sweep_inputs(65, 2, 8, "plain")
    scores, boxes = [other[0], f["scores"]], [other[1], f["boxes"]]
    bounds = np.stack([np.array([50.0, 3000.0], np.float32), f["bounds"]])
    on = detect.nms_limit_batch(scores, boxes, area_bounds=bounds)
    _assert_same(on, detect_batch_np.nms_limit_batch(scores, boxes, 1e-5, 0.3, 100, area_bounds=bounds))
    off = _check(scores, boxes)
    assert list(on[1][on[0] == 1]) == [0, 2, 4, 0, 2, 4] and list(off[1][off[0] == 1]) == [0, 1, 3, 4, 0, 1, 3, 4]
    assert not np.array_equal(on[1][on[0] == 0], off[1][off[0] == 0])   # the other image is filtered by ITS bounds
    _assert_same(detect.nms_limit_batch(scores, boxes, area_bounds=torch.from_numpy(bounds).to(DEV)), on)
    with pytest.raises(_lib_error(), match="score_thr >= 0"):
        detect.nms_limit_batch(scores, boxes, score_thr=-1.0, area_bounds=bounds)

    m = class_mask_case()
    other = _sweep_inputs(64, 2, 9, "plain")
    scores, boxes = [m["scores"], other[0]], [m["boxes"], other[1]]
    for present in (np.stack([m["present"], [1, 1]]), np.stack([m["present"], [1, 0]])):
        present = present.astype(np.uint8)
        got = detect.nms_limit_batch(scores, boxes, max_det=m["max_det"], class_mask=present)
        _assert_same(got, detect_batch_np.nms_limit_batch(scores, boxes, 1e-5, 0.3, m["max_det"], class_mask=present))
        assert got[4][0].sum() == 0                                     # (masking before the limit would give 2 here)
    assert got[4][1, 1] == 0


def _lib_error():
    from cim_amd import _lib
    return _lib.CimHipError


# ---------------------------------------------------------------- drivers
SIZES = ((7, 9), (16, 5), (33, 64), (65, 3))                           # (height, width)
NPROP, NCLS = 12, 3


@pytest.fixture(scope="module")
def dataset():
    rng = np.random.RandomState(20261018)
    roidb, all_boxes, masks = [], {}, {}
    for k, (h, w) in enumerate(SIZES):
        name = "/data/JPEGImages/2008_%06d.jpg" % (k + 1)
        m = (rng.rand(NPROP, h, w) < 0.4).astype(np.uint8)
        m[0] = 0
        m[0, 0, 0] = 1                                                   # pixel (0, 0) set: a leading 0 count
        m[1] = 0                                                         # empty: consumes an id, is not written
        m[2] = 1                                                         # full
        m[3] = 0
        m[3, h - 1, 0] = m[3, 0, 1] = 1                                  # one run across a column boundary
        sc = (rng.rand(NPROP, NCLS) * 0.9 + 0.05).astype(np.float32)
        sc[4, 1] = sc[5, 1] = sc[2, 1]                                   # equal scores within a class
        sc[:, 0] = np.round(sc[:, 0] * 4) / 4                            # many ties, also for the best of class 0
        gt = np.array([[1, k % 2, 1 - k % 2]], np.float32)
        roidb.append(dict(image=name, id=100 + k, height=h, width=w, gt_classes=gt))
        all_boxes[name] = dict(scores=sc, boxes=grid_boxes(NPROP))
        masks[name] = m
    return roidb, all_boxes, masks


@pytest.mark.parametrize("masks_on_device", [False, True])
@pytest.mark.parametrize("max_det", [100, 20])
def test_drivers_match_the_restatement(dataset, masks_on_device, max_det):
    from cim_amd.datasets import results
    roidb, all_boxes, masks = dataset
    host = lambda e: masks[e["image"]]
    masks_of = (lambda e: torch.from_numpy(masks[e["image"]]).to(DEV)) if masks_on_device else host
    cats = [{"id": i + 1, "name": "c%d" % i} for i in range(NCLS)]
    ids = [11, 22, 33]

    for filt, cat_ids in ((False, None), (True, ids)):
        got = results.instance_predictions(all_boxes, roidb, masks_of, NCLS, category_ids=cat_ids, proposal_filter=filt,
                                           max_det=max_det, images_per_call=3)
        ref = detect_batch_np.instance_predictions(all_boxes, roidb, host, NCLS, 1e-5, 0.3, category_ids=cat_ids,
                                                   proposal_filter=filt, max_det=max_det)
        assert got == ref and len(got) > 0
        assert all(type(p["score"]) is float and type(p["segmentation"]["counts"]) is str for p in got)
    for is_best in (False, True):
        got = results.pseudo_labels(all_boxes, roidb, masks_of, NCLS, cats, is_best=is_best, max_det=max_det, images_per_call=3)
        ref = detect_batch_np.pseudo_labels(all_boxes, roidb, host, NCLS, 1e-5, 0.3, cats, is_best=is_best, max_det=max_det)
        assert got == ref
        anns = got["annotations"]
        assert len(got["images"]) == len(SIZES) and len(anns) > 0
        assert [a["id"] for a in anns] == sorted(a["id"] for a in anns)
        if not is_best and max_det == 100:                               # every (proposal, present class) is written
            assert anns[-1]["id"] > len(anns)                            # the empty masks took ids
            assert any(a["segmentation"]["counts"][0] == 0 for a in anns)
        assert all(type(a["area"]) is int and all(type(v) is int for v in a["bbox"] + a["segmentation"]["counts"]) for a in anns)


def test_instance_predictions_feed_the_mask_evaluator(dataset):
    from cim_amd.datasets import json_inference, results
    roidb, all_boxes, masks = dataset
    preds = results.instance_predictions(all_boxes, roidb, lambda e: masks[e["image"]], NCLS)
    gt = {"images": [{"id": e["id"], "height": e["height"], "width": e["width"]} for e in roidb],
          "categories": [{"id": i + 1, "name": "c%d" % i} for i in range(NCLS)], "annotations": []}
    for e in roidb:
        for p in (2, 3, 6):
            m = masks[e["image"]][p]
            gt["annotations"].append({"id": len(gt["annotations"]) + 1, "image_id": e["id"], "category_id": 1 + p % NCLS, "iscrowd": 0,
                                      "area": int(m.sum()), "segmentation": {"size": list(m.shape), "counts": detect_batch_np.run_lengths(m)}})
    mAP, cls_ap, names = json_inference.coco_inst_seg_eval(gt, preds)
    assert names == ["c0", "c1", "c2"] and set(mAP) == {"0.25", "0.50", "0.70", "0.75"}
    assert all(0.0 <= v <= 1.0 for v in mAP.values()) and mAP["0.25"] > 0
