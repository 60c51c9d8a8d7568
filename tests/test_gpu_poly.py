"""-m gpu: COCO's polygon fill on the device (csrc/poly_fill.hip, cim_amd.segm_eval.poly_masks) bit for bit against the
restatement tests/golden/poly_np.py: masks at the word-boundary sizes and on one 480 x 640 image of 40 annotations, run
counts, polygon ground truth through SegmEvaluator.add_image and the JSON evaluator, two threads on two streams, and a
workspace full of garbage."""
import json
import threading

import numpy as np
import pytest
import torch

import poly_cases
import poly_np as pn
import segm_eval_np as sen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def unpack(packed, h, w):
    """device int64 [n, words] -> host uint8 [n, h, w]; the bits past h w must be zero."""
    words = packed.cpu().numpy().view(np.uint64)
    bits = np.unpackbits(words.view(np.uint8).reshape(len(words), -1), axis=1, bitorder="little")
    assert not bits[:, h * w:].any(), "bits past h * w are set"
    return bits[:, :h * w].reshape(len(words), w, h).transpose(0, 2, 1).copy()


def _small_scene(h, w, seed):
    """Random polygons plus the ones a tiny image needs to show anything: the whole image and beyond, one pixel, a triangle
    over the bottom-right corner, an annotation without polygons."""
    rs = np.random.RandomState(seed)
    anns = poly_cases.random_scene(rs, h, w, 5, max_polys=3, kmin=3, kmax=12)
    anns.append([[-1.0, -1.0, w + 1.0, -1.0, w + 1.0, h + 1.0, -1.0, h + 1.0]])
    anns.append([[0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0]])
    anns.append([[w - 0.5, h + 2.0, w + 2.0, h - 0.5, w - 3.0, h - 3.0]])
    anns.append([])
    return anns


@pytest.mark.parametrize("h,w", [(1, 1), (1, 70), (70, 1), (9, 11), (37, 53), (64, 64)])
def test_small_images_bit_identical(h, w):
    from cim_amd import segm_eval
    anns = _small_scene(h, w, 100 * h + w)
    want = pn.annotation_masks(anns, h, w)
    assert want[5].all() and want[6].sum() == 1 and not want[8].any()
    got = unpack(segm_eval.poly_masks(anns, h, w, DEV), h, w)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def _crafted(h, w):
    """The cases the 480 x 640 image must hold whatever the seeds draw."""
    return [
        [[10.5, 20.5, 200.5, 30.0, 180.0, 150.5, 15.5, 140.0]],                           # half-integer coordinates
        [[-40.0, -25.5, 120.0, -10.0, 90.0, 80.0, -60.5, 60.0]],                          # negative coordinates
        [[w - 50.0, h - 80.0, w + 30.0, h - 60.0, w + 45.5, h + 40.0, w - 70.0, h + 25.0]],   # past the right and bottom borders
        [[300.0, 100.0, 300.0, 100.0, 400.0, 100.0, 400.0, 100.0, 400.0, 220.0, 300.0, 220.0, 300.0, 100.0]],   # zero-length edges
        [[100.0, 300.0, 160.0, 360.0, 163.0, 460.0, 330.0, 463.0, 230.0, 363.0, 101.0, 301.0]],   # diagonal, steep, shallow
        [[500.0, 50.0, 600.0, 50.0, 600.0, 150.0, 500.0, 150.0], [550.0, 100.0, 639.0, 100.0, 639.0, 200.0, 550.0, 200.0]],  # overlap
    ]


@pytest.fixture(scope="module")
def big():
    h, w = 480, 640
    rs = np.random.RandomState(11)
    anns = _crafted(h, w) + poly_cases.random_scene(rs, h, w, 34, max_polys=4, kmin=3, kmax=60)
    return h, w, anns, pn.annotation_masks(anns, h, w)


def test_480x640_40_annotations_bit_identical(big):
    from cim_amd import segm_eval
    h, w, anns, want = big
    assert len(anns) == 40 and all(1 <= len(a) <= 4 for a in anns)
    assert all(3 <= len(p) // 2 <= 61 for a in anns for p in a)          # (a repeated vertex adds one to the 60 drawn)
    flat = np.concatenate([np.asarray(p) for a in anns for p in a])
    assert (flat < 0).any() and (flat != np.round(flat)).any() and (flat[0::2] > w).any() and (flat[1::2] > h).any()
    assert want[5, 100:150, 550:600].all()                              # the overlap of annotation 5's two squares is filled
    got = unpack(segm_eval.poly_masks(anns, h, w, DEV), h, w)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert sum(int(m.any()) for m in want) >= 30


def test_rle_counts_of_polygon_masks(big):
    from cim_amd import segm_eval
    h, w, anns, want = big
    counts, off = segm_eval.rle_counts(segm_eval.poly_masks(anns, h, w, DEV), h, w)
    for i, m in enumerate(want):
        assert np.array_equal(counts[off[i]:off[i + 1]], sen.encode_counts(m)), i


def _check_eval_imgs(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is None:
            continue
        assert g["image_id"] == w["image_id"] and g["category_id"] == w["category_id"]
        assert list(g["dtIds"]) == list(w["dtIds"]) and list(g["gtIds"]) == list(w["gtIds"])
        assert np.array_equal(g["dtMatches"], w["dtMatches"].astype(np.int64).reshape(g["dtMatches"].shape))
        assert np.array_equal(g["dtScores"], np.asarray(w["dtScores"], np.float64))
        assert np.array_equal(g["gtIgnore"], np.asarray(w["gtIgnore"]).astype(bool))
        assert np.array_equal(g["dtIgnore"], w["dtIgnore"].reshape(g["dtIgnore"].shape))


def _eval_inputs(h, w, anns, masks, seed):
    """Annotation fields and detections (the annotations' own masks, shifted ones and two empty ones) for an evaluator."""
    rs = np.random.RandomState(seed)
    n = len(anns)
    cats = rs.randint(1, 4, size=n)
    crowd = (rs.rand(n) < 0.15).astype(np.int32)
    area = masks.reshape(n, -1).sum(1).astype(np.float64)
    ids = np.arange(n) + 10
    dt = np.concatenate([masks, np.roll(masks, 7, axis=2), np.zeros((2, h, w), np.uint8)])
    dcat = np.concatenate([cats, cats, [1, 2]])
    score = ((rs.permutation(1 << 16)[:len(dt)] + 1) / np.float32(1 << 16)).astype(np.float32)
    return cats, crowd, area, ids, dt, dcat, score


def test_add_image_mixed_polygons_and_rles(big):
    """Polygon lists among RLEs, and polygons alone, give the same evalImgs records as the same masks passed as RLEs."""
    from cim_amd import segm_eval
    h, w, anns, masks = big
    cats, crowd, area, ids, dt, dcat, score = _eval_inputs(h, w, anns, masks, 5)
    rles = [sen.encode(m) for m in masks]
    dt_rles = [sen.encode(m) for m in dt]
    mixed = [rles[i] if i % 3 == 0 else anns[i] for i in range(len(anns))]
    evs = []
    for gt, size in ((rles, None), (mixed, None), (mixed, (h, w)), (list(anns), (h, w))):
        ev = segm_eval.SegmEvaluator([7], [1, 2, 3])
        ev.add_image(7, gt, cats, crowd, area, ids, dt_rles, dcat, score, size=size)
        evs.append((ev.eval_imgs(), segm_eval.to_host(ev.accumulate())))
    ref = sen.SegmEvalNp([7], [1, 2, 3])
    ref.add_image(7, masks, cats, crowd, area, ids, dt, dcat, score)
    ref.evaluate()
    ref.accumulate()
    for imgs, res in evs:
        _check_eval_imgs(imgs, ref.evalImgs)
        for k in ("precision", "recall", "scores"):
            assert np.array_equal(res[k].view(np.uint64), ref.eval[k].view(np.uint64)), k
    ev = segm_eval.SegmEvaluator([7], [1, 2, 3])
    with pytest.raises(ValueError, match="must match"):                  # the size refusals still apply
        ev.add_image(7, mixed, cats, crowd, area, ids, dt_rles, dcat, score, size=(h, w + 1))
    with pytest.raises(ValueError, match="must match"):
        ev.add_image(7, list(anns), cats, crowd, area, ids, [sen.encode(m[:, :-1]) for m in dt], dcat, score, size=(h, w))
    with pytest.raises(ValueError, match="size"):
        ev.add_image(7, list(anns), cats, crowd, area, ids, dt_rles, dcat, score)             # polygons alone, no size
    with pytest.raises(ValueError, match="ground truths only"):
        ev.add_image(7, rles, cats, crowd, area, ids, [anns[0]] * len(dt), dcat, score)


def _json_dataset(seed):
    """Three images of polygon annotations (one crowd region as uncompressed counts, one annotation already a compressed
    RLE) and RLE predictions."""
    rs = np.random.RandomState(seed)
    images, annotations, preds, per_image = [], [], [], []
    next_id = 1
    for img_id, (h, w) in ((3, (60, 80)), (1, (75, 50)), (2, (64, 64))):
        images.append({"id": img_id, "height": h, "width": w})
        anns = poly_cases.random_scene(rs, h, w, 6, max_polys=3, kmin=3, kmax=10)
        masks = pn.annotation_masks(anns, h, w)
        cats, crowd, area, ids, dt, dcat, score = _eval_inputs(h, w, anns, masks, seed + img_id)
        ids = np.arange(next_id, next_id + len(anns))
        next_id += len(anns)
        for j in range(len(anns)):
            seg = anns[j]
            if j == 1:
                seg = {"size": [h, w], "counts": [int(c) for c in sen.encode_counts(masks[j])]}
            elif j == 2:
                seg = sen.encode(masks[j])
            annotations.append({"id": int(ids[j]), "image_id": img_id, "category_id": int(cats[j]), "iscrowd": int(crowd[j]),
                                "area": float(area[j]), "segmentation": seg})
        for m, c, s in zip(dt, dcat, score):
            preds.append({"image_id": img_id, "category_id": int(c), "score": float(s), "segmentation": sen.encode(m)})
        per_image.append((img_id, masks, cats, crowd, area, ids, dt, dcat, score))
    gt = {"images": images, "annotations": annotations, "categories": [{"id": c, "name": "class%d" % c} for c in (3, 1, 2)]}
    return gt, preds, per_image


def test_json_evaluator_rasterize(tmp_path):
    from cim_amd.datasets import json_inference
    gt, preds, per_image = _json_dataset(31)
    with pytest.raises(NotImplementedError):                            # the default still refuses polygons
        json_inference.coco_inst_seg_eval(gt, preds)
    with pytest.raises(ValueError):
        json_inference.InstanceEvaluator(gt, preds, polygons="fill")
    direct = json_inference.coco_inst_seg_eval(gt, preds, polygons="rasterize")
    out_file = tmp_path / "gt_rle.json"
    before = json.dumps(gt)
    converted = json_inference.rasterize_polygons(gt, str(out_file))
    assert json.dumps(gt) == before                                      # the input is not modified
    assert json.loads(out_file.read_text()) == converted
    assert all(isinstance(a["segmentation"]["counts"], (str, list)) for a in converted["annotations"])
    by_default = json_inference.coco_inst_seg_eval(str(out_file), preds)
    assert direct[0] == by_default[0] and direct[1] == by_default[1] and direct[2] == by_default[2]
    # the converter's strings and annToRLE are the restatement's masks, encoded
    coco = json_inference.CocoJson(gt)
    masks_of = {int(i): m for _, masks, _, _, _, ids, _, _, _ in per_image for i, m in zip(ids, masks)}
    for a_in, a_out in zip(gt["annotations"], converted["annotations"]):
        want = sen.encode(masks_of[a_in["id"]])
        assert coco.annToRLE(a_in) == want, a_in["id"]
        if isinstance(a_in["segmentation"], list):
            assert a_out["segmentation"] == want
        else:
            assert a_out is a_in
    # and the AP is the restatement's of those masks
    thr = np.asarray([0.25, 0.5, 0.7, 0.75])
    ref = sen.SegmEvalNp([1, 2, 3], [1, 2, 3], iou_thrs=thr)
    for img_id, masks, cats, crowd, area, ids, dt, dcat, score in per_image:
        ref.add_image(img_id, masks, cats, crowd, area, ids, dt, dcat, score)
    ref.evaluate()
    ref.accumulate()
    mAP, cls_ap, names = direct
    assert names == ["class3", "class1", "class2"]
    for ti, t in enumerate(thr):
        want = []
        for ci in range(3):
            p = ref.eval["precision"][ti, :, ci, 0, -1]
            tmp = p[p > -1]
            want.append(np.mean(tmp) if len(tmp) else 0)
        assert cls_ap["%.2f" % t] == want
        assert mAP["%.2f" % t] == np.asarray(want).mean()
    assert any(v > 0 for v in mAP.values())


def test_two_threads_two_streams(big):
    from cim_amd import segm_eval
    h, w, anns, want = big
    parts = [(anns[:20], want[:20]), (anns[20:], want[20:])]
    torch.cuda.synchronize()
    errors = []

    def worker(k):
        try:
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                for _ in range(3):
                    packed = segm_eval.poly_masks(parts[k][0], h, w, DEV)
                    stream.synchronize()
                    assert np.array_equal(unpack(packed, h, w), parts[k][1]), k
        except BaseException as e:                                    # noqa: BLE001 - reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


@pytest.mark.parametrize("h,w", [(9, 11), (37, 53)])
def test_garbage_in_workspace_and_output_does_not_leak(h, w):
    """The C entry point with its workspace and its output pre-filled with ones: same masks, nothing past h w."""
    from cim_amd import _lib, segm_eval
    anns = _small_scene(h, w, 7)
    want = pn.annotation_masks(anns, h, w)
    xy, poly_off, poly_ann, edge_off, total = segm_eval._polygon_arrays(anns, h, w)
    words = segm_eval.words_of(h, w)
    assert (h * w) % 64 != 0
    ws_bytes = _lib.call("cim_poly_ws_bytes", len(poly_ann), h, w)
    assert ws_bytes >= 8 * len(poly_ann) * words
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=DEV)
    packed = torch.full((len(anns), words), -1, dtype=torch.int64, device=DEV)
    d = [torch.from_numpy(a).to(DEV) for a in (xy, poly_off, poly_ann, edge_off)]
    _lib.call("cim_poly_fill", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), len(poly_ann), xy.size // 2,
              total, len(anns), h, w, ws.data_ptr(), packed.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(unpack(packed, h, w), want)


def test_poly_masks_refusals():
    from cim_amd import _lib, segm_eval
    tri = [0.0, 0.0, 4.0, 0.0, 4.0, 4.0]
    for bad in ([0, 0, 4, 0, 4, 4, 1], [0, 0, 4, 4], [0, 0, 4, 0, float("nan"), 4], [0, 0, 4, 0, 2.0 ** 20 + 1, 4]):
        with pytest.raises(ValueError):
            segm_eval.poly_masks([[tri], [bad]], 8, 8, DEV)
    with pytest.raises(ValueError):
        segm_eval.poly_masks([[tri]], 2048, 2049, DEV)
    with pytest.raises(_lib.CimHipError):
        segm_eval.poly_masks([[tri]], 8, 8, "cpu")
    assert segm_eval.poly_masks([], 8, 8, DEV).shape == (0, 1)
    assert not unpack(segm_eval.poly_masks([[], []], 8, 8, DEV), 8, 8).any()
