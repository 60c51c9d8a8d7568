"""-m gpu: instance-segmentation evaluation on the device (csrc/segm_eval.hip) bit for bit against the NumPy restatement of
pycocotools (tests/golden/segm_eval_np.py): RLE counts and strings, every evalImgs record, fp64 precision / recall /
scores, the 12 stats - on a VOC-shaped and a COCO-shaped seeded synthetic dataset, end to end from detection scores, through
the JSON evaluator, and from two host threads on two streams."""
import json
import threading

import numpy as np
import pytest
import torch

import segm_eval_np as sen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dataset(seed, n_img, h, w, num_cats, crowd_frac=0.0, score_levels=0, big_group=False):
    from cim_amd import synthetic
    rs = np.random.RandomState(seed)
    imgs = []
    next_id = 0                                                        # ground-truth ids start at 0 (the dtm == 0 quirk)
    for i in range(n_img):
        n_gt = int(rs.randint(0, 7)) if i % 11 else 0
        n_det = int(rs.randint(0, 101)) if i % 13 != 5 else 0
        d = synthetic.make_segm_image(rs, h, w, num_cats, n_gt, n_gt + 40, n_det, crowd_frac, score_levels)
        if big_group and i == 1:                                      # > 100 detections of one (image, category)
            extra = 130
            d["dt_idx"] = np.concatenate([d["dt_idx"], rs.randint(0, d["masks"].shape[0], size=extra)])
            d["dt_cat"] = np.concatenate([d["dt_cat"], np.full(extra, 3)])
            d["dt_score"] = np.concatenate([d["dt_score"], (rs.randint(1, 9, size=extra) / np.float32(8)).astype(np.float32)])
        d["bits"], d["w"] = np.packbits(d.pop("masks"), axis=-1), w       # (200 images of dense masks would take GBs)
        d["gt_ids"] = np.arange(next_id, next_id + n_gt)
        gap = int(rs.randint(0, 3))
        next_id += n_gt + (gap if n_gt else 0)                           # (the first ground truth of the set has id 0)
        if n_gt and d["gt_ids"][0] == 0:                               # a detection of ground truth 0 itself
            d["dt_idx"] = np.concatenate([d["dt_idx"], [0]])
            d["dt_cat"] = np.concatenate([d["dt_cat"], d["gt_cat"][:1]])
            d["dt_score"] = np.concatenate([d["dt_score"], np.float32([0.99])])
        d["img_id"] = 1000 + 7 * (n_img - i)                             # ascending ids != insertion order
        imgs.append(d)
    return imgs


def masks_of(d):
    return np.unpackbits(d["bits"], axis=-1, count=d["w"]).astype(bool)


def _restatement(imgs, cat_ids, **kw):
    ev = sen.SegmEvalNp([d["img_id"] for d in imgs], cat_ids, **kw)
    for d in imgs:
        g = len(d["gt_cat"])
        m = masks_of(d)
        ev.add_image(d["img_id"], m[:g], d["gt_cat"], d["gt_crowd"], d["gt_area"], d["gt_ids"], m[d["dt_idx"]], d["dt_cat"],
                     d["dt_score"])
    ev.evaluate()
    ev.accumulate()
    if len(ev.maxDets) >= 3:                                           # (COCOeval.summarize indexes maxDets[2])
        ev.summarize()
    return ev


def _device(imgs, cat_ids, mode=0, **kw):
    """mode cycles through the input forms: 0 masks, 1 (proposals, indices), 2 RLEs."""
    from cim_amd import segm_eval
    ev = segm_eval.SegmEvaluator([d["img_id"] for d in imgs], cat_ids, **kw)
    for j, d in enumerate(imgs):
        g = len(d["gt_cat"])
        m = (mode + j) % 3
        host = masks_of(d)
        props = torch.from_numpy(host).to(DEV)
        gt = [sen.encode(x) for x in host[:g]] if m == 2 else props[:g]
        if m == 0:
            dt = props[torch.from_numpy(d["dt_idx"]).to(DEV)]
        elif m == 1:
            dt = (props, d["dt_idx"])
        else:
            dt = [sen.encode(host[k]) for k in d["dt_idx"]]
        scores = torch.from_numpy(d["dt_score"]).to(DEV) if j % 2 else d["dt_score"]
        ev.add_image(d["img_id"], gt, d["gt_cat"], d["gt_crowd"], d["gt_area"], d["gt_ids"], dt, d["dt_cat"], scores)
        del props, gt, dt                                              # (add_image does not synchronise: freeing is safe)
    res = segm_eval.to_host(ev.accumulate())
    return ev, res


def _check_eval_imgs(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is None:
            continue
        assert g["image_id"] == w["image_id"] and g["category_id"] == w["category_id"]
        assert list(g["dtIds"]) == list(w["dtIds"]), (g["image_id"], g["category_id"])
        assert list(g["gtIds"]) == list(w["gtIds"])
        assert np.array_equal(g["dtMatches"], w["dtMatches"].astype(np.int64).reshape(g["dtMatches"].shape))
        assert np.array_equal(g["dtScores"], np.asarray(w["dtScores"], np.float64))
        assert np.array_equal(g["gtIgnore"], np.asarray(w["gtIgnore"]).astype(bool))
        assert np.array_equal(g["dtIgnore"], w["dtIgnore"].reshape(g["dtIgnore"].shape))


def _check_bits(res, ref):
    for k in ("precision", "recall", "scores"):
        assert res[k].dtype == np.float64 and res[k].shape == ref.eval[k].shape
        bad = res[k].view(np.uint64) != ref.eval[k].view(np.uint64)
        assert not bad.any(), (k, np.argwhere(bad)[:5], res[k][bad][:5], ref.eval[k][bad][:5])


@pytest.fixture(scope="module")
def voc():
    imgs = _dataset(1, 200, 375, 500, 20)
    cats = list(range(1, 21))
    return imgs, cats, _restatement(imgs, cats)


@pytest.fixture(scope="module")
def coco():
    imgs = _dataset(2, 36, 480, 640, 80, crowd_frac=0.15, score_levels=16, big_group=True)
    cats = list(range(1, 81))
    return imgs, cats, _restatement(imgs, cats)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_voc_shaped_bit_identical(voc, mode):
    imgs, cats, ref = voc
    ev, res = _device(imgs, cats, mode)
    _check_eval_imgs(ev.eval_imgs(), ref.evalImgs)
    _check_bits(res, ref)
    assert np.array_equal(ev.summarize(res), ref.stats)
    assert (res["precision"] > 0).any() and (res["precision"] == -1).any()


def test_coco_shaped_bit_identical(coco):
    imgs, cats, ref = coco
    assert any(len(d["dt_idx"]) > 100 and np.count_nonzero(d["dt_cat"] == 3) > 100 for d in imgs)
    assert any((d["gt_crowd"] == 1).any() for d in imgs)
    ev, res = _device(imgs, cats, 1)
    _check_eval_imgs(ev.eval_imgs(), ref.evalImgs)
    _check_bits(res, ref)
    assert np.array_equal(ev.summarize(res), ref.stats)
    # the quirks the data exercises: a match to ground-truth id 0, crowd matches, ties of score
    recs = [e for e in ref.evalImgs if e is not None]
    assert any(0 in e["gtIds"] and (e["gtMatches"][:, e["gtIds"].index(0)] > 0).any() for e in recs)   # matched, yet dtm == 0
    assert any(e["gtIgnore"].any() for e in recs)


def test_coco_shaped_other_parameters(coco):
    """Thresholds of json_inference, one area range, maxDets (1, 100): the device takes the host's arrays as given."""
    imgs, cats, _ = coco
    kw = dict(iou_thrs=np.asarray([0.25, 0.5, 0.7, 0.75]), area_rng=[[0, 1e10]], max_dets=(1, 100))
    ref = _restatement(imgs, cats, **kw)
    ev, res = _device(imgs, cats, 2, **kw)
    _check_eval_imgs(ev.eval_imgs(), ref.evalImgs)
    _check_bits(res, ref)


def test_rle_encode_decode_match_restatement(coco):
    from cim_amd import segm_eval
    from cim_amd.utils import mask_eval_utils
    m = masks_of(coco[0][3])
    extra = np.zeros((4,) + m.shape[1:], bool)
    extra[1] = True                                                    # all ones: a zero-length first run
    extra[2, 0, 0] = True                                              # first pixel only
    extra[3, -1, -1] = True                                            # last pixel only
    m = np.concatenate([m, extra])
    md = torch.from_numpy(m).to(DEV)
    got = segm_eval.rle_encode(md)
    want = [sen.encode(x) for x in m]
    assert got == want
    packed, hw = segm_eval.rle_decode(want, DEV)
    assert hw == m.shape[1:]
    assert torch.equal(packed, segm_eval.pack_masks(md))
    packed_u, _ = segm_eval.rle_decode([{"size": w["size"], "counts": sen.string_to_counts(w["counts"]).tolist()} for w in want], DEV)
    assert torch.equal(packed_u, packed)
    area = segm_eval.mask_areas(packed).cpu().numpy()
    assert np.array_equal(area, m.reshape(len(m), -1).sum(1))
    for x in (m[0], m[5].astype(np.uint8), extra[1]):
        assert mask_eval_utils.coco_encode(x.astype(np.uint8)) == sen.encode(x)
    assert mask_eval_utils.coco_encode(md[7]) == sen.encode(m[7])
    odd = np.zeros((7, 9), np.uint8)                                   # 63 pixels: a partial last word
    odd[2:5, 3:8] = 1
    assert mask_eval_utils.coco_encode(odd) == sen.encode(odd)


def test_end_to_end_from_scores(voc):
    """scores -> mask_results_with_nms_and_limit_get_index -> proposal masks -> evaluator, against the restatement fed
    the same indices."""
    from cim_amd import segm_eval, synthetic
    from cim_amd.core.config import cfg
    from cim_amd.utils import mask_eval_utils
    rs = np.random.RandomState(9)
    C = 20
    cfg.MODEL.NUM_CLASSES = C
    cfg.TEST.SCORE_THRESH, cfg.TEST.NMS, cfg.TEST.DETECTIONS_PER_IM = 1e-5, 0.3, 100
    ids = list(range(1, 25))
    ref = sen.SegmEvalNp(ids, list(range(1, C + 1)))
    ev = segm_eval.SegmEvaluator(ids, list(range(1, C + 1)))
    for img_id in ids:
        d = synthetic.make_segm_image(rs, 375, 500, C, int(rs.randint(1, 6)), 300, 0)
        cls, _, _ = synthetic.make_scores(300, C, rs)
        scores = torch.from_numpy(np.ascontiguousarray(cls[:, 1:])).to(DEV)
        boxes = torch.from_numpy(d["boxes"]).to(DEV)
        _, _, cls_boxes, cls_inds = mask_eval_utils.mask_results_with_nms_and_limit_get_index(cfg, scores, boxes, 100)
        idx = np.concatenate([np.asarray(cls_inds[j + 1], np.int64) for j in range(C)])
        cat = np.concatenate([np.full(len(cls_inds[j + 1]), j + 1) for j in range(C)])
        sc = np.concatenate([cls_boxes[j + 1][:, 4] for j in range(C)]).astype(np.float32)
        g = len(d["gt_cat"])
        gids = np.arange(g) + 10 * img_id
        props = torch.from_numpy(d["masks"]).to(DEV)
        ev.add_image(img_id, props[:g], d["gt_cat"], d["gt_crowd"], d["gt_area"], gids, (props, idx), cat, sc)
        ref.add_image(img_id, d["masks"][:g], d["gt_cat"], d["gt_crowd"], d["gt_area"], gids, d["masks"][idx], cat, sc)
    ref.evaluate()
    ref.accumulate()
    res = segm_eval.to_host(ev.accumulate())
    _check_eval_imgs(ev.eval_imgs(), ref.evalImgs)
    _check_bits(res, ref)


def _json_files(tmp_path, imgs, cats):
    images = [{"id": int(d["img_id"]), "height": 480, "width": 640} for d in imgs]
    anns, preds = [], []
    for d in imgs:
        m = masks_of(d)
        for j in range(len(d["gt_cat"])):
            r = sen.encode(m[j])
            if d["gt_crowd"][j]:                                        # crowd regions come with uncompressed counts
                r = {"size": r["size"], "counts": [int(c) for c in sen.encode_counts(m[j])]}
            anns.append({"id": int(d["gt_ids"][j]), "image_id": int(d["img_id"]), "category_id": int(d["gt_cat"][j]),
                         "iscrowd": int(d["gt_crowd"][j]), "area": float(d["gt_area"][j]), "segmentation": r})
        for k, c, s in zip(d["dt_idx"], d["dt_cat"], d["dt_score"]):
            preds.append({"image_id": int(d["img_id"]), "category_id": int(c), "score": float(s),
                          "segmentation": sen.encode(m[k])})
    categories = [{"id": c, "name": "class%d" % c} for c in cats[::-1]]     # file order != id order
    gt_file, pred_file = tmp_path / "gt.json", tmp_path / "pred.json"
    gt_file.write_text(json.dumps({"images": images, "annotations": anns, "categories": categories}))
    pred_file.write_text(json.dumps(preds))
    return str(gt_file), str(pred_file), categories


def test_coco_inst_seg_eval_json(coco, tmp_path):
    from cim_amd.datasets import json_inference
    imgs, cats, _ = coco
    imgs = imgs[:12]
    gt_file, pred_file, categories = _json_files(tmp_path, imgs, cats)
    mAP, cls_ap, names = json_inference.coco_inst_seg_eval(gt_file, pred_file)
    thr = np.asarray([0.25, 0.5, 0.7, 0.75])
    ref = _restatement(imgs, cats, iou_thrs=thr)
    assert names == [c["name"] for c in categories]
    for ti, t in enumerate(thr):
        want = []
        for ci in range(len(names)):
            p = ref.eval["precision"][ti, :, ci, 0, -1]
            tmp = p[p > -1]
            want.append(np.mean(tmp) if len(tmp) else 0)
        assert cls_ap["%.2f" % t] == want
        assert mAP["%.2f" % t] == np.asarray(want).mean()
    assert sorted(mAP) == ["0.25", "0.50", "0.70", "0.75"]


def test_json_evaluator_refusals(tmp_path):
    from cim_amd.datasets import json_inference
    gt = {"images": [{"id": 1, "height": 4, "width": 4}], "categories": [{"id": 1, "name": "a"}],
          "annotations": [{"id": 5, "image_id": 1, "category_id": 1, "iscrowd": 0, "area": 4.0,
                           "segmentation": [[0, 0, 2, 0, 2, 2]]}]}
    with pytest.raises(NotImplementedError, match="5"):
        json_inference.InstanceEvaluator(gt, []).evaluate()
    with pytest.raises(AssertionError):
        json_inference.InstanceEvaluator(gt, [{"image_id": 2, "category_id": 1, "score": 0.5,
                                               "segmentation": {"size": [4, 4], "counts": "<0"}}])
    with pytest.raises(NotImplementedError):
        json_inference.coco_encode(np.zeros((3, 4), np.uint8), 5, 3)
    assert json_inference.coco_encode(np.ones((3, 4), np.uint8) * 7, 4, 3) == sen.encode(np.ones((3, 4), np.uint8))


def test_add_image_refusals():
    from cim_amd import _lib, segm_eval
    ev = segm_eval.SegmEvaluator([1, 2], [1])
    m = torch.zeros(1, 8, 8, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError, match="not among"):
        ev.add_image(3, m, [1], [0], [1.0], [1], m, [1], np.float32([0.5]))
    with pytest.raises(_lib.CimHipError):
        ev.add_image(1, m.cpu(), [1], [0], [1.0], [1], m, [1], np.float32([0.5]))
    with pytest.raises(ValueError, match="must match"):
        ev.add_image(1, m, [1], [0], [1.0], [1], torch.zeros(1, 8, 9, dtype=torch.bool, device=DEV), [1], np.float32([0.5]))
    with pytest.raises(ValueError):
        ev.add_image(2, torch.zeros(1025, 2, 2, dtype=torch.bool, device=DEV), [1] * 1025, [0] * 1025, [1.0] * 1025,
                     list(range(1025)), None, [], np.float32([]))


def test_two_threads_two_streams(voc):
    from cim_amd import segm_eval
    imgs, cats, _ = voc
    parts = [imgs[0:60], imgs[60:120]]
    refs = [_restatement(p, cats) for p in parts]
    torch.cuda.synchronize()
    errors, results = [], [None, None]

    def worker(k):
        try:
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                for rnd in range(3):
                    ev, res = _device(parts[k], cats, (k + rnd) % 3)
                    stream.synchronize()
                    for key in ("precision", "recall", "scores"):
                        assert np.array_equal(res[key].view(np.uint64), refs[k].eval[key].view(np.uint64)), (k, rnd, key)
                results[k] = ev.eval_imgs()
        except BaseException as e:                                    # noqa: BLE001 - reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for k in range(2):
        _check_eval_imgs(results[k], refs[k].evalImgs)
