"""-m gpu: box evaluation on the device (csrc/box_eval.hip) against the NumPy restatement (tests/golden/box_eval_np.py) and
the golden captured from the reference (tests/golden/box_eval_voc.npz): COCOeval 'bbox' records and fp64 precision / recall /
scores bit for bit, the box path against the mask path on rectangles, cim_voc_match's decisions, cim_voc_ap's rec / prec /
AP, and the voc_eval / dis_eval file drop-ins."""
import os

import numpy as np
import pytest
import torch

import box_eval_np as ben

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53


def xyxy(x, y, w, h):
    """The fp32 (x1, y1, x2, y2) box whose reference xywh form is (x, y, w, h)."""
    return [x, y, x + w - 1, y + h - 1]


def to_xywh(b):
    b = np.asarray(b, np.float32).reshape(-1, 4).astype(np.float64)
    return np.hstack((b[:, 0:2], b[:, 2:4] - b[:, 0:2] + 1))


def bits_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_eval_imgs(got, want):
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


# ---- COCO 'bbox' ---------------------------------------------------------------------------------------------------------------
def coco_images():
    """3 images x 3 categories; every edge case of the issue's list is named where it is built."""
    rs = np.random.RandomState(5)
    gid = [0]

    def gts(rows):                                                       # (x, y, w, h, cat, crowd) -> fields
        out = dict(box=[], cat=[], crowd=[], area=[], ids=[])
        for x, y, w, h, c, cr in rows:
            gid[0] += 1
            out["box"].append((x, y, w, h)), out["cat"].append(c), out["crowd"].append(cr), out["area"].append(w * h)
            out["ids"].append(gid[0])
        return out

    a_g = gts([(10, 10, 20, 20, 1, 0),                                   # g1
               (50, 50, 40, 40, 1, 1),                                   # a crowd, matched twice below
               (120, 10, 16, 16, 1, 0), (120, 10, 16, 16, 1, 0),         # equal IoUs: the later ground truth wins
               (200, 200, 30, 30, 3, 0)])                                # category 3: ground truth and no detection
    a_d = [(xyxy(10, 10, 20, 20), 1, 0.9), (xyxy(12, 10, 20, 20), 1, 0.9),    # equal scores on g1
           (xyxy(55, 55, 10, 10), 1, 0.8), (xyxy(60, 60, 20, 20), 1, 0.7),    # both inside the crowd
           (xyxy(30, 10, 10, 10), 1, 0.6),                               # only touches g1 (w == 0)
           (xyxy(12, 12, 0, 5), 1, 0.5),                                 # zero area
           (xyxy(300, 300, 32, 32), 1, 0.4),                             # area 1024: the small / medium edge
           (xyxy(300, 100, 96, 96), 1, 0.35),                            # area 9216: the medium / large edge
           (xyxy(120, 10, 16, 16), 1, 0.3),
           (xyxy(5, 5, 50, 50), 2, 0.9), (xyxy(7.25, 5.5, 40.75, 50), 2, 0.2)]     # category 2: detections and no ground truth
    b_rows = [(8 * (k % 10) * 3, 8 * (k // 10) * 3, 20, 20, 1, int(k % 17 == 3)) for k in range(70)]   # 70 ground truths, one group
    b_rows += [(40, 40, 60, 50, 2, 0), (200, 40, 35.5, 50.25, 2, 0), (100, 200, 80, 80, 2, 1)]
    b_g = gts(b_rows)
    b_d = []
    for k in range(0, 70, 2):
        x, y = 8 * (k % 10) * 3, 8 * (k // 10) * 3
        j = rs.randint(-3, 4, 2)
        b_d.append((xyxy(x + j[0], y + j[1], 20, 20), 1, rs.randint(1, 9) / 8.0))
    for k in range(130):                                                 # 130 detections of one group, maxDets[-1] = 100
        x, y = np.round(rs.uniform(0, 250, 2) * 4) / 4
        w, h = np.round(rs.uniform(5, 90, 2) * 4) / 4
        b_d.append((xyxy(x, y, w, h), 2, rs.randint(1, 33) / 32.0))
    empty = gts([])
    return [(10, a_g, a_d), (20, b_g, b_d), (30, empty, [])]             # image 30 has neither


def coco_run(cls, imgs, device, **kw):
    ev = cls([i for i, _, _ in imgs], [1, 2, 3], **kw)
    for j, (img_id, g, d) in enumerate(imgs):
        boxes = np.asarray([x[0] for x in d], np.float32).reshape(-1, 4)
        cats, scores = [x[1] for x in d], np.asarray([x[2] for x in d], np.float32)
        if device:
            db = torch.from_numpy(boxes).to(DEV) if j % 2 == 0 else boxes
            sc = torch.from_numpy(scores).to(DEV) if j % 2 else scores
            ev.add_image(img_id, g["box"], g["cat"], g["crowd"], g["area"], g["ids"], db, cats, sc)
        else:
            ev.add_image(img_id, g["box"], g["cat"], g["crowd"], g["area"], g["ids"], to_xywh(boxes), cats, scores)
    return ev


def test_coco_bbox_bit_identical():
    from cim_amd import box_eval
    imgs = coco_images()
    ref = coco_run(ben.BoxEvalNp, imgs, False)
    ref.evaluate()
    ref.accumulate()
    ref.summarize()
    ev = coco_run(box_eval.BoxEvaluator, imgs, True)
    res = box_eval.to_host(ev.accumulate())
    check_eval_imgs(ev.eval_imgs(), ref.evalImgs)
    for k in ("precision", "recall", "scores"):
        assert bits_equal(res[k], ref.eval[k]), k
    assert np.array_equal(ev.summarize(res), ref.stats)
    # the restatement saw the cases the inputs were built for
    e = {(x["image_id"], x["category_id"], tuple(x["aRng"])): x for x in ref.evalImgs if x is not None}
    allr = (0.0, 1e10)
    a1 = e[10, 1, allr]
    crowd_id, later_id = 2, 4
    assert np.count_nonzero(a1["dtMatches"][0] == crowd_id) == 2        # the crowd, twice
    assert later_id in a1["dtMatches"][0] and 3 not in a1["dtMatches"][0]
    assert a1["dtMatches"][0][list(a1["dtIds"]).index(4)] == 0           # the touching box matches nothing
    small, medium = e[10, 1, (0.0, 1024.0)], e[10, 1, (1024.0, 9216.0)]
    i1024 = list(small["dtIds"]).index(6)
    assert not small["dtIgnore"][0][i1024] and not medium["dtIgnore"][0][i1024]      # 1024 lies in both ranges
    assert len(e[20, 2, allr]["dtIds"]) == 100 and len(e[20, 1, allr]["gtIds"]) == 70
    assert len(e[10, 2, allr]["gtIds"]) == 0 and len(e[10, 3, allr]["dtIds"]) == 0 and (30, 1, allr) not in e


def test_box_path_equals_mask_path_on_rectangles():
    """Axis-aligned rectangles with integer (x, y, w, h): bbIou is the pixel IoU, so the two evaluators agree bit for bit."""
    from cim_amd import box_eval, segm_eval
    rs = np.random.RandomState(11)
    H = W = 64
    imgs = []
    for i in range(4):
        rect = lambda: (int(rs.randint(0, 40)), int(rs.randint(0, 40)), int(rs.randint(1, 24)), int(rs.randint(1, 24)))
        g = [rect() for _ in range(rs.randint(0, 5))]
        d = [rect() for _ in range(rs.randint(0, 12))] + [b for b in g if rs.rand() < 0.7]
        imgs.append((i + 1, g, rs.randint(1, 3, len(g)), (rs.rand(len(g)) < 0.2).astype(int), d, rs.randint(1, 3, len(d)),
                     (rs.randint(1, 17, len(d)) / 16.0).astype(np.float32)))
    sev = segm_eval.SegmEvaluator(range(1, 5), [1, 2])
    bev = box_eval.BoxEvaluator(range(1, 5), [1, 2])

    def masks(rects):
        m = np.zeros((len(rects), H, W), np.uint8)
        for k, (x, y, w, h) in enumerate(rects):
            m[k, y:y + h, x:x + w] = 1
        return torch.from_numpy(m).to(DEV)

    for img_id, g, gc, gcrowd, d, dc, sc in imgs:
        area, ids = [w * h for _, _, w, h in g], [100 * img_id + k for k in range(len(g))]
        sev.add_image(img_id, masks(g), gc, gcrowd, area, ids, masks(d), dc, sc)
        bev.add_image(img_id, g, gc, gcrowd, area, ids, np.asarray([xyxy(*b) for b in d], np.float32).reshape(-1, 4), dc, sc)
    s, b = segm_eval.to_host(sev.accumulate()), box_eval.to_host(bev.accumulate())
    assert (s["precision"] > 0).any()
    for k in ("precision", "recall", "scores"):
        assert bits_equal(s[k], b[k]), k


# ---- VOC match -------------------------------------------------------------------------------------------------------------------
def voc_match_case():
    rs = np.random.RandomState(3)
    dbox, conf, gbox, diff, groups = [], [], [], [], []

    def group(d, c, g, df):
        groups.append((len(conf), len(c), len(diff), len(df)))
        dbox.extend(d), conf.extend(c), gbox.extend(g), diff.extend(df)

    group([(1, 1, 50, 50), (10, 10, 30, 30)], [0.5, 0.7], [], [])                               # n_gt = 0
    group([], [], [(5, 5, 40, 40)], [0])                                                        # n_det = 0
    group([(5, 5, 40, 40), (6, 6, 41, 41), (100, 100, 120, 130)], [0.9, 0.8, 0.7], [(5, 5, 40, 40), (100, 100, 121, 131)],
          [1, 1])                                                                               # all difficult
    group([(5, 5, 40, 40), (6, 6, 41, 41)], [0.6, 0.9], [(5, 5, 40, 40)], [0])                  # two detections, one ground truth
    group([(20, 20, 60, 60)], [0.4], [(20, 20, 60, 60), (20, 20, 60, 60)], [0, 0])              # equal overlap: the first wins
    group([(5, 5, 40, 40), (5, 5, 41, 41), (5, 5, 41, 41), (200, 200, 210, 210)], [0.5, 0.5, 0.5, 0.5],
          [(5, 5, 40, 40), (5, 5, 41, 41)], [0, 0])                                             # confidence ties
    g = [(30 * (k % 13), 30 * (k // 13), 30 * (k % 13) + 24, 30 * (k // 13) + 24) for k in range(65)]
    d = []
    for k in range(300):                                                                        # 300 detections, 65 ground truths
        b = np.asarray(g[rs.randint(65)], np.float64) + np.round(rs.uniform(-8, 8, 4) * 10) / 10
        d.append(tuple(b))
    group(d, list(rs.randint(1, 101, 300) / 100.0), g, list((rs.rand(65) < 0.2).astype(int)))
    return (np.asarray(dbox, np.float64).reshape(-1, 4), np.asarray(conf, np.float64), np.asarray(gbox, np.float64).reshape(-1, 4),
            np.asarray(diff, np.uint8), np.asarray(groups, np.int32))


@pytest.mark.parametrize("mode", [0, 1])
def test_voc_match_decisions(mode):
    from cim_amd import box_eval
    dbox, conf, gbox, diff, groups = voc_match_case()
    want = ben.voc_match_np(dbox, conf, gbox, diff, groups, 0.5, mode)
    t = lambda a: torch.from_numpy(a).to(DEV)
    got = [x.cpu().numpy() for x in box_eval.voc_match(t(dbox), t(conf), t(gbox), t(diff), t(groups), 0.5, mode)]
    for name, g, w in zip(("tp", "fp", "ovmax", "jmax"), got, want):
        assert g.dtype == w.dtype, name
        bad = np.flatnonzero(g.view(np.uint64) != w.view(np.uint64)) if name == "ovmax" else np.flatnonzero(g != w)
        assert not bad.size, (name, bad[:8], g[bad[:8]], w[bad[:8]])
    tp, fp, ovmax, jmax = want
    assert tp.sum() > 20 and fp.sum() > 20 and np.isneginf(ovmax[:2]).all() and (jmax[:2] == -1).all()
    if mode == 0:
        assert not tp[2:5].any() and not fp[2:5].any()                   # difficult: neither true nor false positive
        assert tp[6] and fp[5]                                           # the higher confidence claims the ground truth
        assert jmax[7] == 0 and tp[7]
        assert list(tp[8:12]) == [1, 1, 0, 0] and list(fp[8:12]) == [0, 0, 1, 1] and list(jmax[8:11]) == [0, 1, 1]   # ties: input order
    else:
        assert tp[2:4].all() and tp[5] and tp[6] and np.array_equal(fp, 1 - tp)


# ---- VOC AP ----------------------------------------------------------------------------------------------------------------------
def voc_ap_case():
    rs = np.random.RandomState(9)
    sizes = [0, 40, 5000, 700]                                           # no detections; npos = 0; 60 runs; ties
    npos = np.asarray([7.0, 0.0, 1800.0, 300.0])
    conf, tp, fp, runs = [], [], [], ([], [], [])
    off = np.concatenate([[0], np.cumsum(sizes)])
    for k, n in enumerate(sizes):
        c = rs.randint(1, 1001, n) / 1000.0 if k == 3 else rs.rand(n)
        kind = rs.randint(0, 3, n) if k != 1 else np.full(n, 1)
        conf.append(c), tp.append((kind == 0).astype(np.uint8)), fp.append((kind == 1).astype(np.uint8))
        cuts = 83 * np.arange(1, 60) + rs.randint(-20, 21, 59) if k == 2 else np.arange(256, n, 256)
        edges = np.concatenate([[0], cuts, [n]]) if n else np.zeros(1, int)
        for a, b in zip(edges[:-1], edges[1:]):
            runs[0].append(off[k] + a), runs[1].append(b - a), runs[2].append(k)
    assert np.count_nonzero(np.asarray(runs[2]) == 2) == 60 and max(runs[1]) <= 256
    return np.concatenate(conf), np.concatenate(tp), np.concatenate(fp), off, npos, tuple(np.asarray(r, np.int64) for r in runs)


@pytest.mark.parametrize("use_07", [True, False])
def test_voc_ap_rec_prec_ap(use_07):
    from cim_amd import box_eval
    conf, tp, fp, off, npos, runs = voc_ap_case()
    rec_w, prec_w = ben.voc_pr_np(conf, tp, fp, off, npos)
    t = lambda a: torch.from_numpy(a).to(DEV)
    rec, prec, ap = (x.cpu().numpy() for x in box_eval.voc_ap(t(conf), t(tp), t(fp), off, npos, runs, use_07))
    assert np.isnan(rec_w[off[1]:off[2]]).all()
    assert np.array_equal(rec, rec_w, equal_nan=True) and bits_equal(rec[off[2]:], rec_w[off[2]:])
    assert bits_equal(prec, prec_w)
    for k in range(4):
        a, b = off[k], off[k + 1]
        with np.errstate(invalid="ignore"):
            want = ben.voc_ap_np(rec_w[a:b], prec_w[a:b], use_07) if b > a else 0.0
        print("class", k, "ap", ap[k], "want", want)
        if use_07:
            assert bits_equal(ap[k], np.float64(want)), k
        elif np.isnan(want):
            assert k == 1 and np.isnan(ap[k])
        else:
            mrec = np.concatenate(([0.], rec_w[a:b], [1.]))
            n = np.count_nonzero(mrec[1:] != mrec[:-1])
            assert abs(ap[k] - want) <= 2 * (n + 1) * U, (k, ap[k], want, n)
    assert ap[0] == 0 and ap[2] > 0.1 and ap[3] > 0.1


# ---- the golden, through the evaluator and through the files --------------------------------------------------------------------
def check_against_golden(g, k, rec, prec, ap07, ap, corloc):
    a, b = g["cls_off"][k], g["cls_off"][k + 1]
    if b == a:
        assert (rec, prec, ap07, ap) == (0, 0, 0, 0)
    else:
        assert np.array_equal(rec, g["rec"][a:b], equal_nan=True) and bits_equal(prec, g["prec"][a:b]), k
        assert bits_equal(np.float64(ap07), g["ap07"][k]), k
        if np.isnan(g["ap"][k]):
            assert np.isnan(ap)
        else:
            mrec = np.concatenate(([0.], g["rec"][a:b], [1.]))
            n = np.count_nonzero(mrec[1:] != mrec[:-1])
            print("class", k, "ap", ap, "golden", g["ap"][k])
            assert abs(ap - g["ap"][k]) <= 2 * (n + 1) * U, k
    assert np.array_equal(np.float64(corloc), g["corloc"][k], equal_nan=True), k


def test_voc_evaluator_equals_reference_golden(golden_dir):
    from cim_amd import box_eval
    g = dict(np.load(os.path.join(golden_dir, "box_eval_voc.npz")))
    K = len(g["classes"])
    evs = [box_eval.VocBoxEvaluator(list(g["classes"]), use_07_metric=u) for u in (True, False)]
    for i, name in enumerate(g["imagenames"]):
        gi = np.flatnonzero(g["gt_img"] == i)
        dets = []
        for k in range(K):
            d = g["dets"][(g["dt_img"] == i) & (g["dt_cls"] == k)]
            dets.append(torch.from_numpy(d).to(DEV) if (i + k) % 2 and len(d) else (d if len(d) else []))
        for ev in evs:
            ev.add_image(str(name), g["gt_box"][gi], g["gt_cls"][gi], g["gt_diff"][gi], dets)
    (r7, m7), (r, m) = evs[0].evaluate(), evs[1].evaluate()
    cl, cmean = evs[0].corloc()
    for k, c in enumerate(g["classes"]):
        assert r7[c][2] == 0 or bits_equal(r7[c][0], r[c][0]) or np.isnan(r[c][0]).all()
        check_against_golden(g, k, r7[c][0], r7[c][1], r7[c][2], r[c][2], cl[c])
    assert bits_equal(np.float64(m7), np.mean(g["ap07"])) and np.isnan(m) and np.isnan(cmean)


def test_voc_eval_and_dis_eval_on_files(golden_dir, tmp_path):
    from cim_amd.datasets import dis_eval, voc_eval
    g = dict(np.load(os.path.join(golden_dir, "box_eval_voc.npz")))
    detpath, annopath, imageset = ben.write_voc_files(str(tmp_path), g)
    cache = str(tmp_path / "cache")
    for k, c in enumerate(g["classes"]):
        r7, p7, a7 = voc_eval.voc_eval(detpath, annopath, imageset, str(c), cache, 0.5, True)
        _, _, a = voc_eval.voc_eval(detpath, annopath, imageset, str(c), cache, use_07_metric=False)
        cl = dis_eval.dis_eval(detpath, annopath, imageset, str(c), cache)
        check_against_golden(g, k, r7, p7, a7, a, cl)


# ---- the COCO drop-in ------------------------------------------------------------------------------------------------------------
def test_evaluate_boxes_on_all_boxes_and_on_a_results_list():
    """cim_amd.datasets.json_dataset_evaluator.evaluate_boxes on a small annotation dict, fed the reference's all_boxes
    structure and the same detections as a results list: .eval and .stats equal the restatement, and category_ap is the
    mean over category k's own column of precision (no __background__ offset)."""
    from cim_amd.datasets import json_dataset_evaluator as jde
    imgs = coco_images()
    cat_ids = [1, 2, 3]
    gt = {"images": [{"id": i, "height": 400, "width": 400} for i, _, _ in imgs],
          "categories": [{"id": c, "name": "cat%d" % c} for c in cat_ids], "annotations": []}
    for img_id, g, _ in imgs:
        for b, c, cr, ar, aid in zip(g["box"], g["cat"], g["crowd"], g["area"], g["ids"]):
            gt["annotations"].append({"id": aid, "image_id": img_id, "category_id": c, "iscrowd": cr, "area": ar,
                                      "bbox": [float(v) for v in b]})
    all_boxes = [[[] for _ in imgs] for _ in range(len(cat_ids) + 1)]
    results = []
    for i, (img_id, _, d) in enumerate(imgs):                            # (sorted image ids: 10, 20, 30)
        for k, c in enumerate(cat_ids):
            rows = [np.r_[x[0], x[2]] for x in d if x[1] == c]
            if rows:
                all_boxes[k + 1][i] = np.asarray(rows, np.float32)
        for box, c, s in d:
            xywh = to_xywh(box)[0]
            results.append({"image_id": img_id, "category_id": c, "bbox": [float(v) for v in xywh], "score": float(np.float32(s))})
    ref = coco_run(ben.BoxEvalNp, imgs, False)
    ref.evaluate()
    ref.accumulate()
    ref.summarize()
    for fed in (all_boxes, results):
        ev = jde.evaluate_boxes(gt, fed)
        for k in ("precision", "recall", "scores"):
            assert bits_equal(ev.eval[k], ref.eval[k]), k
        assert np.array_equal(ev.stats, ref.stats)
        assert list(ev.category_ap) == cat_ids
        for k, c in enumerate(cat_ids):
            p = ref.eval["precision"][:, :, k, 0, 2]
            want = np.mean(p[p > -1]) if (p > -1).any() else np.nan
            assert np.array_equal(np.float64(ev.category_ap[c]), np.float64(want), equal_nan=True), c
    assert ev.category_ap[1] > 0.1 and ev.category_ap[1] != ev.category_ap[2]
    with pytest.raises(ValueError, match="fp32"):
        jde.evaluate_boxes(gt, [dict(results[0], score=0.1)])
    with pytest.raises(AssertionError):
        jde.evaluate_boxes(gt, [dict(results[0], image_id=99)])
