"""Instance-segmentation evaluation (cim_amd.segm_eval, csrc/segm_eval.hip): the C ABI and its size queries, the host RLE
codec, and the NumPy restatement of COCOeval (tests/golden/segm_eval_np.py) against cases derived by hand below.
No GPU needed."""
import json
import os
import re

import numpy as np
import pytest
import torch

import segm_eval_np as sen

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.spacing(1)
ONE_RNG = [[0, 1e10]]


def box(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def run(gts, dts, iou_thrs=(0.5,), area_rng=ONE_RNG, max_dets=(100,), cats=(1,), img_ids=(1,), images=None):
    """gts: (mask, cat, iscrowd, area, id) per ground truth, dts: (mask, cat, score); one image unless `images`."""
    ev = sen.SegmEvalNp(list(img_ids), list(cats), iou_thrs=None if iou_thrs is None else list(iou_thrs), area_rng=area_rng, max_dets=max_dets)
    for img, (g, d) in (images or {img_ids[0]: (gts, dts)}).items():
        ev.add_image(img, [x[0] for x in g], [x[1] for x in g], [x[2] for x in g], [x[3] for x in g], [x[4] for x in g],
                     [x[0] for x in d], [x[1] for x in d], np.asarray([x[2] for x in d], np.float32))
    ev.evaluate()
    ev.accumulate()
    return ev


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
SEGM_ENTRIES = {"cim_segm_words", "cim_segm_pack", "cim_segm_area", "cim_segm_rle_count", "cim_segm_rle_write",
                "cim_segm_rle_decode_ws_bytes", "cim_segm_rle_decode", "cim_segm_image_ws_bytes", "cim_segm_record_bytes",
                "cim_segm_eval_image", "cim_segm_accumulate_ws_bytes", "cim_segm_accumulate"}


def test_header_declares_and_lib_binds_segm_entries():
    from cim_amd import _lib, build
    header = open(os.path.join(REPO, "include", "cim_hip.h")).read()
    declared = set(re.findall(r"\b(cim_segm_[a-z0-9_]+)\s*\(", header))
    assert declared == SEGM_ENTRIES
    assert declared <= set(_lib.SIGNATURES)
    assert "ABI-16 addition" in header
    for d in ("#define CIM_SEGM_MAX_HW (1 << 22)", "#define CIM_SEGM_MAX_GT 1024", "#define CIM_SEGM_MAX_T 16",
              "#define CIM_SEGM_MAX_R 128", "#define CIM_SEGM_MAX_A 8", "#define CIM_SEGM_MAX_M 4"):
        assert d in header
    build.build()
    lib = _lib.load()
    assert lib.cim_abi_version() == 16
    for name in declared:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]


def test_size_queries_refuse_out_of_range_shapes():
    from cim_amd import _lib, build
    build.build()
    err = lambda: _lib.load().cim_last_error().decode()
    assert _lib.call("cim_segm_words", 375, 500) == (375 * 500 + 63) // 64
    assert _lib.call("cim_segm_words", 2048, 2048) == (1 << 22) // 64
    for h, w in ((0, 5), (5, 0), (2049, 2048), (-1, 3)):
        assert _lib.call("cim_segm_words", h, w) == -1
        assert "H * W <= 4194304" in err()
    assert _lib.call("cim_segm_image_ws_bytes", 100, 20, 2000) > 8 * 2000
    for d, g, p in ((-1, 3, 0), (10, 1025, 0), (10, 10, 101), (10, 10, -1)):
        assert _lib.call("cim_segm_image_ws_bytes", d, g, p) == -1
        assert "1024 ground truths" in err()
    # dtm 8 A T nd + score 4 nd + order 4 nd + npig 4 A + gt order 4 A ng + dt ignore A T nd + gt ignore A ng, 8-aligned
    assert _lib.call("cim_segm_record_bytes", 100, 3, 4, 10) == 32000 + 400 + 400 + 16 + 48 + 4000 + 16
    for args in ((8193, 1, 4, 10), (1, 1025, 4, 10), (1, 1, 9, 10), (1, 1, 4, 17), (1, 1, 0, 10)):
        assert _lib.call("cim_segm_record_bytes", *args) == -1
    assert _lib.call("cim_segm_accumulate_ws_bytes", 1000, 80, 4, 10) > 0
    for args in ((-1, 80, 4, 10), (1 << 31, 80, 4, 10), (10, 0, 4, 10), (10, 80, 9, 10), (10, 80, 4, 17)):
        assert _lib.call("cim_segm_accumulate_ws_bytes", *args) == -1
    assert _lib.call("cim_segm_rle_decode_ws_bytes", 10) >= 40
    assert _lib.call("cim_segm_rle_decode_ws_bytes", -1) == -1


def test_record_layout_matches_the_library():
    from cim_amd import _lib, build, segm_eval
    build.build()
    for nd, ng, A, T in ((0, 0, 1, 1), (1, 0, 4, 10), (0, 5, 4, 10), (100, 7, 4, 10), (37, 1024, 8, 16)):
        assert _lib.call("cim_segm_record_bytes", nd, ng, A, T) == segm_eval.record_layout(nd, ng, A, T)["bytes"]


def test_segm_eval_rejects_cpu_tensors():
    from cim_amd import _lib, segm_eval
    with pytest.raises(_lib.CimHipError):
        segm_eval.pack_masks(torch.zeros(2, 5, 5, dtype=torch.uint8))
    with pytest.raises(_lib.CimHipError):
        segm_eval.rle_encode(torch.zeros(1, 5, 5, dtype=torch.bool))
    with pytest.raises(_lib.CimHipError):
        segm_eval.rle_decode([{"size": [2, 2], "counts": "04"}], device="cpu")


def test_merge_schedule_pairs_runs_within_categories():
    from cim_amd.segm_eval import merge_rounds
    # category 0: runs of 3, 2, 4, 1 elements; category 1: one run; category 2: runs of 2, 2, 2
    start = [0, 3, 5, 9, 10, 15, 17, 19]
    length = [3, 2, 4, 1, 5, 2, 2, 2]
    cat = [0, 0, 0, 0, 1, 2, 2, 2]
    r = merge_rounds(start, length, cat)
    assert len(r) == 2
    assert r[0].tolist() == [[0, 3, 2], [5, 4, 1], [10, 5, 0], [15, 2, 2], [19, 2, 0]]
    assert r[1].tolist() == [[0, 5, 5], [10, 5, 0], [15, 4, 2]]
    for jobs in r:                                                      # every round covers every element once
        covered = np.concatenate([np.arange(s, s + a + b) for s, a, b in jobs])
        assert np.array_equal(covered, np.arange(21))
    assert merge_rounds([0, 4], [4, 3], [0, 1]) == []


# ---- RLE ---------------------------------------------------------------------------------------------------------------------
def test_rle_hand_derived_strings():
    from cim_amd.utils import rle
    # [[0, 1], [1, 1]] column-major: 0, 1, 1, 1 -> counts [1, 3] -> '1', '3'
    m = np.array([[0, 1], [1, 1]], np.uint8)
    assert sen.encode_counts(m).tolist() == [1, 3]
    assert sen.encode(m) == {"size": [2, 2], "counts": "13"}
    # starts with a one: a zero-length first run
    assert sen.encode_counts(np.ones((3, 3), np.uint8)).tolist() == [0, 9]
    assert sen.encode(np.ones((3, 3), np.uint8))["counts"] == "09"
    assert sen.encode(np.zeros((3, 4), np.uint8))["counts"] == "<"                 # [12] -> chr(48 + 12)
    # 20 needs two groups: 20 has bit 0x10 set, so a second (zero) group follows: chr(48 + (20 | 0x20)) + '0'
    # 100: groups 4 | 0x20, 3; index 3 codes 30 - 20 = 10; index 4 codes 1 - 100 = -99
    cnts = [5, 20, 100, 30, 1]
    want = "5" + chr(48 + (20 | 0x20)) + "0" + chr(48 + (4 | 0x20)) + "3" + chr(48 + 10)
    x = -99                                                                        # -99 = ...1110011101: groups 29 | 0x20, 28
    want += chr(48 + ((x & 31) | 0x20)) + chr(48 + ((x >> 5) & 31))
    assert (x & 31) == 29 and ((x >> 5) & 31) == 28 and (x >> 10) == -1
    assert sen.counts_to_string(cnts) == want
    assert rle.counts_to_string(cnts) == want
    # i > 2, not i >= 2: index 2 is coded whole; index 3 against index 1 - a difference of -1 is the one group 31
    assert sen.counts_to_string([1, 2, 3, 1]) == "123O"
    assert rle.counts_to_string([1, 2, 3, 1]) == "123O"
    assert rle.string_to_counts("123O").tolist() == [1, 2, 3, 1]
    assert rle.string_to_counts(want).tolist() == cnts
    assert rle.counts_to_string([]) == "" and rle.string_to_counts("").size == 0


def test_rle_round_trips_string_counts_mask():
    from cim_amd.utils import rle
    rs = np.random.RandomState(0)
    for trial in range(200):
        n = rs.randint(1, 60)
        big = trial % 5 == 0
        cnts = rs.randint(0, (1 << 31) if big else 3000, size=n).astype(np.uint32)
        if trial % 7 == 0:
            cnts[rs.randint(0, n)] = 0xFFFFFFFF if big else 0
        s = rle.counts_to_string(cnts)
        assert s == sen.counts_to_string(cnts)
        assert np.array_equal(rle.string_to_counts(s), cnts)
        assert np.array_equal(sen.string_to_counts(s), cnts)
    for trial in range(50):
        h, w = rs.randint(1, 40), rs.randint(1, 40)
        m = (rs.rand(h, w) < rs.rand()).astype(np.uint8)
        c = sen.encode_counts(m)
        assert c.sum() == h * w and (c[1:] > 0).all()
        assert np.array_equal(sen.decode_counts(c, h, w), m)
        assert np.array_equal(rle.counts_to_mask(c, h, w), m)
        assert np.array_equal(rle.string_to_counts(sen.encode(m)["counts"]), c)


def test_rle_rejects_malformed_strings():
    from cim_amd.utils import rle
    with pytest.raises(ValueError):
        rle.string_to_counts("1" + chr(48 + 0x20))                   # continuation bit on the last character
    with pytest.raises(ValueError):
        rle.string_to_counts("/")
    with pytest.raises(ValueError):
        rle.counts_to_string([-1])


# ---- COCOeval restatement against hand-derived results ----------------------------------------------------------------------
def test_tp_fp_tp_average_precision():
    """Two ground truths, detections TP / FP / TP at 0.9 / 0.8 / 0.7, t = 0.5: tp = [1, 1, 2], fp = [0, 1, 1], npig = 2,
    rc = [.5, .5, 1], pr = [1 / (1 + 2^-52), 1 / 2, 2 / 3] -> envelope [p0, 2/3, 2/3]; recall thresholds <= .5 (51 of
    them) land on detection 0, the other 50 on detection 2: AP = (51 p0 + 50 (2/3)) / 101."""
    g1, g2 = box(10, 10, 0, 4, 0, 4), box(10, 10, 6, 10, 6, 10)
    fp = box(10, 10, 0, 3, 6, 10)
    ev = run([(g1, 1, 0, 16, 11), (g2, 1, 0, 16, 12)], [(g1, 1, 0.9), (fp, 1, 0.8), (g2, 1, 0.7)])
    p0 = 1.0 / (1.0 + 2.0 ** -52)
    assert p0 != 1.0 and 2.0 / (3.0 + EPS) == 2.0 / 3.0
    q = ev.eval["precision"][0, :, 0, 0, 0]
    assert np.count_nonzero(ev.recThrs <= 0.5) == 51
    assert np.array_equal(q, np.array([p0] * 51 + [2.0 / 3.0] * 50))
    assert abs(q.mean() - (51 * p0 + 50 * (2.0 / 3.0)) / 101) < 1e-15
    assert ev.eval["recall"][0, 0, 0, 0] == 1.0
    assert np.array_equal(ev.eval["scores"][0, :, 0, 0, 0], [np.float64(np.float32(0.9))] * 51 + [np.float64(np.float32(0.7))] * 50)
    e = ev.evalImgs[0]
    assert e["dtIds"] == [0, 1, 2] and e["dtMatches"].tolist() == [[11, 0, 12]]


def test_crowd_ground_truth_matches_many_and_is_ignored():
    """A crowd region: IoU = inter / area_d (1 for a detection inside it), matched any number of times, and its matches
    are ignored; npig counts the non-crowd ground truth only."""
    crowd = box(20, 20, 0, 10, 0, 20)
    g = box(20, 20, 12, 20, 0, 8)
    d1, d2 = box(20, 20, 0, 4, 0, 4), box(20, 20, 5, 9, 5, 9)
    ev = run([(crowd, 1, 1, 200, 7), (g, 1, 0, 64, 8)], [(d1, 1, 0.9), (d2, 1, 0.8), (g, 1, 0.5)])
    e = ev.evalImgs[0]
    assert e["gtIds"] == [8, 7] and e["gtIgnore"].tolist() == [0, 1]            # non-ignored first
    assert e["dtMatches"].tolist() == [[7, 7, 8]]
    assert e["dtIgnore"].tolist() == [[True, True, False]]
    assert ev.eval["recall"][0, 0, 0, 0] == 1.0
    assert np.all(ev.eval["precision"][0, :, 0, 0, 0] == 1.0 / (1.0 + EPS))
    # crowd IoU itself: inter / area_d, so a detection twice the crowd's size still gets 0.5
    big = box(20, 20, 0, 20, 0, 20)
    assert sen.mask_iou([big], [crowd], [1])[0, 0] == 0.5
    assert sen.mask_iou([big], [crowd], [0])[0, 0] == 0.5
    assert sen.mask_iou([box(20, 20, 0, 10, 0, 10)], [crowd], [0])[0, 0] == 0.5
    assert sen.mask_iou([box(20, 20, 0, 10, 0, 10)], [crowd], [1])[0, 0] == 1.0


def test_equal_iou_later_ground_truth_wins():
    """The matching test is `ious < iou -> continue`, so among equal IoUs the later ground truth replaces the earlier."""
    a, b = box(10, 10, 0, 4, 0, 4), box(10, 10, 0, 4, 4, 8)
    d = box(10, 10, 0, 4, 2, 6)                                      # 8 px in each: IoU 8 / 24 with both
    ev = run([(a, 1, 0, 16, 1), (b, 1, 0, 16, 2)], [(d, 1, 0.9)], iou_thrs=(0.3,))
    assert ev.evalImgs[0]["dtMatches"].tolist() == [[2]]


def test_stop_at_first_ignored_ground_truth_once_matched():
    """A non-ignored ground truth at IoU 0.6 and an ignored one (area outside the range) at IoU 1: the non-ignored one is
    kept - the scan stops at the first ignored ground truth once a non-ignored one is matched."""
    g_ok = box(20, 20, 0, 10, 0, 10)
    d = box(20, 20, 0, 10, 0, 6)                                     # IoU 60 / 100 with g_ok
    g_ig = d.copy()
    ev = run([(g_ig, 1, 0, 5000, 1), (g_ok, 1, 0, 100, 2)], [(d, 1, 0.9)], area_rng=[[0, 1000]])
    e = ev.evalImgs[0]
    assert e["gtIds"] == [2, 1] and e["gtIgnore"].tolist() == [0, 1]
    assert e["dtMatches"].tolist() == [[2]] and e["dtIgnore"].tolist() == [[False]]
    # without the non-ignored one (already taken by a better detection) it falls through to the ignored one
    ev = run([(g_ig, 1, 0, 5000, 1), (g_ok, 1, 0, 100, 2)], [(g_ok, 1, 0.95), (d, 1, 0.9)], area_rng=[[0, 1000]])
    e = ev.evalImgs[0]
    assert e["dtMatches"].tolist() == [[2, 1]] and e["dtIgnore"].tolist() == [[False, True]]


def test_ground_truth_id_zero_counts_as_unmatched():
    """dtm holds the ground-truth id; accumulate's 'matched' is dtm != 0, so a match to id 0 is a false positive, and an
    unmatched-looking detection outside the area range is ignored."""
    g = box(10, 10, 0, 5, 0, 5)
    ev = run([(g, 1, 0, 25, 0)], [(g, 1, 0.9)])
    e = ev.evalImgs[0]
    assert e["dtMatches"].tolist() == [[0]] and e["dtIgnore"].tolist() == [[False]]
    assert ev.eval["recall"][0, 0, 0, 0] == 0.0
    assert np.all(ev.eval["precision"][0, :, 0, 0, 0] == 0.0)
    ev = run([(g, 1, 0, 25, 0)], [(g, 1, 0.9)], area_rng=[[0, 10]])     # det area 25 > 10, annotation area 25 too
    assert ev.evalImgs[0]["dtIgnore"].tolist() == [[True]]
    assert np.all(ev.eval["precision"][0, :, 0, 0, 0] == -1)           # the ground truth is ignored: npig == 0


def test_annotation_area_not_pixel_count_decides_ground_truth_ignore():
    g = box(10, 10, 0, 5, 0, 5)                                       # 25 pixels, annotated area 2000
    ev = run([(g, 1, 0, 2000, 3)], [(g, 1, 0.9)], area_rng=[[0, 1000]])
    e = ev.evalImgs[0]
    assert e["gtIgnore"].tolist() == [1]
    assert e["dtMatches"].tolist() == [[3]] and e["dtIgnore"].tolist() == [[True]]


def test_empty_category_no_ground_truth_and_no_detections():
    g = box(10, 10, 0, 5, 0, 5)
    # category 2: no ground truth and no detection anywhere -> -1; category 3: detections only -> npig == 0 -> -1;
    # category 4: a ground truth and no detection -> recall 0, precision 0
    ev = run([(g, 1, 0, 25, 1), (g, 4, 0, 25, 2)], [(g, 1, 0.9), (g, 3, 0.8)], cats=(1, 2, 3, 4))
    P, Rc = ev.eval["precision"], ev.eval["recall"]
    assert np.all(P[0, :, 1] == -1) and np.all(Rc[0, 1] == -1)
    assert np.all(P[0, :, 2] == -1) and np.all(Rc[0, 2] == -1)
    assert np.all(P[0, :, 3] == 0) and np.all(Rc[0, 3] == 0)
    assert np.all(ev.eval["scores"][0, :, 3] == 0)
    assert np.all(P[0, :, 0] == 1.0 / (1.0 + EPS))
    # (image, category) without ground truth or detection is absent from evalImgs
    assert ev.evalImgs[1] is None and ev.evalImgs[0] is not None


def test_threshold_one_compares_below_one_minus_1e10():
    g = box(10, 10, 0, 5, 0, 5)
    ev = run([(g, 1, 0, 25, 1)], [(g, 1, 0.9)], iou_thrs=(1.0,))
    assert ev.evalImgs[0]["dtMatches"].tolist() == [[1]]


def test_max_dets_prefixes_and_truncation_before_matching():
    """Matching happens once at maxDets[-1] = 2 on the two best detections; maxDet 1 takes the first of them per image,
    it does not match again."""
    g = box(10, 10, 0, 5, 0, 5)
    dbad = box(10, 10, 6, 10, 6, 10)
    ev = run([(g, 1, 0, 25, 1)], [(dbad, 1, 0.9), (g, 1, 0.8), (g, 1, 0.1)], max_dets=(1, 2))
    e = ev.evalImgs[0]
    assert e["dtIds"] == [0, 1] and e["dtMatches"].tolist() == [[0, 1]]
    assert ev.eval["recall"][0, 0, 0].tolist() == [0.0, 1.0]


def test_stable_order_of_equal_scores_across_images():
    """Equal scores: image order (ascending id), then rank in the image - here FP (image 1) before TP (image 2)."""
    g = box(10, 10, 0, 5, 0, 5)
    bad = box(10, 10, 6, 10, 6, 10)
    ev = run(None, None, img_ids=(2, 1), images={2: ([(g, 1, 0, 25, 5)], [(g, 1, 0.5)]), 1: ([], [(bad, 1, 0.5)])})
    q = ev.eval["precision"][0, :, 0, 0, 0]
    # FP first: tp = [0, 1], fp = [1, 1], pr = [0, 1 / (2 + eps)] = [0, 1/2]; TP first would give 1 / (1 + eps) everywhere
    assert np.all(q == 0.5)


def test_summarize_of_hand_case():
    g1, g2 = box(10, 10, 0, 4, 0, 4), box(10, 10, 6, 10, 6, 10)
    fp = box(10, 10, 0, 3, 6, 10)
    ev = run([(g1, 1, 0, 16, 11), (g2, 1, 0, 16, 12)], [(g1, 1, 0.9), (fp, 1, 0.8), (g2, 1, 0.7)], iou_thrs=None,
             area_rng=None, max_dets=(1, 10, 100))
    s = ev.summarize()
    assert s[3] != -1 and s[4] == -1 and s[5] == -1                   # small only (16-pixel objects)
    assert s[6] == 0.5 and s[8] == 1.0
