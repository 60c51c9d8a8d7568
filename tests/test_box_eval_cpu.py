"""Box evaluation (cim_amd.box_eval, csrc/box_eval.hip) without a GPU: the NumPy restatement (tests/golden/box_eval_np.py)
against the golden captured by running the reference's voc_eval / dis_eval (tests/golden/box_eval_voc.npz), hand-derived
bbIou cases, the text round trip, the C ABI's declarations and refusals, and the Python layer's argument checks."""
import os
import re

import numpy as np
import pytest
import torch

import box_eval_np as ben

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
BOX_ENTRIES = {"cim_box_image_ws_bytes", "cim_box_eval_image", "cim_voc_match", "cim_voc_ap_ws_bytes", "cim_voc_ap"}


def bits_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "box_eval_voc.npz")))


@pytest.fixture(scope="module")
def restated(golden):
    return ben.voc_dataset_np(golden)


# ---- the restatement against the reference's own results ------------------------------------------------------------------------
def test_restatement_rec_prec_ap07_corloc_equal_the_reference_bit_for_bit(golden, restated):
    assert np.array_equal(restated["cls_off"], golden["cls_off"])
    nan = np.isnan(golden["rec"])
    assert nan.any() and np.array_equal(np.isnan(restated["rec"]), nan)          # the class without ground truth: 0 / 0
    assert bits_equal(restated["rec"][~nan], golden["rec"][~nan])
    assert bits_equal(restated["prec"], golden["prec"])
    assert bits_equal(restated["ap07"], golden["ap07"])
    assert np.array_equal(restated["corloc"], golden["corloc"], equal_nan=True) and np.isnan(golden["corloc"]).sum() == 1
    assert bits_equal(restated["corloc"][~np.isnan(golden["corloc"])], golden["corloc"][~np.isnan(golden["corloc"])])
    assert (golden["ap07"][:3] > 0.1).all() and golden["ap07"][3] == 0 and golden["ap07"][4] == 0


def test_restatement_area_ap_within_the_summation_bound(golden, restated):
    """Two summation orders of n non-negative terms that sum to <= 1 differ by at most 2 (n + 1) 2^-53."""
    for k in range(len(golden["classes"])):
        a, b = golden["cls_off"][k], golden["cls_off"][k + 1]
        if np.isnan(golden["ap"][k]):
            assert np.isnan(restated["ap"][k]) and k == 3
            continue
        mrec = np.concatenate(([0.], golden["rec"][a:b], [1.]))
        n = np.count_nonzero(mrec[1:] != mrec[:-1])
        assert abs(restated["ap"][k] - golden["ap"][k]) <= 2 * (n + 1) * U, k


def test_golden_confidences_stay_distinct_after_the_text_round_trip(golden):
    for k in range(len(golden["classes"])):
        c = ben.text_round_trip(golden["dets"][golden["dt_cls"] == k])[1]
        assert len(np.unique(c)) == len(c)


# ---- bbIou by hand ---------------------------------------------------------------------------------------------------------------
def test_bb_iou_hand_cases():
    d = [[0, 0, 10, 10], [10, 0, 5, 5], [2, 2, 0, 4], [5, 5, 10, 10]]
    g = [[0, 0, 10, 10], [0, 0, 20, 20]]
    iou = ben.bb_iou(d, g, [0, 1])
    assert iou[0, 0] == 1.0 and iou[0, 1] == 1.0                         # crowd: i / da
    assert iou[1, 0] == 0.0                                              # touching: w == 0
    assert iou[1, 1] == 1.0 and iou[2, 0] == 0.0 and iou[2, 1] == 0.0    # zero area: w <= 0
    assert iou[3, 0] == 25.0 / 175.0 and iou[3, 1] == 1.0


def test_bbox_restatement_uses_box_area_for_the_area_rule():
    ev = ben.BoxEvalNp([1], [1], iou_thrs=[0.5], area_rng=[[0, 1e10], [0, 1024]], max_dets=(100,))
    ev.add_image(1, [[0, 0, 10, 10]], [1], [0], [100], [7], [[100, 100, 32, 32], [200, 200, 32.5, 32], [0, 0, 10, 10]], [1, 1, 1],
                 np.float32([0.9, 0.8, 0.7]))
    ev.evaluate()
    small = ev.evalImgs[1]
    assert list(small["dtIgnore"][0]) == [False, True, False] and list(small["dtMatches"][0]) == [0, 0, 7]


# ---- the text round trip -----------------------------------------------------------------------------------------------------------
def test_voc_text_round_trip_matches_python_formatting():
    from cim_amd import box_eval
    vals = np.float32([0.0005, 0.0015, 0.0025, 0.1235, 0.9995, 0.99949, 1.0, 3e-5, 0.5])
    coords = np.float32([0.05, 0.15, 0.25, 0.35, 1.45, 2.55, 10.65, 100.75, 7.85, 0.95, 1023.95, 0.0])
    dets = np.zeros((len(vals) * 3, 5), np.float32)
    dets[:, 4] = np.tile(vals, 3)
    dets[:, :4] = np.resize(coords, (len(dets), 4))
    boxes, conf = box_eval.voc_text_round_trip(dets)
    assert boxes.dtype == conf.dtype == np.float64
    for row, b, c in zip(dets, boxes, conf):
        line = "{:s} {:.3f} {:.1f} {:.1f} {:.1f} {:.1f}".format("x", float(row[4]), *(float(v) + 1 for v in row[:4]))
        want = [float(z) for z in line.split(" ")[1:]]
        assert c == want[0] and list(b) == want[1:]
    assert box_eval.voc_text_round_trip(np.float32([[0.25, 0, 0, 0, 0.0005]]))[0][0, 0] == 1.2      # 1.25 -> '1.2' (half to even)
    b2, c2 = ben.text_round_trip(dets)
    assert np.array_equal(b2, boxes) and np.array_equal(c2, conf)


def test_xyxy_to_xywh_in_fp64_from_fp32_values():
    from cim_amd import box_eval
    b = np.float32([[0.1, 0.2, 16777216.0, 5.3]])
    got = box_eval.xyxy_to_xywh64(b)
    assert got.dtype == np.float64 and got[0, 2] == 16777216.0 - float(np.float32(0.1)) + 1 and got[0, 0] == float(np.float32(0.1))


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_box_entries():
    from cim_amd import _lib, build
    header = open(os.path.join(REPO, "include", "cim_hip.h")).read()
    declared = set(re.findall(r"\b(cim_(?:box|voc)_[a-z0-9_]+)\s*\(", header))
    assert declared == BOX_ENTRIES and declared <= set(_lib.SIGNATURES)
    assert "#define CIM_VOC_MAX_RUN 256" in header
    build.build()
    lib = _lib.load()
    assert lib.cim_abi_version() == 16
    for name in declared:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]


def test_shapes_are_refused_before_any_launch():
    from cim_amd import _lib, build
    build.build()
    lib = _lib.load()
    err = lambda: lib.cim_last_error().decode()
    assert _lib.call("cim_box_image_ws_bytes", 100, 20, 2000) >= 8 * 100 + 8 * 2000
    for d, g, p in ((-1, 3, 0), (10, 1025, 0), (10, 10, 101), (10, 10, -1)):
        assert _lib.call("cim_box_image_ws_bytes", d, g, p) == -1 and "1024 ground truths" in err()
    assert _lib.call("cim_voc_ap_ws_bytes", 1000) >= 16000
    assert _lib.call("cim_voc_ap_ws_bytes", -1) == -1 and _lib.call("cim_voc_ap_ws_bytes", 1 << 31) == -1
    z = [None] * 4
    assert lib.cim_box_eval_image(None, 10, None, 2000, None, None, 1, 0, 0, 0, None, None, None, 1, None, 1, None, None, None) == -1
    assert "1024 ground truths" in err()
    assert lib.cim_box_eval_image(None, 10, None, 10, None, None, 1, 0, 0, 0, None, None, None, 17, None, 1, None, None, None) == -1
    assert lib.cim_voc_match(None, None, 5, None, None, 0, None, 1, 0.5, 2, *z, None) == -1 and "mode" in err()
    assert lib.cim_voc_match(None, None, -1, None, None, 0, None, 1, 0.5, 0, *z, None) == -1
    assert lib.cim_voc_match(None, None, 5, None, None, 0, None, 1, 0.5, 0, *z, None) == -1 and "bad argument" in err()
    assert lib.cim_voc_ap(None, None, None, 5, None, None, 0, None, 1, None, None, 0, None, None, None, None, None, None) == -1
    assert "K >= 1" in err()
    assert lib.cim_voc_ap(None, None, None, 5, None, None, 1, None, 1, None, None, 64, None, None, None, None, None, None) == -1
    assert lib.cim_voc_ap(None, None, None, 5, None, None, 1, None, 1, None, None, 0, None, None, None, None, None, None) == -1
    assert "bad argument" in err()


def test_matcher_has_one_copy():
    """evaluateImg's matcher, the score sort and the merge round live in csrc/eval_match.h; neither evaluator keeps its own."""
    csrc = os.path.join(REPO, "cim_amd", "csrc")
    shared = open(os.path.join(csrc, "eval_match.h")).read()
    assert shared.count("void segm_match_kernel(") == 1 and shared.count("void segm_merge_kernel(") == 1
    for name in ("segm_eval.hip", "box_eval.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "eval_match.h"' in src and "void segm_match_kernel(" not in src and "void segm_merge_kernel(" not in src
        assert "segm_match_kernel<" in src and "segm_merge_kernel<" in src


# ---- the Python layer's checks ---------------------------------------------------------------------------------------------------
def test_box_evaluator_rejects_bad_arguments():
    from cim_amd import _lib, box_eval
    ev = box_eval.BoxEvaluator([1], [1], device="cuda:0")
    one = np.float32([[0, 0, 5, 5]])
    with pytest.raises(_lib.CimHipError):                                # CPU tensors: no CPU fallback
        ev.add_image(1, [], [], [], [], [], torch.zeros(1, 4), [1], np.float32([0.5]))
    with pytest.raises(_lib.CimHipError):
        ev.add_image(1, [], [], [], [], [], one, [1], torch.zeros(1))
    with pytest.raises(TypeError):
        ev.add_image(1, [], [], [], [], [], one.astype(np.float64), [1], np.float32([0.5]))
    with pytest.raises(TypeError):
        ev.add_image(1, [], [], [], [], [], one, [1], np.float64([0.5]))
    with pytest.raises(ValueError, match="NaN"):
        ev.add_image(1, [], [], [], [], [], one, [1], np.float32([np.nan]))
    with pytest.raises(ValueError, match="1 detections, 2 scores"):
        ev.add_image(1, [], [], [], [], [], one, [1], np.float32([0.5, 0.4]))
    with pytest.raises(ValueError, match="different lengths"):
        ev.add_image(1, [[0, 0, 1, 1]], [1], [0, 0], [1], [1], np.zeros((0, 4), np.float32), [], np.zeros(0, np.float32))
    with pytest.raises(ValueError, match="1 ground truths, 2 boxes"):
        ev.add_image(1, [[0, 0, 1, 1], [0, 0, 2, 2]], [1], [0], [1], [1], np.zeros((0, 4), np.float32), [], np.zeros(0, np.float32))
    with pytest.raises(ValueError, match="not among"):
        ev.add_image(2, [], [], [], [], [], np.zeros((0, 4), np.float32), [], np.zeros(0, np.float32))
    assert not ev._images                                                # nothing was registered by a refused call


def test_voc_evaluator_rejects_bad_arguments():
    from cim_amd import _lib, box_eval
    with pytest.raises(_lib.CimHipError):
        box_eval.VocBoxEvaluator(["a"], device="cpu")
    ev = box_eval.VocBoxEvaluator(["a", "b"], device="cuda:0")
    det = np.float32([[0, 0, 5, 5, 0.5]])
    with pytest.raises(_lib.CimHipError):
        ev.add_image("i", [], [], [], [torch.zeros(1, 5), []])
    with pytest.raises(TypeError):
        ev.add_image("i", [], [], [], [det.astype(np.float64), []])
    with pytest.raises(ValueError, match="NaN"):
        ev.add_image("i", [], [], [], [np.float32([[0, 0, 5, 5, np.nan]]), []])
    with pytest.raises(ValueError, match="non-finite"):
        ev.add_image("i", [], [], [], [np.float32([[0, np.inf, 5, 5, 0.5]]), []])
    with pytest.raises(ValueError, match="different lengths"):
        ev.add_image("i", [[1, 1, 5, 5]], [0, 1], [0], [det, []])
    with pytest.raises(ValueError, match="class outside"):
        ev.add_image("i", [[1, 1, 5, 5]], [2], [0], [det, []])
    with pytest.raises(ValueError, match="2 classes, detections of 1"):
        ev.add_image("i", [], [], [], [det])
    assert not ev._index
    ev.add_image("i", [[1, 1, 5, 5]], [0], [0], [det, None])
    with pytest.raises(ValueError, match="added twice"):
        ev.add_image("i", [], [], [], [[], []])
    for fn, args in ((box_eval.voc_match, (torch.zeros(1, 4, dtype=torch.float64),) * 5),
                     (box_eval.voc_ap, (torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.uint8),
                                        torch.zeros(1, dtype=torch.uint8), [0, 1], [1.0], ([0], [1], [0])))):
        with pytest.raises(_lib.CimHipError):
            fn(*args)


def test_voc_runs_and_their_merge_schedule():
    from cim_amd import box_eval
    s, n, c = box_eval.voc_runs([0, 300, 305], [300, 5, 0], [0, 1, 1])
    assert s.tolist() == [0, 256, 300] and n.tolist() == [256, 44, 5] and c.tolist() == [0, 0, 1]
    rounds = box_eval.merge_rounds(s, n, c)
    assert [r.tolist() for r in rounds] == [[[0, 256, 44], [300, 5, 0]]]


def test_voc_annotation_and_results_readers(golden, tmp_path):
    from cim_amd.datasets import voc_eval
    detpath, annopath, imageset = ben.write_voc_files(str(tmp_path), golden)
    names, recs = voc_eval.load_annotations(annopath, imageset, str(tmp_path / "cache"))
    assert names == [str(n) for n in golden["imagenames"]]
    again = voc_eval.load_annotations(annopath, imageset, str(tmp_path / "cache"))[1]          # (from the cache file)
    assert again == recs and os.path.isfile(str(tmp_path / "cache" / "val_annots_cim.pkl"))
    for i, name in enumerate(names):
        gi = np.flatnonzero(golden["gt_img"] == i)
        assert [o["bbox"] for o in recs[name]] == golden["gt_box"][gi].tolist()
        assert [o["difficult"] for o in recs[name]] == golden["gt_diff"][gi].tolist()
        assert [o["name"] for o in recs[name]] == [str(golden["classes"][k]) for k in golden["gt_cls"][gi]]
    k = 1
    ids, conf, boxes = voc_eval.read_detections(detpath.format(str(golden["classes"][k])))
    sel = golden["dt_cls"] == k
    b, c = ben.text_round_trip(golden["dets"][sel])
    assert np.array_equal(boxes, b) and np.array_equal(conf, c) and ids == [names[i] for i in golden["dt_img"][sel]]
    assert voc_eval.read_detections(detpath.format("nodet"))[2].shape == (0, 4)


def test_install_as_lib_routes_the_voc_evaluators():
    import cim_amd
    for name in ("voc_eval", "dis_eval"):
        assert cim_amd.ALIASES["datasets." + name] == "cim_amd.datasets." + name
        spec = cim_amd._finder.find_spec("datasets." + name)
        mod = spec.loader.create_module(spec)
        assert mod.__name__ == "cim_amd.datasets." + name and callable(getattr(mod, name))


def test_add_parsed_checks_what_add_image_checks():
    from cim_amd import box_eval
    ev = box_eval.VocBoxEvaluator(["a", "b"], device="cuda:0", text_round_trip=False)
    box, conf = np.float64([[1, 1, 5, 5]]), np.float64([0.5])
    for gt, dets, msg in ((([[1, 1, 5, 5]], [0, 1], [0]), [], "different lengths"), (([[1, 1, 5, 5]], [2], [0]), [], "class outside"),
                          (([], [], []), [(0, box, np.float64([np.nan]))], "NaN"), (([], [], []), [(0, box * np.inf, conf)], "non-finite"),
                          (([], [], []), [(0, box, np.float64([0.5, 0.4]))], "1 boxes, 2 confidences"),
                          (([], [], []), [(0, box, conf), (0, box, conf)], "distinct"), (([], [], []), [(2, box, conf)], "distinct")):
        with pytest.raises(ValueError, match=msg):
            ev.add_parsed("i", gt[0], gt[1], gt[2], dets)
    assert not ev._index and not any(ev._gt) and not any(ev._dt)
