"""-m gpu: cim_amd.proposal_prep (csrc/proposal_prep.hip) bit for bit against the goldens captured from the
reference (tests/golden/proposal_prep_*.npz) and against the NumPy restatement (tests/golden/proposal_prep_np.py) at the
benchmark's sizes and at ragged ones; the packed words and maps against cim_amd.mask_iou; the empty-mask error; two host
threads on two streams; a training forward fed from roidb_fields()."""
import os
import threading

import numpy as np
import pytest
import torch

import proposal_prep_np as ppn

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from cim_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def load_golden(name):
    d = np.load(os.path.join(GOLDEN, "proposal_prep_%s.npz" % name))
    g = {k: d[k] for k in d.files}
    g["masks_full"] = ppn.unpack_bits(g["mask_bits"], g["mask_shape"])
    return g


def check_prepare(prep, masks, size=7):
    boxes, small, area = ppn.boxes_and_small(masks, size)
    assert prep.boxes.dtype == torch.int32 and prep.masks.dtype == torch.bool and prep.area.dtype == torch.int32
    assert prep.packed.dtype == torch.int64 and tuple(prep.masks.shape) == (masks.shape[0], size, size)
    np.testing.assert_array_equal(prep.boxes.cpu().numpy(), boxes)
    np.testing.assert_array_equal(prep.masks.cpu().numpy(), small)
    np.testing.assert_array_equal(prep.area.cpu().numpy(), area)


def random_points(masks, p, num_classes, rng):
    """p points: mostly inside some proposal (so that they select masks), some anywhere."""
    n, h, w = masks.shape
    rows, cols = [], []
    for j in range(p):
        if j % 4 == 3:
            rows.append(int(rng.randint(0, h))), cols.append(int(rng.randint(0, w)))
        else:
            ys, xs = np.nonzero(masks[rng.randint(0, n)])
            k = rng.randint(0, ys.size)
            rows.append(int(ys[k])), cols.append(int(xs[k]))
    return rows, cols, [int(c) for c in rng.randint(0, num_classes, size=p)]


@pytest.mark.parametrize("name", ("voc", "coco", "nopoints"))
@pytest.mark.parametrize("dtype", (torch.bool, torch.uint8))
def test_device_equals_the_reference_goldens(dev, name, dtype):
    from cim_amd import proposal_prep as pp
    g = load_golden(name)
    prep = pp.prepare(torch.from_numpy(g["masks_full"]).to(dev).to(dtype))
    np.testing.assert_array_equal(prep.boxes.cpu().numpy(), g["boxes"].astype(np.int32))
    np.testing.assert_array_equal(prep.masks.cpu().numpy(), g["small"])
    np.testing.assert_array_equal(prep.area.cpu().numpy(), g["masks_full"].reshape(len(g["boxes"]), -1).sum(1))
    rows, cols, classes = pp.points_to_pixels(g["points"])
    mat = pp.assign_clusters(prep, rows, cols, classes, 20)
    assert mat.dtype == torch.float32 and tuple(mat.shape) == g["mat"].shape
    np.testing.assert_array_equal(mat.cpu().numpy(), g["mat"])
    fields = prep.roidb_fields(mat)
    assert fields["boxes"].dtype == np.uint16 and fields["masks"].dtype == bool and fields["mat"].dtype == np.float32
    np.testing.assert_array_equal(fields["boxes"], g["boxes"])
    np.testing.assert_array_equal(fields["masks"], g["small"])
    np.testing.assert_array_equal(fields["mat"], g["mat"])


def test_peaks_reach_the_same_matrix_as_points(dev):
    """AGPL_label_assign.py:154-180 is the point form's statements behind [:, x, y] indexing: peaks on the 112 grid that land on
    the golden's pixels give the golden's matrix."""
    from cim_amd import proposal_prep as pp
    g = load_golden("voc")
    h, w = g["masks_full"].shape[1:]
    rows, cols, classes = pp.points_to_pixels(g["points"])
    peaks = [[0, c, -(-r * 112 // h), -(-x * 112 // w)] for r, x, c in zip(rows, cols, classes)]      # ceil: int(a H / 112) == r
    assert pp.peaks_to_pixels(peaks, h, w) == (rows, cols, classes)
    prep = pp.prepare(torch.from_numpy(g["masks_full"]).to(dev))
    mat = pp.assign_clusters(prep, *pp.peaks_to_pixels(peaks, h, w), 20)
    np.testing.assert_array_equal(mat.cpu().numpy(), g["mat"])


@pytest.mark.parametrize("config,p", (("resnet50_voc", 6), ("resnet50_coco2017", 12)))
def test_device_equals_restatement_at_benchmark_sizes(dev, config, p):
    """1000 x 375 x 500 with 20 classes and 6 points; 2000 x 480 x 640 with 80 classes and 12 points."""
    from cim_amd import mask_iou, proposal_prep as pp, synthetic
    inp = synthetic.make_image_inputs(config, seed=3, with_image=False)
    masks = inp["full_masks"]
    c = synthetic.CONFIGS[config]["classes"]
    assert masks.shape == {"resnet50_voc": (1000, 375, 500), "resnet50_coco2017": (2000, 480, 640)}[config]
    dm = torch.from_numpy(masks).to(dev)
    prep = pp.prepare(dm)
    check_prepare(prep, masks)
    # the packed words and the maps are those of the existing entry points
    assert torch.equal(prep.packed, mask_iou.pack_masks(dm))
    iou, asy = prep.maps()
    riou, rasy = mask_iou.mask_iou_maps(dm)
    assert iou.dtype == torch.float16 and torch.equal(iou, riou) and torch.equal(asy, rasy)
    rows, cols, classes = random_points(masks, p, c, np.random.RandomState(11))
    mat = pp.assign_clusters(prep, rows, cols, classes, c)
    want = ppn.assign_clusters(masks, rows, cols, classes, c)
    assert tuple(mat.shape) == (masks.shape[0], c + 1)
    np.testing.assert_array_equal(mat.cpu().numpy(), want)
    assert (want[:, 1:] != 0).any() and (want[:, 0] != 0).any(), "the case assigns nothing: it would test nothing"


@pytest.mark.parametrize("n,h,w,size,p,c", ((1, 5, 7, 7, 2, 3), (37, 33, 45, 7, 5, 20), (130, 61, 67, 16, 9, 80), (64, 1, 300, 1, 3, 4),
                                            (65, 300, 1, 3, 3, 4), (200, 50, 40, 7, 0, 20), (90, 23, 29, 7, 256, 80)))
def test_device_equals_restatement_at_ragged_sizes(dev, n, h, w, size, p, c):
    """H W not a multiple of 64 nor of 4, N = 1, N not a multiple of 64, one-row and one-column images, P = 0 and the cap."""
    from cim_amd import mask_iou, proposal_prep as pp, synthetic
    rng = np.random.RandomState(1000 * n + h)
    if min(h, w) >= 16:
        masks, _ = synthetic.make_masks(n, h, w, rng, min_side=2)
    else:
        masks = rng.rand(n, h, w) < 0.4
        masks[np.arange(n), rng.randint(0, h, size=n), rng.randint(0, w, size=n)] = True
    dm = torch.from_numpy(masks).to(dev)
    prep = pp.prepare(dm, mask_size=size)
    check_prepare(prep, masks, size)
    assert torch.equal(prep.packed, mask_iou.pack_masks(dm))
    rows, cols, classes = random_points(masks, p, c, rng)
    mat = pp.assign_clusters(prep, rows, cols, classes, c)
    np.testing.assert_array_equal(mat.cpu().numpy(), ppn.assign_clusters(masks, rows, cols, classes, c))
    # a non-contiguous view and an integer dtype give the same
    wide = torch.zeros((n, h, w + 3), dtype=torch.int32, device=dev)
    wide[:, :, :w] = dm.to(torch.int32) * 7
    again = pp.prepare(wide[:, :, :w], mask_size=size)
    assert torch.equal(again.packed, prep.packed) and torch.equal(again.boxes, prep.boxes) and torch.equal(again.masks, prep.masks)


def test_empty_mask_raises_naming_the_first_such_proposal(dev):
    from cim_amd import proposal_prep as pp
    masks = np.zeros((70, 20, 30), dtype=bool)
    masks[:, 3:9, 4:20] = True
    masks[41] = False
    masks[66] = False
    with pytest.raises(ValueError, match="proposal 41 has no pixel"):
        pp.prepare(torch.from_numpy(masks).to(dev))
    with pytest.raises(ValueError, match="proposal 41 has no pixel"):
        ppn.boxes_and_small(masks)
    masks[41, 19, 29] = True
    with pytest.raises(ValueError, match="proposal 66 has no pixel"):
        pp.prepare(torch.from_numpy(masks).to(dev))
    masks[66, 0, 0] = True
    prep = pp.prepare(torch.from_numpy(masks).to(dev))
    assert prep.boxes[41].tolist() == [29, 19, 30, 20] and prep.boxes[66].tolist() == [0, 0, 1, 1]


def test_device_refusals(dev):
    from cim_amd import proposal_prep as pp
    ok = torch.ones((3, 8, 8), dtype=torch.bool, device=dev)
    for size in (0, 17):
        with pytest.raises(ValueError, match="mask_size"):
            pp.prepare(ok, mask_size=size)
    with pytest.raises(ValueError):
        pp.prepare(ok[:0])
    with pytest.raises(ValueError):
        pp.prepare(ok[0])
    prep = pp.prepare(ok)
    with pytest.raises(ValueError, match="outside"):
        pp.assign_clusters(prep, [8], [0], [0], 20)
    with pytest.raises(ValueError, match="class 20"):
        pp.assign_clusters(prep, [0], [0], [20], 20)


def test_two_threads_two_streams(dev):
    """As tests/test_gpu_reentrant.py does for the rest of the library: every call owns its workspace, nothing is kept between
    calls, so two host threads on their own streams get the single-threaded results."""
    from cim_amd import proposal_prep as pp, synthetic
    cases = []
    for k, (n, h, w, p, c) in enumerate(((300, 120, 160, 6, 20), (450, 97, 131, 9, 80))):
        rng = np.random.RandomState(50 + k)
        masks, _ = synthetic.make_masks(n, h, w, rng, min_side=4)
        rows, cols, classes = random_points(masks, p, c, rng)
        boxes, small, _ = ppn.boxes_and_small(masks)
        cases.append((torch.from_numpy(masks).to(dev), rows, cols, classes, c, boxes, small,
                      ppn.assign_clusters(masks, rows, cols, classes, c)))
    torch.cuda.synchronize()
    errors = []

    def worker(k):
        try:
            dm, rows, cols, classes, c, boxes, small, want = cases[k]
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                for it in range(25):
                    prep = pp.prepare(dm)
                    mat = pp.assign_clusters(prep, rows, cols, classes, c)
                    iou, asy = prep.maps()
                    stream.synchronize()
                    np.testing.assert_array_equal(prep.boxes.cpu().numpy(), boxes, err_msg="thread %d round %d" % (k, it))
                    np.testing.assert_array_equal(prep.masks.cpu().numpy(), small)
                    np.testing.assert_array_equal(mat.cpu().numpy(), want)
                    assert float(iou.diagonal().min()) == 1.0 and float(asy.diagonal().min()) == 1.0
        except BaseException as e:                                    # noqa: BLE001 - reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_training_forward_fed_from_roidb_fields(dev):
    """prep.roidb_fields() drops into a roidb entry of get_minibatch; the step's losses equal those of an entry filled from the
    NumPy restatement's arrays."""
    from cim_amd import proposal_prep as pp, synthetic
    from cim_amd.core.config import cfg
    from cim_amd.core.presets import apply_preset
    from cim_amd.modeling.model_builder import Generalized_RCNN
    from cim_amd.roi_data import get_minibatch
    apply_preset("resnet50_voc")
    cfg.TRAIN.SCALES = (128, 160)
    rng = np.random.RandomState(7)
    h, w, n = 75, 100, 36
    im = rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    full_masks, _ = synthetic.make_masks(n, h, w, rng, min_side=8)
    labels = np.zeros(20, np.float32)
    labels[[3, 11]] = 1
    rows, cols, classes = random_points(full_masks, 3, 20, rng)
    classes = [3, 11, 3]
    dm = torch.from_numpy(full_masks).to(dev)
    prep = pp.prepare(dm)
    fields = prep.roidb_fields(pp.assign_clusters(prep, rows, cols, classes, 20))
    iou, asy = prep.maps()
    rb, rs, _ = ppn.boxes_and_small(full_masks)
    ref_fields = dict(boxes=rb.astype(np.uint16), masks=rs, mat=ppn.assign_clusters(full_masks, rows, cols, classes, 20))
    assert (ref_fields["mat"] != 0).any()
    losses = []
    for f in (fields, ref_fields):
        entry = dict(image=im, flipped=False, gt_classes=labels, path="/x/img.jpg")
        entry.update(f)
        np.random.seed(5)
        blobs, ok = get_minibatch([entry], 20, "ToTensor", device=dev)
        assert ok and tuple(blobs["masks"].shape) == (n, 7, 7) and tuple(blobs["mat"].shape) == (n, 21)
        torch.manual_seed(0)
        model = Generalized_RCNN().to(dev).train()
        out = model(data=blobs["data"], rois=blobs["rois"].unsqueeze(0), masks=blobs["masks"].unsqueeze(0),
                    labels=blobs["labels"].unsqueeze(0), gtrois=blobs["gtrois"], mat=blobs["mat"].unsqueeze(0),
                    index=blobs["index"].unsqueeze(0), iou_map=iou, asy_iou_map=asy)
        total = sum(v.sum() for v in out["losses"].values())
        total.backward()
        assert torch.isfinite(total)
        losses.append({k: float(v.detach().sum()) for k, v in out["losses"].items()})
    assert losses[0] == losses[1], losses
