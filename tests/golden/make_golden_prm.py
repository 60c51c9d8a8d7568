#!/usr/bin/env python3
"""Capture the PRM goldens by RUNNING THE REFERENCE on the CPU (its checkout: _ref_shims.REF_ROOT).

    python tests/golden/make_golden_prm.py      # rewrites tests/golden/prm_{peaks,net,e2e}.npz, byte-identically

Runs the reference's own lib/prm/prm_modules.py `PeakStimulation`, lib/prm/prm_model_gt.py `FC_ResNet` +
`PeakResponseMapping(...).inference()` (its peak back-propagation included: that is what the reference does) and
tools/pre/AGPL_label_assign.py `assign_voc2012` over seeded .mat / image files in a temporary ./data tree.  Nothing of the
reference is written into this repository.  Stubs, all in this file, stand in for the packages prm_model_gt.py imports and this
host lacks (cv2, mmcv, matplotlib, skimage, pycocotools, tqdm, torchvision): torchvision.models.resnet50 is a plain-torch
ResNet-50 of `width` 16 written here, torchvision.transforms the four transforms of prm_configs.open_transform on Pillow.
Weights are regenerated from a seed on both sides (prm_cases.seeded_weights), never stored.

Three files:
  prm_peaks  the crafted exact maps of prm_cases.crafted() through the reference's forward (an exact pass-through module as the
             backbone, sub_pixel_locating_factor 1): all peaks, the valid peaks, their scores, the AGPL order.
  prm_net    the thin network on two 64 x 96 images, one at a time (the reference is fixed at batch 1): class response maps in
             fp32 and float64, valid peaks / scores / order for label classes chosen from the maps (the two strongest and the
             weakest class), the state_dict key list.
  prm_e2e    three 448 x 448 inputs through assign_voc2012: several classes, the fallback alone, one class with several
             clusters; the decoded images, the proposal masks, peaks, scores and the final `mat`.
Condition on the network cases: the device's up-sampled maps differ from ATen's in the last bits and its class response maps by
summation order, so every decisive comparison (pixel against its eight neighbours, local maximum against the median, value
against the threshold, adjacent scores) must hold with a margin of 100 x the bound on the maps (4 x max |fp32 - float64|); a seed
at which one does not is skipped.  The classifier's gain is set per case so that the largest response is about 30.  The margins are recorded in the files."""
import copy
import importlib
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import scipy.io
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_shims  # noqa: E402
import prm_cases  # noqa: E402
import prm_np  # noqa: E402
import proposal_prep_np as ppn  # noqa: E402
from cim_amd import synthetic  # noqa: E402
from make_golden_proposal_prep import FakeCOCO, save_npz  # noqa: E402

f32 = np.float32
FACTOR = 8
MARGIN = 100.0
IDS = (2008000011, 2008000012, 2008000013)


# ---- a plain-torch ResNet-50 with torchvision's attribute names (the `resnet50` the reference wraps) ---------------------------
class _Block(nn.Module):
    def __init__(self, cin, planes, stride, down):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, 4 * planes, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(4 * planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = down

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        y = self.relu(self.bn1(self.conv1(x)))
        y = self.relu(self.bn2(self.conv2(y)))
        return self.relu(self.bn3(self.conv3(y)) + idt)


class PlainResNet50(nn.Module):
    def __init__(self, width=prm_cases.WIDTH):
        super().__init__()
        w = width
        self.conv1 = nn.Conv2d(3, w, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(w)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        cin = w
        for i, (planes, blocks, stride) in enumerate(((w, 3, 1), (2 * w, 4, 2), (4 * w, 6, 2), (8 * w, 3, 2))):
            layers = []
            for j in range(blocks):
                s = stride if j == 0 else 1
                down = None
                if j == 0:
                    down = nn.Sequential(nn.Conv2d(cin, 4 * planes, 1, s, bias=False), nn.BatchNorm2d(4 * planes))
                layers.append(_Block(cin, planes, s, down))
                cin = 4 * planes
            setattr(self, "layer%d" % (i + 1), nn.Sequential(*layers))


class PassThrough(nn.Module):
    """An exact backbone for the crafted maps: x * 1 (every float, -0.0 and inf included, comes back bit for bit)."""

    def forward(self, x):
        return x * 1


# ---- stubs -------------------------------------------------------------------------------------------------------------------
def _missing(name):
    try:
        importlib.import_module(name)
        return False
    except ImportError:
        return True


class _Compose(object):
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, x):
        for t in self.ts:
            x = t(x)
        return x


class _Resize(object):
    def __init__(self, size):
        self.size = size

    def __call__(self, img):
        from PIL import Image
        return img.resize((self.size[1], self.size[0]), Image.BILINEAR)


class _ToTensor(object):
    def __call__(self, img):
        a = torch.from_numpy(np.array(img, dtype=np.uint8)).permute(2, 0, 1).contiguous()
        return a.to(torch.float32).div(255)


class _Normalize(object):
    def __init__(self, mean, std):
        self.mean, self.std = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)

    def __call__(self, t):
        return t.clone().sub_(self.mean[:, None, None]).div_(self.std[:, None, None])


class _Flip(object):
    def __init__(self, p):
        pass


def install():
    _ref_shims.install(resnet50_factory=lambda pretrained=True: PlainResNet50())
    tr = sys.modules["torchvision.transforms"]
    tr.Compose, tr.Resize, tr.ToTensor, tr.Normalize, tr.RandomHorizontalFlip = _Compose, _Resize, _ToTensor, _Normalize, _Flip
    sys.modules["torchvision"].transforms = tr
    if _missing("cv2"):
        _ref_shims._module("cv2")
    if _missing("matplotlib"):
        m = _ref_shims._module("matplotlib")
        m.pyplot = _ref_shims._module("matplotlib.pyplot")
    if _missing("skimage"):
        m = _ref_shims._module("skimage")
        m.segmentation = _ref_shims._module("skimage.segmentation", mark_boundaries=None)
    if _missing("tqdm"):
        _ref_shims._module("tqdm", tqdm=lambda it, *a, **k: it)
    pc = _ref_shims._module("pycocotools")
    pc.coco = _ref_shims._module("pycocotools.coco", COCO=FakeCOCO)
    pc.mask = _ref_shims._module("pycocotools.mask")
    lib = types.ModuleType("lib")                                # lib/ has no __init__.py: a namespace package
    lib.__path__ = [os.path.join(_ref_shims.REF_ROOT, "lib")]
    sys.modules["lib"] = lib
    if not hasattr(np, "bool"):
        np.bool = bool
    sys.path.insert(0, os.path.join(_ref_shims.REF_ROOT, "tools", "pre"))
    cwd = os.getcwd()
    os.chdir(_ref_shims.REF_ROOT)                                # prm_configs.py loads lib/prm/cls_labels.npy relative to it
    try:
        gt = importlib.import_module("lib.prm.prm_model_gt")
        importlib.import_module("lib.prm.prm_configs")
    finally:
        os.chdir(cwd)
    return gt


# ---- the reference on given inputs -----------------------------------------------------------------------------------------
def ref_forward(model, x, labels, threshold):
    """model(x, lables, peak_threshold) of an .inference() model -> (all peaks [n,4], valid [P,4] as found, scores [P])."""
    out = model(x.clone(), torch.tensor(labels), class_threshold=0, peak_threshold=threshold)
    assert out is not None
    _, up, valid, prms, score = out
    assert len(prms) == valid.shape[0] == score.shape[0]         # what AGPL_label_assign.py:155 loops over
    return up.detach().numpy(), valid.numpy().astype(np.int64), score.numpy().astype(f32)


def agpl_order(score):
    return score.argsort()                                       # AGPL_label_assign.py:148


def crafted_goldens(gt):
    mods = importlib.import_module("lib.prm.prm_modules")
    model = gt.peak_response_mapping(backbone=PassThrough(), sub_pixel_locating_factor=1).inference()
    out = {}
    for name, case in prm_cases.crafted().items():
        ncls = max(case["maps"]) + 1
        shape = next(iter(case["maps"].values())).shape
        x = np.zeros((1, ncls) + shape, dtype=f32)
        for c, m in case["maps"].items():
            x[0, c] = m
        xt = torch.from_numpy(x)
        allp = mods.peak_stimulation(xt, return_aggregation=False, win_size=3, peak_filter=model.peak_filter).numpy()
        allp = allp[np.isin(allp[:, 1], case["labels"])]
        _, valid, score = ref_forward(model, xt, case["labels"], case["threshold"])
        order = agpl_order(score)
        if len(score) > 16:
            assert len(set(score.tolist())) == len(score)        # beyond 16 entries NumPy's introsort leaves ties unspecified
        out[name + "__all"] = allp[:, 1:]
        out[name + "__valid"] = valid[:, 1:]
        out[name + "__scores"] = score
        out[name + "__order"] = order.astype(np.int64)
        # the restatement on the same exact maps
        res = prm_np.image_points([case["maps"][c] for c in case["labels"]], case["labels"], shape[0], shape[1], case["threshold"])
        assert res["count"] == len(score), name
        if not res["status"]:
            got = np.stack([res["classes"], res["ys"], res["xs"]], 1)
            assert np.array_equal(got, valid[order, 1:]) and np.array_equal(res["scores"], score[order]), name
        for c in case["labels"]:
            _, npk, _, _ = prm_np.pair_peaks(case["maps"][c], case["threshold"])
            assert npk == int(np.sum(allp[:, 1] == c)), name
    assert np.array_equal(out["constant__all"], [[0, 0, 0]]) and np.array_equal(out["plateau__valid"], [[0, 0, 1]])
    assert out["at_threshold__scores"].size == 1 and out["many_257__scores"].size == 257
    assert np.array_equal(out["none_above__valid"], [[0, 0, 2]])
    return out


def build_reference(gt, seed, gain):
    backbone = gt.FC_ResNet(PlainResNet50(), prm_cases.NUM_CLASSES)
    model = gt.peak_response_mapping(backbone=backbone, sub_pixel_locating_factor=FACTOR)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in prm_cases.seeded_weights(shapes, seed, gain).items()}
    model.load_state_dict(sd)
    return model, list(shapes)


def calibrated(gt, seed, x, target=30.0):
    """The reference model with the classifier's gain set so that the largest |response| is about `target` (three digits)."""
    model, _ = build_reference(gt, seed, 1.0)
    gain = float("%.3g" % (target / float(np.abs(crms(model, x)[0]).max())))
    model, keys = build_reference(gt, seed, gain)
    return model, keys, gain


def crms(model, x):
    """The backbone's output in fp32 and in float64 (the same weights widened)."""
    model.eval()
    with torch.no_grad():
        c32 = model[0](x).numpy()
        c64 = copy.deepcopy(model[0]).double()(x.double()).numpy()
    return c32, c64


def choose_labels(c32):
    """The two strongest classes and the weakest one, ascending (torch.unique's order)."""
    peak = c32.reshape(c32.shape[0], -1).max(1)
    rank = np.argsort(peak)
    return sorted(int(c) for c in (rank[-1], rank[-2], rank[0]))


def margins(c32, c64, labels, threshold):
    """None if a decisive comparison of the restatement on this image's maps is closer than MARGIN x the bound; else the record.
    Decisive are the comparisons of the peaks that reach the output - those whose value could pass the threshold, or the
    arg-max where none does: the peak against its eight neighbours (`window`), against the median, its value against the
    threshold, adjacent scores (`score_gap`; for the fallback the distance to the largest value outside the peak's window).
    Low peaks under the threshold come and go with the last bits and change nothing the reference's caller reads.
    `others`: how far every other pixel that could pass median and threshold is from being a local maximum - these only have
    to stay what they are, and are held to 2 x the bound."""
    bound = 4.0 * float(np.abs(c32.astype(np.float64) - c64).max())
    delta = MARGIN * bound
    up = prm_np.upsample(c32[None], [(0, c) for c in labels], FACTOR)
    rec = {"delta": delta, "window": np.inf, "median": np.inf, "threshold": np.inf, "score_gap": np.inf, "others": np.inf}
    scores = []
    for m in up:
        h, w = m.shape
        m = m.astype(np.float64)
        pad = np.full((h + 2, w + 2), -np.inf)
        pad[1:-1, 1:-1] = m
        nb = np.max([pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3) if (dy, dx) != (1, 1)], axis=0)
        med = float(prm_np.lower_median(m))
        local = m > nb
        if np.any(local & (m >= med) & (m > threshold)):
            cand = m > threshold - delta
            pk = local & cand
            rec["window"] = min(rec["window"], float((m[pk] - nb[pk]).min()))
            rec["median"] = min(rec["median"], float(np.abs(m[pk] - med).min()))
            rec["threshold"] = min(rec["threshold"], float(np.abs(m[pk] - threshold).min()))
            rest = ~local & cand & (m >= med - delta)
            if rest.any():
                rec["others"] = min(rec["others"], float((nb[rest] - m[rest]).min()))
            scores += m[pk & (m >= med) & (m > threshold)].tolist()
        else:                                                        # the fallback: the first occurrence of the map's maximum
            y, x = np.unravel_index(int(np.argmax(m)), m.shape)
            rec["window"] = min(rec["window"], float(m[y, x] - nb[y, x]))
            rec["median"] = min(rec["median"], float(m[y, x] - med))
            rec["threshold"] = min(rec["threshold"], float(threshold - m[y, x]))
            far = m.copy()
            far[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = -np.inf
            rec["score_gap"] = min(rec["score_gap"], float(m[y, x] - far.max()))
            scores.append(float(m[y, x]))
    s = np.sort(np.array(scores))
    if s.size > 1:
        rec["score_gap"] = min(rec["score_gap"], float(np.diff(s).min()))
    ok = all(rec[k] >= delta for k in ("window", "median", "threshold", "score_gap")) and rec["others"] >= 2.0 * bound
    return rec if ok else None


def check_against_restatement(c32, labels, threshold, valid, score, img_h, img_w):
    up = prm_np.upsample(c32[None], [(0, c) for c in labels], FACTOR)
    res = prm_np.image_points(list(up), labels, img_h, img_w, threshold)
    order = agpl_order(score)
    assert res["status"] == 0 and res["count"] == len(score)
    assert np.array_equal(np.stack([res["classes"], res["ys"], res["xs"]], 1), valid[order, 1:])
    # (the scores themselves are ATen's up-sampled values: equal to the restatement's to the last bits only)
    assert np.allclose(res["scores"], score[order], rtol=1e-5, atol=1e-5)
    return res


def margin_record(recs):
    keys = ("delta", "window", "median", "threshold", "score_gap", "others")
    return np.array([[min(r[k], 1e30) for k in keys] for r in recs], dtype=np.float64)


def net_golden(gt):
    h, w = prm_cases.NET_SHAPE
    for seed in range(100, 200):
        x = torch.from_numpy(prm_cases.normalise(prm_cases.seeded_images(seed, 2, h, w)))
        model, keys, gain = calibrated(gt, seed, x)
        c32, c64 = crms(model, x)
        labels = [choose_labels(c32[i]) for i in range(2)]
        recs = [margins(c32[i], c64[i], labels[i], prm_cases.THRESHOLD) for i in range(2)]
        tops = [prm_np.upsample(c32[i][None], [(0, c) for c in labels[i]], FACTOR).reshape(3, -1).max(1) for i in range(2)]
        covered = any((t > prm_cases.THRESHOLD).any() for t in tops) and any((t < prm_cases.THRESHOLD).any() for t in tops)
        if None in recs or not covered:
            continue
        inf = model.inference()
        out = {"seed": np.int64(seed), "gain": np.float64(gain), "crm32": c32, "crm64": c64, "keys": np.array(keys),
               "labels": np.array(labels, dtype=np.int64), "margins": margin_record(recs)}
        for i in range(2):
            _, valid, score = ref_forward(inf, x[i:i + 1], labels[i], prm_cases.THRESHOLD)
            check_against_restatement(c32[i], labels[i], prm_cases.THRESHOLD, valid, score, FACTOR * c32.shape[2], FACTOR * c32.shape[3])
            order = agpl_order(score)
            out["valid_%d" % i], out["scores_%d" % i], out["order_%d" % i] = valid[:, 1:], score, order.astype(np.int64)
        return out
    raise AssertionError("no seed in 100..199 gives the margins")


def write_image_files(img_id, rgb, masks, classes):
    from PIL import Image
    s = str(img_id)
    name = s[:4] + "_" + s[4:]
    # a lossless file under the name assign_voc2012 opens (Pillow reads by content): the decoded array is the seeded one
    Image.fromarray(rgb).save(os.path.join("data", "VOC2012", "JPEGImages", name + ".jpg"), format="PNG")
    cell = np.empty((len(masks), 1), dtype=object)
    for i, m in enumerate(masks):
        cell[i, 0] = m.astype(np.uint8)
    scipy.io.savemat(os.path.join("data", "VOC2012", "COB_SBD_trainaug", name + ".mat"), {"maskmat": cell})
    FakeCOCO.table[img_id] = (name + ".jpg", [c + 1 for c in classes])


def e2e_golden(gt):
    from PIL import Image
    agpl = importlib.import_module("AGPL_label_assign")
    transform = sys.modules["lib.prm.prm_configs"].open_transform
    sizes = ((50, 70), (61, 45), (48, 48))
    for seed in range(300, 400):
        rgbs = [prm_cases.seeded_images(seed + 1000 * i, 1, hh, ww)[0] for i, (hh, ww) in enumerate(sizes)]
        x = torch.stack([transform(Image.fromarray(r)) for r in rgbs])
        assert tuple(x.shape[2:]) == (448, 448)
        model, _, gain = calibrated(gt, seed, x)
        c32, c64 = crms(model, x)
        weakest = int(np.argmin(c32[1].reshape(c32.shape[1], -1).max(1)))
        strongest = int(np.argmax(c32[2].reshape(c32.shape[1], -1).max(1)))
        labels = [choose_labels(c32[0]), [weakest], [strongest]]     # several classes | the fallback alone | one class, several peaks
        recs = [margins(c32[i], c64[i], labels[i], prm_cases.THRESHOLD) for i in range(3)]
        if None in recs:
            continue
        pre = [prm_np.image_points(list(prm_np.upsample(c32[i][None], [(0, c) for c in labels[i]], FACTOR)), labels[i],
                                   sizes[i][0], sizes[i][1], prm_cases.THRESHOLD) for i in range(3)]
        fallback = c32[1, weakest].max() < prm_cases.THRESHOLD and pre[1]["count"] == 1
        if not (fallback and pre[2]["count"] >= 3 and pre[0]["count"] >= 3 and len(set(pre[0]["classes"].tolist())) >= 2):
            continue
        rng = np.random.RandomState(seed)
        masks = [synthetic.make_masks(40, hh, ww, rng, min_side=6)[0] for hh, ww in sizes]
        for m in masks:
            m[0] = True                                              # the full image: every point is covered by a proposal
        seen = []
        inf_forward = model.forward

        def recording(*a, **k):
            res = inf_forward(*a, **k)
            seen.append(res)
            return res
        model.forward = recording
        cwd = os.getcwd()
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            try:
                for d in ("VOC2012/COB_SBD_trainaug", "VOC2012/JPEGImages", "trash"):
                    os.makedirs(os.path.join("data", d))
                for i in range(3):
                    write_image_files(IDS[i], rgbs[i], masks[i], labels[i])
                agpl.assign_voc2012(list(IDS), 0, model, "cpu", "voc", FakeCOCO())
                mats = pickle.load(open(os.path.join("data", "trash", agpl.useless_file.format(0)), "rb"))
            finally:
                os.chdir(cwd)
        assert mats["indexes"] == list(IDS) and len(seen) == 3
        out = {"seed": np.int64(seed), "gain": np.float64(gain), "margins": margin_record(recs)}
        for i in range(3):
            _, _, valid, prms, score = seen[i]
            valid, score = valid.numpy().astype(np.int64), score.numpy().astype(f32)
            res = check_against_restatement(c32[i], labels[i], prm_cases.THRESHOLD, valid, score, sizes[i][0], sizes[i][1])
            order = agpl_order(score)
            mat = mats["mat"][i]
            assert mat.dtype == np.float32 and mat.shape == (40, 21)
            # the restatement end to end: its points through proposal_prep_np give the reference's matrix
            assert np.array_equal(ppn.assign_clusters(masks[i], res["rows"], res["cols"], res["classes"], 20), mat)
            bits, shape = ppn.pack_bits(masks[i])
            out.update({"rgb_%d" % i: rgbs[i], "mask_bits_%d" % i: bits, "mask_shape_%d" % i: shape, "crm32_%d" % i: c32[i],
                        "labels_%d" % i: np.array(labels[i], dtype=np.int64), "valid_%d" % i: valid[:, 1:], "scores_%d" % i: score,
                        "order_%d" % i: order.astype(np.int64), "mat_%d" % i: mat})
        assert len(np.unique(out["mat_2"][out["mat_2"] > 0])) >= 2 or out["valid_2"].shape[0] >= 3
        return out
    raise AssertionError("no seed in 300..399 gives the margins and the situations")


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    gt = install()
    files = {"prm_peaks": crafted_goldens(gt), "prm_net": net_golden(gt), "prm_e2e": e2e_golden(gt)}
    for name, arrays in files.items():
        path = os.path.join(HERE, name + ".npz")
        save_npz(path, arrays)
        print(name, os.path.getsize(path), "bytes", {k: int(v) for k, v in arrays.items() if k == "seed"})


if __name__ == "__main__":
    main()
