#!/usr/bin/env python3
"""Capture the peak response maps by RUNNING THE REFERENCE on the CPU (its checkout: _ref_shims.REF_ROOT).

    python tests/golden/make_golden_prm_backprop.py      # rewrites tests/golden/prm_backprop.npz, byte-identically

Runs lib/prm/prm_model_gt.py `PeakResponseMapping(...).inference()` - its peak back-propagation through the convolutions patched by
lib/prm/prm_modules.py pr_conv2d - on the thin network of make_golden_prm.py (stubs and the torchvision-shaped ResNet are imported
from there; prm_cases' seeded weights, WIDTH = 16, regenerated on both sides, never stored) and the two 64 x 96 images of
prm_net.npz, one at a time, in fp32 and, with the same weights widened, in float64.  Nothing of the reference is written into this
repository.

Per image i: peaks_i [P, 3] = (class, y, x) in the order the reference found them, prm32_i / prm64_i [P, 64, 96] (at most MAX_P maps
are kept).  One crafted case, `nan`: image 0 with the classifier row of one more class replaced by -|row| - no positive weight, so
no gradient passes the classifier and that class's maps are 0 / 0 = NaN, its neighbours in the same call those of image 0.

Condition: a near-tie in a max-pool window would move gradient by a pixel - a discrete change.  The margin make_golden_prm.py asks
of its decisions (the winner of every window leading the window's second value by MARGIN x the forward bound, 4 x max |fp32 -
float64| of the pool's input, wherever it is positive) cannot be had here: on smooth images neighbouring stem outputs are closer
than that in some of the 6144 windows at every seed tried (100..111: smallest leads 9e-8..8e-5 against 4e-4..2e-3 needed).  What is
asked instead is what decides: the arg-max of EVERY window is the same in the fp32 and in the float64 forward pass of the seed of
prm_net.npz (asserted), so the two captured runs route alike; the margins are recorded (`pool_margins`: per image MARGIN x bound and
the smallest lead of a positive winner).  The smallest lead at this seed, 5.8e-6, is about the forward bound itself (7.6e-6):
nothing here guarantees that an implementation which sums the stem in another order routes every window as these two runs do.
tests/test_gpu_prm_backprop.py therefore compares the device's arg-max of every window with the restatement's before it compares
maps, so that a flipped window is reported as a routing flip.  ReLU gates need no margin: a unit near 0 carries a gradient proportional to its own value."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden_prm as mg  # noqa: E402
import prm_backprop_np as bp  # noqa: E402
import prm_cases  # noqa: E402
from make_golden_proposal_prep import save_npz  # noqa: E402

MAX_P = 6
MARGIN = mg.MARGIN


def pool_margin(model, x):
    """(MARGIN x bound, smallest lead of a positive window winner over the second value of its window) for one image."""
    y32 = bp.Network(model[0].features, model[0].classifier[0], torch.float32)
    y64 = bp.Network(model[0].features, model[0].classifier[0], torch.float64)
    y32.forward(x)
    y64.forward(x)
    bound = 4.0 * float((y32.y0.double() - y64.y0).abs().max())
    win = F.unfold(F.pad(y64.y0, (1, 1, 1, 1), value=-np.inf).reshape(-1, 1, y64.y0.shape[2] + 2, y64.y0.shape[3] + 2), 3, stride=2)
    top = win.sort(dim=1, descending=True).values
    lead = (top[:, 0] - top[:, 1])[top[:, 0] > 0]
    assert torch.equal(y32.idx, y64.idx), "a max-pool window has different winners in fp32 and float64: choose another seed"
    return MARGIN * bound, float(lead.min())


def run_reference(gt, seed, gain, x, labels, double, edit=None):
    """-> (peaks [P, 3] as found, maps [P, H, W]) of the reference's .inference() model on one image."""
    model, _ = mg.build_reference(gt, seed, gain)
    if edit is not None:
        edit(model)
    if double:
        model, x = model.double(), x.double()
    out = model.inference()(x.clone(), torch.tensor(labels), class_threshold=0, peak_threshold=prm_cases.THRESHOLD)
    assert out is not None
    _, _, valid, prms, _ = out
    return valid.numpy().astype(np.int64)[:, 1:], prms.detach().numpy()


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    gt = mg.install()
    net = np.load(os.path.join(HERE, "prm_net.npz"))
    seed, gain = int(net["seed"]), float(net["gain"])
    h, w = prm_cases.NET_SHAPE
    x = torch.from_numpy(prm_cases.normalise(prm_cases.seeded_images(seed, 2, h, w)))
    plain, _ = mg.build_reference(gt, seed, gain)
    plain.eval()
    out = {"seed": np.int64(seed), "gain": np.float64(gain), "factor": np.int64(mg.FACTOR)}
    margins = []
    for i in range(2):
        need, lead = pool_margin(plain, x[i:i + 1])
        margins.append((need, lead))
        labels = net["labels"][i].tolist()
        pk32, m32 = run_reference(gt, seed, gain, x[i:i + 1], labels, False)
        pk64, m64 = run_reference(gt, seed, gain, x[i:i + 1], labels, True)
        assert np.array_equal(pk32, pk64) and np.array_equal(pk32, net["valid_%d" % i])
        assert m32.dtype == np.float32 and m64.dtype == np.float64 and m32.shape == (len(pk32), h, w)
        assert np.isfinite(m64).all() and np.allclose(m64.reshape(len(pk64), -1).sum(1), 1.0)
        out["peaks_%d" % i], out["prm32_%d" % i], out["prm64_%d" % i] = pk32[:MAX_P], m32[:MAX_P], m64[:MAX_P]
        # the restatement in float64 on the same weights
        mine = bp.Network(plain[0].features, plain[0].classifier[0], torch.float64).maps(x[i:i + 1], pk64[:MAX_P], mg.FACTOR)
        err = max(float(np.abs(mine[k] - m64[k]).max() / m64[k].max()) for k in range(len(mine)))
        assert err <= 1e-12, err
        print("image", i, "peaks", len(pk32), "kept", len(out["peaks_%d" % i]), "restatement", err)
    out["pool_margins"] = np.array(margins, dtype=np.float64)
    # the crafted case: one more class whose classifier row has no positive weight
    labels0 = net["labels"][0].tolist()
    c_nan = next(c for c in range(prm_cases.NUM_CLASSES) if c not in labels0)

    def edit(model):
        with torch.no_grad():
            wt = model[0].classifier[0].weight
            wt[c_nan] = -wt[c_nan].abs()
    pk, m = run_reference(gt, seed, gain, x[0:1], sorted(labels0 + [c_nan]), False, edit)
    rows = [k for k in range(len(pk)) if pk[k, 0] == c_nan][:2] + [k for k in range(len(pk)) if pk[k, 0] != c_nan][:MAX_P - 2]
    rows = sorted(rows)
    assert any(pk[k, 0] == c_nan for k in rows) and any(pk[k, 0] != c_nan for k in rows)
    for k in rows:
        assert np.isnan(m[k]).all() if pk[k, 0] == c_nan else np.isfinite(m[k]).all()
    out["nan_class"], out["nan_labels"] = np.int64(c_nan), np.array(sorted(labels0 + [c_nan]), dtype=np.int64)
    out["nan_peaks"], out["nan_prm32"] = pk[rows], m[rows]
    path = os.path.join(HERE, "prm_backprop.npz")
    save_npz(path, out)
    print("prm_backprop", os.path.getsize(path), "bytes", "nan class", c_nan, "rows", pk[rows].tolist())


if __name__ == "__main__":
    main()
