#!/usr/bin/env python3
"""Capture the PRM training goldens by RUNNING THE REFERENCE on the CPU (its checkout: _ref_shims.REF_ROOT).

    python tests/golden/make_golden_prm_train.py      # rewrites tests/golden/prm_train.npz, byte-identically

Runs the reference's own lib/prm/prm_modules.py `peak_stimulation` (forward and backward) with `PeakResponseMapping._median_filter`
as its peak filter on the GIVEN up-sampled maps of prm_train_cases.crafted_batch (factor 1), and stores per shape the peak list,
the aggregation and the gradient it returns for the seeded grad_output.  Nothing of the reference is written into this
repository; the import shims are those of make_golden_prm.py.

The maps hold dyadic values, so the reference's sums are exact.  Its hand-written backward returns peak_map * grad_output - it
does not divide by the number of peaks as the derivative of its forward would (prm_modules.py:47-51); the file stores what it
returns, and the tests compare that divided by the count."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden_prm  # noqa: E402
import prm_train_cases as cases  # noqa: E402
import prm_train_np as ptn  # noqa: E402
from make_golden_proposal_prep import save_npz  # noqa: E402


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    gt = make_golden_prm.install()
    mods = importlib.import_module("lib.prm.prm_modules")
    median_filter = gt.PeakResponseMapping._median_filter
    out = {}
    for shape in cases.SHAPES:
        key = "%dx%d" % shape
        x = torch.from_numpy(cases.crafted_batch(shape)).requires_grad_(True)
        peak_list, agg = mods.peak_stimulation(x, return_aggregation=True, win_size=3, peak_filter=median_filter)
        agg.backward(torch.from_numpy(cases.grad_output(shape)))
        out[key + "__peak_list"] = peak_list.numpy().astype(np.int64)
        out[key + "__agg"] = agg.detach().numpy().astype(np.float32)
        out[key + "__grad"] = x.grad.numpy().astype(np.float32)
        # the restatement on the same maps: the same peaks
        res = ptn.stimulate(cases.crafted_batch(shape), 1)
        assert np.array_equal(ptn.peak_list(res["peaks"]), out[key + "__peak_list"]), key
    path = os.path.join(HERE, "prm_train.npz")
    save_npz(path, out)
    print("prm_train", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
