#!/usr/bin/env python3
"""The PRM label assignment on the device (cim_amd.prm, proposal_prep.label_assign): HIP-event ms, warm, median
of --repeats, of
  - the forward pass at 448 x 448, full width, per image at B = 1 and B = 8,
  - the three launches of csrc/prm.hip for 3 classes per image (and the call with its one read),
  - the whole label_assign of one image at 1000 x 375 x 500 proposal masks;
beside them, in the same run on the same device and NOT credited as a speed-up, the same network through ATen / MIOpen and a
torch restatement of the reference's peak stimulation (all C maps, as the reference computes them).  The reference additionally
runs one backward pass through the patched network per valid peak, which this package does not reproduce: the comparison that
matters is "one forward instead of one forward plus P backwards", not a kernel against a kernel.

    python tools/bench_prm.py [--repeats 20] [--no-aten]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cim_amd import _lib, prm, proposal_prep, synthetic  # noqa: E402


def median_ms(fn, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return round(float(np.median(times)), 4), [round(float(np.min(times)), 4), round(float(np.max(times)), 4)]


def aten_forward(model, x):
    """The same modules through ATen / MIOpen (what the reference's network runs on)."""
    f = model[0].features
    with torch.no_grad():
        x = f[3](f[2](f[1](f[0](x))))
        for i in range(4, 8):
            for blk in f[i]:
                idt = x if blk.downsample is None else blk.downsample(x)
                y = F.relu(blk.bn1(blk.conv1(x)))
                y = F.relu(blk.bn2(blk.conv2(y)))
                x = F.relu(blk.bn3(blk.conv3(y)) + idt)
        return model[0].classifier(x)


def torch_peak_stimulation(crm, factor):
    """prm_model_gt.py:227-232 + prm_modules.py:16-34 in torch on the device: every class map, the nonzero at the end."""
    up = F.interpolate(crm, scale_factor=factor, mode="bilinear", align_corners=True)
    b, c, h, w = up.shape
    padded = F.pad(up, (1, 1, 1, 1), value=float("-inf"))
    element = torch.arange((h + 2) * (w + 2), device=up.device).view(1, 1, h + 2, w + 2)[:, :, 1:-1, 1:-1]
    _, idx = F.max_pool2d(padded, 3, 1, return_indices=True)
    med = torch.median(up.view(b, c, h * w), dim=2)[0].view(b, c, 1, 1)
    return torch.nonzero((idx == element) & (up >= med))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-aten", action="store_true", help="skip the ATen / MIOpen forward (its first call tunes)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = prm.PeakResponseMapping(prm.fc_resnet50(20)).to(dev)
    x8 = torch.randn(8, 3, prm.INPUT_SIZE, prm.INPUT_SIZE, device=dev)
    with torch.no_grad():                                        # a few responses above the peak threshold, none non-finite
        cls = model[0].classifier[0]
        cls.bias.zero_()
        cls.weight.mul_(30.0 / float(model(x8).abs().max()))
    rec = dict(bench="prm", repeats=args.repeats, device=torch.cuda.get_device_name(0))
    for b in (1, 8):
        x = x8[:b].contiguous()
        med, lohi = median_ms(lambda: model(x), args.repeats)
        rec["forward_B%d_ms_per_image" % b], rec["forward_B%d_min_max_ms" % b] = round(med / b, 4), lohi
        if not args.no_aten:
            med, lohi = median_ms(lambda: aten_forward(model, x), args.repeats)
            rec["aten_forward_B%d_ms_per_image" % b], rec["aten_forward_B%d_min_max_ms" % b] = round(med / b, 4), lohi
        crm = model(x)
        labels = [[2, 7, 14]] * b
        run = prm._Launch(labels, [(375, 500)] * b, 20, dev)
        ws = run.workspace(112 * 112, dev)
        import ctypes
        host = run.desc_host.ctypes.data_as(ctypes.c_void_p)
        med, lohi = median_ms(lambda: _lib.call("cim_prm_points", crm.data_ptr(), None, b, 20, 14, 14, 8, run.m, host, run.desc_dev.data_ptr(),
                                                10.0, *run.out_ptrs(), ws.data_ptr(), _lib.stream_ptr()), args.repeats)
        rec["peak_launches_B%d_ms" % b], rec["peak_launches_B%d_min_max_ms" % b] = med, lohi
        med, lohi = median_ms(lambda: prm.peaks_from_crm(crm, labels, 8, [(375, 500)] * b), args.repeats)
        rec["peaks_with_read_B%d_ms" % b] = med
        rec["valid_peaks_B%d" % b] = [len(r[0]) for r in prm.peaks_from_crm(crm, labels, 8, [(375, 500)] * b)]
        med, lohi = median_ms(lambda: torch_peak_stimulation(crm, 8), args.repeats)
        rec["torch_peak_stimulation_B%d_ms" % b] = med
    inp = synthetic.make_image_inputs("resnet50_voc", seed=3, with_image=False)
    masks = torch.from_numpy(inp["full_masks"]).to(dev)
    n, h, w = masks.shape
    rgb = np.random.RandomState(1).randint(0, 256, (h, w, 3)).astype(np.uint8)
    med, lohi = median_ms(lambda: proposal_prep.label_assign(model, [rgb], [[2, 7, 14]], [masks]), args.repeats)
    rec["label_assign_%dx%dx%d_ms" % (n, h, w)], rec["label_assign_min_max_ms"] = med, lohi
    rec["note"] = "shared pool: neighbours move these numbers by several per cent; the baselines are printed, not credited"
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
