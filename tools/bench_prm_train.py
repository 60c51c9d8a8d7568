#!/usr/bin/env python3
"""The PRM training head on the device (cim_amd.prm_train, csrc/prm_train.hip): HIP-event ms, warm, median of
--repeats, of the head alone - class response maps [16, C, 14, 14] -> aggregation -> loss, forward plus backward - at C = 20
and C = 80, against two comparators interleaved in the same process on the same device, printed and NOT credited as a speed-up:
  (a) the torch composition of the reference: F.interpolate(align_corners=True), pad, max_pool2d(return_indices), torch.median,
      the peak stimulation Function of prm_modules (aggregation, peak_map * grad backward), F.multilabel_soft_margin_loss;
  (b) forward only: the existing up-sampling + peaks launches of csrc/prm.hip on all B C pairs.
Beside them the bytes each form moves (from the shapes) and the whole training step - prm_train.loss, backward, SGD - at
448 x 448, B = 16, in images per second.

    python tools/bench_prm_train.py [--repeats 20] [--no-step]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cim_amd import _lib, prm, prm_train  # noqa: E402
from cim_amd.optim import SGD  # noqa: E402

B, HW, FACTOR = 16, 14, 8


class TorchPeakStimulation(torch.autograd.Function):
    """The reference's formulation (prm_modules.py:9-51) restated in torch for the comparison: dense maps forward and backward."""

    @staticmethod
    def forward(ctx, up):
        b, c, h, w = up.shape
        padded = F.pad(up, (1, 1, 1, 1), value=float("-inf"))
        element = torch.arange((h + 2) * (w + 2), device=up.device).view(1, 1, h + 2, w + 2)[:, :, 1:-1, 1:-1]
        _, idx = F.max_pool2d(padded, 3, 1, return_indices=True)
        med = torch.median(up.view(b, c, h * w), dim=2)[0].view(b, c, 1, 1)
        peak_map = ((idx == element) & (up >= med)).float()
        ctx.save_for_backward(peak_map)
        return (up * peak_map).view(b, c, -1).sum(2) / peak_map.view(b, c, -1).sum(2)

    @staticmethod
    def backward(ctx, grad):
        peak_map, = ctx.saved_tensors
        return peak_map * grad.view(grad.shape[0], grad.shape[1], 1, 1)


def interleaved_ms(fns, repeats):
    """name -> median ms, the candidates taking turns inside every repeat (neighbours on the device hit all alike)."""
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)] for k, v in times.items()}


def bytes_moved(c):
    maps, low, up = B * c, HW * HW * 4, (HW * FACTOR) ** 2 * 4
    words = ((HW * FACTOR) ** 2 + 31) // 32 * 4
    return {
        # read the map, write bitmap + 4 scalars | read bitmap + 2 scalars, write the gradient
        "hip_fused": maps * (low + words + 16) + maps * (words + 8 + low),
        # forward: up written, padded copy written + read, pooled values + int64 indices written, compare / median (sorted copy) /
        # mask / product each a dense pass; backward: dense gradient written and read by the interpolation's scatter
        "torch_composition_at_least": maps * up * (1 + 2 + 1 + 2 + 4 * 2 + 2 + 2),
        "hip_upsample_plus_peaks_forward": maps * (low + up) + maps * up * 5,      # up written, read by 4 median passes + the peak test
    }


def head(c, repeats):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(c)
    crm = (torch.randn(B, c, HW, HW, generator=g) * 5).to(dev).requires_grad_(True)
    target = (torch.rand(B, c, generator=g) < 0.2).float().to(dev)

    def hip():
        crm.grad = None
        agg, _ = prm_train.peak_stimulation(crm, FACTOR)
        prm_train.multilabel_soft_margin_loss(agg, target).backward()

    def composition():
        crm.grad = None
        up = F.interpolate(crm, scale_factor=FACTOR, mode="bilinear", align_corners=True)
        F.multilabel_soft_margin_loss(TorchPeakStimulation.apply(up), target).backward()

    def hip_forward():
        with torch.no_grad():
            prm_train.peak_stimulation(crm, FACTOR)

    labels = [list(range(c))] * B
    run = prm._Launch(labels, [(448, 448)] * B, c, dev)
    ws = run.workspace((HW * FACTOR) ** 2, dev)
    host = run.desc_host.ctypes.data_as(ctypes.c_void_p)
    data = crm.detach()

    def pairs_forward():
        _lib.call("cim_prm_points", data.data_ptr(), None, B, c, HW, HW, FACTOR, run.m, host, run.desc_dev.data_ptr(), 10.0, *run.out_ptrs(),
                  ws.data_ptr(), _lib.stream_ptr())

    def composition_forward():
        with torch.no_grad():
            TorchPeakStimulation.apply(F.interpolate(data, scale_factor=FACTOR, mode="bilinear", align_corners=True))

    ms = interleaved_ms({"hip_fwd_bwd": hip, "torch_composition_fwd_bwd": composition, "hip_fwd": hip_forward,
                         "hip_upsample_plus_peaks_fwd": pairs_forward, "torch_composition_fwd": composition_forward}, repeats)
    return {"ms_median_min_max": ms, "bytes": bytes_moved(c)}


def training_step(repeats):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = prm_train.freeze(prm.PeakResponseMapping(prm.fc_resnet50(20))).to(dev)
    x = torch.randn(B, 3, prm.INPUT_SIZE, prm.INPUT_SIZE, device=dev)
    target = (torch.rand(B, 20, device=dev) < 0.2).float()
    opt = SGD([p for p in model.parameters() if p.requires_grad], lr=1e-4, momentum=0.9, weight_decay=1e-4)

    def step():
        opt.zero_grad()
        prm_train.loss(model, x, target).backward()
        opt.step()

    ms = interleaved_ms({"step": step}, repeats)["step"]
    return {"ms_median_min_max": ms, "images_per_second": round(B / ms[0] * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="skip the whole training step")
    args = ap.parse_args()
    rec = dict(bench="prm_train", repeats=args.repeats, device=torch.cuda.get_device_name(0), B=B, map="%dx%d x %d^2" % (HW, HW, FACTOR))
    for c in (20, 80):
        rec["head_C%d" % c] = head(c, args.repeats)
    rec["training_step_448_B16"] = "not measured" if args.no_step else training_step(max(5, args.repeats // 2))
    rec["note"] = "shared pool: neighbours move these numbers by several per cent; the comparators are printed, not credited"
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
