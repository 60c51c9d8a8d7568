#!/usr/bin/env python3
"""The PRM peak back-propagation on the device (cim_amd.prm.backprop): HIP-event ms, warm, median of --repeats,
per image at 448 x 448, full width, for P = 1, 4, 16 peaks:
  - `prm.backprop` whole (its forward pass that keeps xs, y, n + the backward walk) and the forward pass alone,
  - what the parent commit's `prm.peaks` costs on the same image (one plain forward + the three peak launches + the read),
  - the reference's own shape on the same device: the network through ATen / MIOpen with every nn.Conv2d patched to the
    probability-normalised rule, ONE forward and then P sequential backward(retain_graph=True) passes at batch 1 (patched in from
    here, as tools/bench_library_paths.py patches its library paths; printed, not credited as a kernel-against-kernel speed-up),
  - the element-wise launches on layer1-sized tensors (256 x 112 x 112) with the HBM rate their bytes give, and the stem kernel.

    python tools/bench_prm_backprop.py [--repeats 10] [--no-aten]

One JSON line per finished section (the last line holds everything)."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cim_amd import _lib, prm, prm_backprop  # noqa: E402


def median_ms(fn, repeats, warm=2):
    for _ in range(warm):
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


class _RuleConv(torch.autograd.Function):
    """One convolution under the rule, through ATen: the ordinary response forward; backward dx = xs * conv_transpose(ghat, W+)."""

    @staticmethod
    def forward(ctx, x, conv):
        xs = x - x.min()
        wpos = conv.weight.clamp(min=0)
        n = F.conv2d(xs, wpos, None, conv.stride, conv.padding)
        ctx.save_for_backward(xs, wpos, n)
        ctx.conv = conv
        return F.conv2d(x, conv.weight, conv.bias, conv.stride, conv.padding)

    @staticmethod
    def backward(ctx, g):
        xs, wpos, n = ctx.saved_tensors
        ghat = torch.where(n < 1e-10, torch.zeros_like(g), g / (n.abs() + 1e-10))
        return xs * torch.nn.grad.conv2d_input(xs.shape, wpos, ghat, ctx.conv.stride, ctx.conv.padding), None


def aten_sequential(model, x, peaks, factor):
    """One ATen forward with the patched convolutions, then one backward per peak: the reference's loop."""
    f = model[0].features
    x = x.clone().requires_grad_()
    conv = lambda m, t: _RuleConv.apply(t, m)
    y = f[3](F.relu(f[1](conv(f[0], x))))
    for i in range(4, 8):
        for blk in f[i]:
            idt = y if blk.downsample is None else blk.downsample[1](conv(blk.downsample[0], y))
            t = F.relu(blk.bn1(conv(blk.conv1, y)))
            t = F.relu(blk.bn2(conv(blk.conv2, t)))
            y = F.relu(blk.bn3(conv(blk.conv3, t)) + idt)
    up = F.interpolate(conv(model[0].classifier[0], y), scale_factor=factor, mode="bilinear", align_corners=True)
    seed = torch.zeros_like(up)
    maps = []
    for c, py, px in peaks:
        seed.zero_()
        seed[0, c, py, px] = 1
        if x.grad is not None:
            x.grad.zero_()
        up.backward(seed, retain_graph=True)
        s = x.grad.detach().sum(1).clamp(min=0)
        maps.append(s / s.sum())
    return torch.cat(maps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-aten", action="store_true", help="skip the sequential ATen / MIOpen passes (their first call tunes)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = prm.PeakResponseMapping(prm.fc_resnet50(20)).to(dev)
    for p in model.parameters():
        p.requires_grad = False
    x = torch.randn(1, 3, prm.INPUT_SIZE, prm.INPUT_SIZE, device=dev)
    with torch.no_grad():
        cls = model[0].classifier[0]
        cls.bias.zero_()
        cls.weight.mul_(30.0 / float(model(x).abs().max()))
    rng = np.random.RandomState(0)
    rec = dict(bench="prm_backprop", repeats=args.repeats, device=torch.cuda.get_device_name(0), size=prm.INPUT_SIZE)
    labels = [[2, 7, 14]]
    med, lohi = median_ms(lambda: prm.peaks(model, x, labels), args.repeats)
    rec["parent_prm_peaks_ms"], rec["parent_prm_peaks_min_max_ms"] = med, lohi
    med, lohi = median_ms(lambda: model(x), args.repeats)
    rec["plain_forward_ms"] = med
    med, lohi = median_ms(lambda: prm_backprop.Forward(model, x), args.repeats)
    rec["keeping_forward_ms"], rec["keeping_forward_min_max_ms"] = med, lohi
    drawn = {P: np.stack([rng.randint(0, 20, P), rng.randint(0, 112, P), rng.randint(0, 112, P)], 1) for P in (1, 4, 16)}
    for P in (1, 4, 16):
        peaks = drawn[P]
        med, lohi = median_ms(lambda: prm.backprop(model, x, peaks), args.repeats)
        rec["backprop_P%d_ms" % P], rec["backprop_P%d_min_max_ms" % P] = med, lohi
        rec["backprop_P%d_chunk" % P] = prm_backprop.default_chunk(64, prm.INPUT_SIZE, prm.INPUT_SIZE, P)
    print(json.dumps(rec), flush=True)
    # the element-wise launches on layer1-sized tensors, the stem kernel
    c, hw = 256, 112 * 112
    shared = [torch.rand(c, hw, device=dev) + 0.5 for _ in range(3)]
    a = torch.rand(c, device=dev) + 0.5
    st = _lib.stream_ptr()
    for P in (4, 16):
        g = torch.rand(P, c, hw, device=dev)
        out, res = torch.empty_like(g), torch.empty_like(g)
        plane = 4 * c * hw
        for name, fn, nbytes in (
                ("gate", lambda: _lib.call("cim_prmb_gate", g.data_ptr(), None, shared[0].data_ptr(), a.data_ptr(), shared[1].data_ptr(),
                                           out.data_ptr(), None, P, c, hw, st), (2 * P + 2) * plane),
                ("gate_mul", lambda: _lib.call("cim_prmb_gate", g.data_ptr(), shared[2].data_ptr(), shared[0].data_ptr(), a.data_ptr(),
                                               shared[1].data_ptr(), out.data_ptr(), None, P, c, hw, st), (2 * P + 3) * plane),
                ("gate_dres", lambda: _lib.call("cim_prmb_gate", g.data_ptr(), None, shared[0].data_ptr(), a.data_ptr(), shared[1].data_ptr(),
                                                out.data_ptr(), res.data_ptr(), P, c, hw, st), (3 * P + 2) * plane),
                ("scale_add", lambda: _lib.call("cim_prmb_scale", shared[2].data_ptr(), g.data_ptr(), res.data_ptr(), out.data_ptr(), P, c * hw, st),
                 (3 * P + 1) * plane)):
            med, lohi = median_ms(fn, args.repeats)
            rec["%s_P%d_ms" % (name, P)], rec["%s_P%d_GBps" % (name, P)] = med, round(nbytes / med / 1e6, 1)
        del g, out, res
    for P in (4, 16):
        ghat = torch.rand(P, 64, 224, 224, device=dev)
        wpos = torch.rand(64, 3, 7, 7, device=dev)
        xs = torch.rand(3, 448, 448, device=dev)
        out = torch.empty(P, 448, 448, device=dev)
        ws = torch.empty(_lib.call("cim_prmb_stem_workspace", P, 448, 448) // 8, dtype=torch.float64, device=dev)
        med, lohi = median_ms(lambda: _lib.call("cim_prmb_stem", ghat.data_ptr(), wpos.data_ptr(), xs.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                                P, 64, 448, 448, 1, st), args.repeats)
        flop = 2.0 * P * 64 * 224 * 224 * 49 * 3                      # every (output pixel, tap, input channel) product once
        rec["stem_P%d_ms" % P], rec["stem_P%d_TFLOPs" % P] = med, round(flop / med / 1e9, 2)
        rec["stem_P%d_GBps" % P] = round(4.0 * (ghat.numel() + 2 * out.numel()) / med / 1e6, 1)
        del ghat, out
    print(json.dumps(rec), flush=True)
    if not args.no_aten:
        for P in (1, 4, 16):
            peaks = drawn[P].tolist()                             # the peaks the device was timed on
            if P == 1:                                            # the same maps, to rounding: the comparison times the same work
                ours = prm.backprop(model, x, peaks)
                theirs = aten_sequential(model, x, peaks, 8)
                rec["aten_vs_device_max_rel"] = float((ours - theirs).abs().max() / theirs.max())
            med, lohi = median_ms(lambda: aten_sequential(model, x, peaks, 8), max(3, args.repeats // 3), warm=1)
            rec["aten_sequential_P%d_ms" % P], rec["aten_sequential_P%d_min_max_ms" % P] = med, lohi
            print(json.dumps(rec), flush=True)
    rec["note"] = "shared pool: neighbours move these numbers by several per cent; the baselines are printed, not credited"
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
