#!/usr/bin/env python3
"""Pillow's antialiased resize on the device (cim_amd.resample, csrc/resample.hip): HIP-event ms, warm, median
of --repeats, B = 1 and 8, sources 375 x 500 -> 448 x 448, of
  - the three launches alone (sources already on the device) and `network_input_from_images` from host arrays (staging into
    pinned memory and the upload included),
  - what it replaces: Pillow's host call per image, and that call + the upload + `network_input` per batch,
  - `label_assign` with resize="device" against resize="pillow": the two settings alternate inside one session; each setting's
    samples are also split into its even and odd rounds, whose two medians show what repeated runs of ONE setting differ by.

    python tools/bench_resample.py [--repeats 20] [--out profiles/r6/bench_resample.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cim_amd import _lib, prm, proposal_prep, resample, synthetic  # noqa: E402
from cim_amd.utils import blob  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(times):
    return round(float(np.median(times)), 4), [round(float(np.min(times)), 4), round(float(np.max(times)), 4)]


def median_ms(fn, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return stats([timed(fn) for _ in range(repeats)])


def interleaved(fns, repeats):
    """name -> fn, run in turn `repeats` times: per name (median, [min, max], [median of even rounds, median of odd rounds])."""
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(timed(fn))
    return {k: stats(t) + ([round(float(np.median(t[0::2])), 4), round(float(np.median(t[1::2])), 4)],) for k, t in times.items()}


def main():
    from PIL import Image
    import PIL
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    size = prm.INPUT_SIZE
    rng = np.random.RandomState(1)
    rec = dict(bench="resample", repeats=args.repeats, device=torch.cuda.get_device_name(0), pillow=PIL.__version__,
               source=[375, 500], output=[size, size])

    def pillow_resize(images):
        return np.stack([np.asarray(Image.fromarray(im).resize((size, size), Image.BILINEAR)) for im in images])

    ms6 = ctypes.cast((ctypes.c_float * 6)(*blob.MEAN, *blob.STD), ctypes.c_void_p)
    for b in (1, 8):
        images = [rng.randint(0, 256, (375, 500, 3)).astype(np.uint8) for _ in range(b)]
        assert np.array_equal(resample.pil_resize(images, size).cpu().numpy(), pillow_resize(images))
        run = resample._gather(images, size, size, dev, "bench")
        out = torch.empty((b, 3, size, size), dtype=torch.float32, device=dev)
        med, lohi = median_ms(lambda: _lib.call("cim_resample_rgb", run.src.data_ptr(), run.desc_ptr, run.desc_dev.data_ptr(), b, size, size,
                                                None, out.data_ptr(), ms6, run.ws.data_ptr(), _lib.stream_ptr()), args.repeats)
        rec["device_launches_B%d_ms" % b], rec["device_launches_B%d_min_max_ms" % b] = med, lohi
        res = interleaved({"device": lambda: prm.network_input_from_images(images),
                           "pillow": lambda: prm.network_input(torch.from_numpy(pillow_resize(images)).to(dev))}, args.repeats)
        for k, (med, lohi, halves) in res.items():
            rec["input_%s_B%d_ms" % (k, b)], rec["input_%s_B%d_min_max_ms" % (k, b)] = med, lohi
        t = []
        for _ in range(args.repeats):                                # the host call alone, wall clock
            t0 = time.perf_counter()
            pillow_resize(images)
            t.append((time.perf_counter() - t0) * 1e3 / b)
        rec["pillow_host_call_B%d_ms_per_image" % b] = round(float(np.median(t)), 4)

    model = prm.PeakResponseMapping(prm.fc_resnet50(20)).to(dev)
    x8 = torch.randn(8, 3, size, size, device=dev)
    with torch.no_grad():                                            # a few responses above the peak threshold, none non-finite
        cls = model[0].classifier[0]
        cls.bias.zero_()
        cls.weight.mul_(30.0 / float(model(x8).abs().max()))
    inp = synthetic.make_image_inputs("resnet50_voc", seed=3, with_image=False)
    masks = torch.from_numpy(inp["full_masks"]).to(dev)
    n, h, w = masks.shape
    rec["label_assign_masks"] = [n, h, w]
    for b in (1, 8):
        images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(b)]
        labels, mlist = [[2, 7, 14]] * b, [masks] * b
        same = [torch.equal(p, q) for p, q in zip(proposal_prep.label_assign(model, images, labels, mlist, resize="device"),
                                                  proposal_prep.label_assign(model, images, labels, mlist, resize="pillow"))]
        assert all(same), same
        res = interleaved({"device": lambda: proposal_prep.label_assign(model, images, labels, mlist, resize="device"),
                           "pillow": lambda: proposal_prep.label_assign(model, images, labels, mlist, resize="pillow")}, args.repeats)
        for k, (med, lohi, halves) in res.items():
            rec["label_assign_%s_B%d_ms_per_image" % (k, b)] = round(med / b, 4)
            rec["label_assign_%s_B%d_min_max_ms" % (k, b)] = lohi
            rec["label_assign_%s_B%d_even_odd_median_ms" % (k, b)] = halves
    rec["note"] = "shared pool: neighbours move these numbers by several per cent; even / odd medians = the spread of one setting"
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
