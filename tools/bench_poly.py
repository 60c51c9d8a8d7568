#!/usr/bin/env python3
"""Time of the device polygon fill (cim_amd.segm_eval.poly_masks, csrc/poly_fill.hip) at 480 x 640 with 40 annotations and at
375 x 500 with 10 annotations (seeded polygons of tests/golden/poly_cases.py: 1-4 polygons of 3-60 vertices each), against
  * `cim_segm_rle_decode` of the same masks in the same run - the existing way ground truth reaches the evaluator, and
  * the NumPy restatement tests/golden/poly_np.py on one CPU thread - a stated baseline, not credited as a speed-up.

    python tools/bench_poly.py [--reps 20]

Device times: HIP events around the C entry point alone (its two memsets and two launches; inputs already on the device)
and around the whole `poly_masks` / `rle_decode` call (host array work and uploads included), warm, median of --reps.
The masks are checked bit for bit against the restatement first.  Prints one JSON line per shape.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))

from cim_amd import _lib, build, segm_eval  # noqa: E402

SHAPES = ((480, 640, 40), (375, 500, 10))


def event_ms(fn, reps):
    """Median of `reps` event-timed calls after three warm ones."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    import poly_cases
    import poly_np as pn
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_poly: needs the GPU (no CPU timing is reported)")
    build.build()
    torch.set_num_threads(1)
    dev = torch.device("cuda", torch.cuda.current_device())
    for h, w, n in SHAPES:
        anns = poly_cases.random_scene(np.random.RandomState(h + n), h, w, n, max_polys=4, kmin=3, kmax=60)
        t0 = time.perf_counter()
        want = pn.annotation_masks(anns, h, w)
        host_ms = (time.perf_counter() - t0) * 1e3
        packed = segm_eval.poly_masks(anns, h, w, dev)
        bits = np.unpackbits(packed.cpu().numpy().view(np.uint8).reshape(n, -1), axis=1, bitorder="little")
        same = bool(np.array_equal(bits[:, :h * w].reshape(n, w, h).transpose(0, 2, 1), want)) and not bits[:, h * w:].any()
        counts, off = segm_eval.rle_counts(packed, h, w)
        rles = [{"size": [h, w], "counts": counts[off[i]:off[i + 1]].tolist()} for i in range(n)]
        assert torch.equal(segm_eval.rle_decode(rles, dev)[0], packed)

        # the C entry points alone, inputs resident
        xy, poly_off, poly_ann, edge_off, total = segm_eval._polygon_arrays(anns, h, w)
        d = [torch.from_numpy(a).to(dev) for a in (xy, poly_off, poly_ann, edge_off)]
        ws = torch.empty(_lib.call("cim_poly_ws_bytes", len(poly_ann), h, w), dtype=torch.uint8, device=dev)
        out = torch.empty_like(packed)
        fill = lambda: _lib.call("cim_poly_fill", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), len(poly_ann),
                                 xy.size // 2, total, n, h, w, ws.data_ptr(), out.data_ptr(), _lib.stream_ptr())
        lens = np.diff(off)
        c_d = torch.from_numpy(counts.view(np.int32).copy()).to(dev)
        off_d, len_d = torch.from_numpy(off[:-1].copy()).to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev)
        ws2 = torch.empty(_lib.call("cim_segm_rle_decode_ws_bytes", int(off[-1])), dtype=torch.uint8, device=dev)
        out2 = torch.empty_like(packed)
        decode = lambda: _lib.call("cim_segm_rle_decode", c_d.data_ptr(), off_d.data_ptr(), len_d.data_ptr(), n, h, w, ws2.data_ptr(),
                                   out2.data_ptr(), _lib.stream_ptr())
        res = {"shape": "%dx%d" % (h, w), "annotations": n, "polygons": int(len(poly_ann)), "vertices": int(xy.size // 2),
               "dense_points": total, "rle_counts": int(off[-1]), "bit_identical": same,
               "poly_fill_ms": round(event_ms(fill, args.reps), 4), "rle_decode_ms": round(event_ms(decode, args.reps), 4),
               "poly_masks_call_ms": round(event_ms(lambda: segm_eval.poly_masks(anns, h, w, dev), args.reps), 4),
               "rle_decode_call_ms": round(event_ms(lambda: segm_eval.rle_decode(rles, dev), args.reps), 4),
               "restatement_host_ms": round(host_ms, 2)}
        assert torch.equal(out, packed) and torch.equal(out2, packed)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
