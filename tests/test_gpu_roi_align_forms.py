"""-m gpu: every ROIAlign kernel form of csrc/roi_align.hip against the oracle, at shapes that reach it.

Each case first asks the library which forms it takes (cim_roi_align_forms), so that a changed threshold cannot move a case to
another form unnoticed.  Then the forward, plain and mask-cat, against oracle/roi_align_ref.c: bit-identical in the reference's
sample order (EXACT, and the default where the form is sample-order), within 1e-6 max|feat| for the table forms.  Then the
backward against the fp64 oracle by three routes: autograd after the default forward (the backward is told the forward's tables
are ready), the C entry point building its own tables, and the C entry point without partial-map scratch where there are
several ROI groups.  Every case's ROIs include the full image, a box smaller than one map pixel, one outside the map, one
partly at negative coordinates, an unclipped box larger than the map, a zero-size box and strips along the left and right
border (x in [-0.5, 0] and [W - 1, W - 0.1] in map pixels, three map heights tall)."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from cim_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _rois(rng, B, H, W, K, scale, extra=()):
    s = 1.0 / scale                                        # input-image pixels per map pixel
    Wi, Hi = W * s, H * s
    fixed = [(0, 0, Wi, Hi),                               # the full image
             (40, 40, 40.5, 40.25),                        # smaller than one map pixel
             (Wi + 500, 10, Wi + 900, 200),                # outside the map
             (-3 * s, -2 * s, 5 * s, 4 * s),               # partly at negative coordinates
             (-0.5 * Wi, -0.5 * Hi, 1.5 * Wi, 1.5 * Hi),   # unclipped, larger than the map
             (4 * s, 3 * s, 4 * s, 3 * s),                 # zero size
             (0, -Hi, 0.5 * s, 2 * Hi),                    # left border strip
             ((W - 0.5) * s, -Hi, (W + 0.4) * s, 2 * Hi)]  # right border strip
    fixed += list(extra)
    n = K - len(fixed)
    assert n >= 0
    x1, y1 = rng.uniform(-2 * s, Wi * 0.8, n), rng.uniform(-2 * s, Hi * 0.8, n)
    boxes = np.concatenate([np.array(fixed, np.float64).reshape(-1, 4),
                            np.stack([x1, y1, x1 + rng.uniform(1, Wi, n), y1 + rng.uniform(1, Hi, n)], 1)])
    return np.concatenate([rng.randint(0, B, (K, 1)), boxes], 1).astype(np.float32)


def _table_support(roi, P, H, W, scale, sr, aligned):
    """The map rows of every bin row and the map columns of every bin column with a non-zero table weight, as roi_tables_kernel
    builds the tables (fp32 sample positions, the bilinear clamp of make_tap): -> (rows[P] sets, cols[P] sets)."""
    f = np.float32
    off = f(0.5) if aligned else f(0.0)
    x1, y1 = f(roi[1]) * f(scale) - off, f(roi[2]) * f(scale) - off
    rw, rh = f(roi[3]) * f(scale) - off - x1, f(roi[4]) * f(scale) - off - y1
    if not aligned:
        rw, rh = max(rw, f(1.0)), max(rh, f(1.0))

    def axis(start, extent, size):
        bin_ = extent / f(P)
        n = sr if sr > 0 else int(np.ceil(extent / f(P)))
        out = []
        for p in range(P):
            support = set()
            for i in range(n):
                v = start + f(p) * bin_ + (f(i) + f(0.5)) * bin_ / f(n)
                if v < -1.0 or v > size:
                    continue
                v = max(v, f(0.0))
                lo = int(v)
                if lo >= size - 1:
                    support.add(size - 1)
                    continue
                support.add(lo)                            # weight 1 - l > 0
                if v - f(lo) != 0.0:
                    support.add(lo + 1)
            out.append(support)
        return out

    return axis(y1, rh, H), axis(x1, rw, W)


def _agg_overflow(rois, P, H, W, scale, sr, aligned):
    """(most rows in one bin row, most (row, column) entries in one bin) over the ROIs: what roi_align_fwd_agg_kernel counts
    against its 64-entry lists (columns as the span of the non-zero ones)."""
    most_rows = most_entries = 0
    for roi in rois:
        rows, cols = _table_support(roi, P, H, W, scale, sr, aligned)
        nx = [max(c) - min(c) + 1 if c else 0 for c in cols]
        for r in rows:
            most_rows = max(most_rows, len(r))
            most_entries = max(most_entries, len(r) * max(nx))
    return most_rows, most_entries


# B, C, H, W, K, P, scale, sampling_ratio, aligned, forward form, backward form
CASES = [
    pytest.param(2, 64, 112, 150, 40, 7, 1 / 8, 0, True, "AGG", "REGION", id="vgg16_1200_landscape"),
    pytest.param(2, 64, 150, 112, 40, 7, 1 / 8, 0, True, "SAMPLE4", "REGION", id="vgg16_1200_portrait"),
    pytest.param(1, 64, 33, 43, 40, 14, 1 / 16, 0, True, "SAMPLE4", "REGION", id="config_default_P14"),
    pytest.param(1, 64, 33, 43, 40, 16, 1 / 16, 0, True, "SAMPLE4", "REGION", id="P16"),
    pytest.param(1, 64, 33, 43, 40, 17, 1 / 16, 0, True, "SAMPLE4", "GENERIC4", id="P17"),
    pytest.param(1, 32, 64, 40, 40, 8, 1 / 16, 0, True, "AGG", "REGION", id="P8_64x40"),
    pytest.param(2, 32, 128, 40, 40, 8, 1 / 16, 0, True, "AGG", "REGION", id="P8_128x40"),
    pytest.param(1, 8, 128, 40, 24, 8, 1 / 16, 0, True, "AGG", "REGION", id="tall_strip"),
    pytest.param(2, 16, 40, 50, 96, 1, 1 / 16, 0, True, "ROWSUM2", "REGION", id="P1_40x50"),
    pytest.param(2, 16, 40, 50, 96, 2, 1 / 16, 0, True, "ROWSUM2", "REGION", id="P2_40x50"),
    pytest.param(2, 16, 40, 50, 96, 3, 1 / 16, 0, True, "ROWSUM2", "REGION", id="P3_40x50"),
    pytest.param(2, 16, 100, 50, 96, 1, 1 / 16, 0, True, "SAMPLE4", "REGION", id="P1_100x50"),
    pytest.param(2, 16, 100, 50, 96, 2, 1 / 16, 0, True, "SAMPLE4", "REGION", id="P2_100x50"),
    pytest.param(2, 16, 100, 50, 96, 3, 1 / 16, 0, True, "SAMPLE4", "REGION", id="P3_100x50"),
    pytest.param(1, 16, 128, 129, 40, 4, 1 / 16, 0, True, "AGG", "REGION", id="W129"),
    pytest.param(1, 8, 64, 40, 96, 7, 1 / 16, 0, True, "ROWSUM2", "REGION", id="H64"),
    pytest.param(1, 8, 65, 40, 96, 7, 1 / 16, 0, True, "ROWSUM2", "REGION", id="H65"),
    pytest.param(1, 8, 128, 40, 96, 7, 1 / 16, 0, True, "ROWSUM2", "REGION", id="H128"),
    pytest.param(1, 8, 129, 40, 96, 7, 1 / 16, 0, True, "SAMPLE4", "REGION", id="H129"),
    pytest.param(1, 8, 255, 40, 96, 7, 1 / 16, 0, True, "SAMPLE4", "REGION", id="255x40"),
    pytest.param(1, 8, 256, 40, 40, 7, 1 / 16, 0, True, "SAMPLE4", "GENERIC4", id="256x40"),
    pytest.param(1, 8, 255, 255, 40, 7, 1 / 16, 0, True, "SAMPLE4", "GENERIC4", id="255x255"),
    pytest.param(2, 3, 33, 43, 40, 7, 1 / 16, 0, True, "SAMPLE1", "GENERIC1", id="C3"),
    pytest.param(1, 6, 33, 43, 40, 7, 1 / 16, 0, True, "SAMPLE1", "GENERIC1", id="C6"),
    pytest.param(1, 516, 33, 43, 40, 7, 1 / 16, 0, True, "ROWSUM2", "REGION", id="C516"),
    pytest.param(2, 16, 100, 50, 96, 3, 1 / 16, 2, True, "SAMPLE4", "REGION", id="sr2_aligned"),
    pytest.param(1, 16, 40, 129, 40, 5, 1 / 16, 2, False, "AGG", "REGION", id="sr2_unaligned"),
    pytest.param(2, 16, 45, 60, 96, 7, 1 / 16, 0, False, "ROWSUM2", "REGION", id="sr0_unaligned"),
]


@pytest.mark.parametrize("B,C,H,W,K,P,scale,sr,aligned,fwd,bwd", CASES)
def test_roi_align_form_vs_oracle(dev, B, C, H, W, K, P, scale, sr, aligned, fwd, bwd, request, monkeypatch):
    from cim_amd import _lib
    from oracle import roi_align as oracle
    RA = importlib.import_module("cim_amd.ops.roi_align")
    name = request.node.callspec.id
    fwd, bwd = getattr(RA, "FWD_" + fwd), getattr(RA, "BWD_" + bwd)
    table_forms = (RA.FWD_ROWSUM2, RA.FWD_AGG)
    rng = np.random.RandomState(sum(map(ord, name)))
    extra = [(0, 0, 8, 10240)] if name == "tall_strip" else []     # map x in [-0.5, 0], 640 map rows: one column, 80-row bins
    rois = _rois(rng, B, H, W, K, scale, extra)

    # (a) the case reaches its forms, plain and mask-cat, after the default forward
    for maskcat in (False, True):
        assert RA.forms(B, C, H, W, K, P, maskcat) == (fwd, bwd, bwd == RA.BWD_REGION and fwd not in table_forms)
    if name == "vgg16_1200_landscape":       # bins beyond the entry-list kernel's 64 entries: its sample-order fallback runs
        assert _agg_overflow(rois, P, H, W, scale, sr, aligned)[1] > 64
    if name == "tall_strip":                 # a bin row of more than 64 rows in a single column
        rows, cols = _table_support(rois[8], P, H, W, scale, sr, aligned)
        assert [len(c) for c in cols] == [1] * P and len(rows[0]) > 64

    # (b) forward
    feat = rng.randn(B, C, H, W).astype(np.float32)
    masks = (rng.rand(K, P, P) > 0.4).astype(np.float32)
    ref = oracle.roi_align_fwd(feat, rois, P=P, scale=scale, sampling_ratio=sr, aligned=aligned)
    ref_cat = np.concatenate([ref, ref * masks[:, None]], 1)
    x = torch.from_numpy(feat).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    r_d, m_d = torch.from_numpy(rois).to(dev), torch.from_numpy(masks).to(dev)
    for exact in (True, False):
        monkeypatch.setattr(RA, "EXACT", exact)
        out = RA.roi_align(x, r_d, P, scale, sr, "avg", aligned)
        cat = RA.roi_align_maskcat(x, r_d, m_d, P, scale, sr, aligned)
        assert out.shape == (K, C, P, P) and cat.shape == (K, 2 * C, P, P)
        for got, want, what in ((out, ref, "plain"), (cat, ref_cat, "mask-cat")):
            got = got.detach().cpu().numpy()
            if exact or fwd not in table_forms:
                np.testing.assert_array_equal(got, want, err_msg="%s forward, EXACT=%s" % (what, exact))
            else:
                np.testing.assert_allclose(got, want, rtol=0, atol=1e-6 * float(np.abs(feat).max()), err_msg=what + " forward")

    # (c) backward (out / cat: the default forward's)
    go = rng.randn(K, C, P, P).astype(np.float32)
    gref = oracle.roi_align_bwd(go, rois, feat.shape, P=P, scale=scale, sampling_ratio=sr, aligned=aligned)
    tol = dict(rtol=1e-4, atol=1e-4 * max(1.0, K / 300.0))
    out.backward(torch.from_numpy(go).to(dev))
    np.testing.assert_allclose(x.grad.cpu().numpy(), gref, err_msg="autograd, plain", **tol)
    x.grad = None
    m4 = masks[:, None]
    cat.backward(torch.from_numpy(np.concatenate([go * (1 - m4), go * m4], 1)).to(dev))     # g_lo + mask g_hi == go exactly
    np.testing.assert_allclose(x.grad.cpu().numpy(), gref, err_msg="autograd, mask-cat", **tol)
    go_nhwc = torch.from_numpy(go).to(dev).permute(0, 2, 3, 1).contiguous()
    ws = torch.zeros_like(RA._workspace(K, P, H, W, dev))
    scratch = RA._scratch(K, B, C, H, W, dev)
    routes = [(scratch, "tables built by the backward")]
    if scratch is not None:                                                # several ROI groups
        routes.append((None, "no scratch: the ROI groups meet through atomics"))
    for s, what in routes:
        gin = torch.full((B, H, W, C), float("nan"), device=dev)         # fully overwritten by the call
        _lib.call("cim_roi_align_bwd_ws", go_nhwc.data_ptr(), r_d.data_ptr(), gin.data_ptr(), B, C, H, W, K, P, scale, sr,
                  int(aligned), ws.data_ptr(), 0, _lib.ptr(s), _lib.stream_ptr())
        np.testing.assert_allclose(gin.permute(0, 3, 1, 2).cpu().numpy(), gref, err_msg=what, **tol)
