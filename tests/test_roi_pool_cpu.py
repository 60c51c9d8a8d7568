"""RoIPool without a GPU: the NumPy restatement (tests/golden/roi_pool_np.py) against an independent
formulation, the case table against what it claims to hold, the header and the binding, the operator's constructor, every
refusal of the C entry points (they return before any device work) and MaskFuse's dispatch."""
import ctypes

import numpy as np
import pytest
import torch

import roi_pool_np as rp

ENTRIES = ("cim_roi_pool_fwd", "cim_roi_pool_maskcat_fwd", "cim_roi_pool_bwd_scratch", "cim_roi_pool_bwd", "cim_roi_pool_maskcat_bwd")


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,scale", rp.A_VARIANTS)
def test_restatement_against_amax_and_autograd(P, scale):
    """Tie-free float64 data (held exactly by float32): per non-empty bin `x[b, :, y0:y1, x0:x1].amax((1, 2))` through torch
    autograd gives the restatement's values and its grad_in."""
    B, H, W = rp.A_SHAPE
    C = 5
    rs = np.random.RandomState(P)
    feat = rs.permutation(B * C * H * W).reshape(B, C, H, W).astype(np.float32) / 8 - 30           # all different
    out, arg = rp.forward(feat, rp.A_ROIS, P, scale)
    dy = rs.standard_normal(out.shape)
    grad, n, mag = rp.backward(dy, arg, rp.A_ROIS, feat.shape)

    x = torch.from_numpy(feat).double().requires_grad_(True)
    want = torch.zeros(out.shape, dtype=torch.float64)
    filled = np.zeros(out.shape, bool)
    for k, roi in enumerate(rp.A_ROIS):
        bn = rp.bins(roi, scale, P, H, W)
        if bn is None:
            continue
        ylo, yhi, xlo, xhi = bn
        for ph in range(P):
            for pw in range(P):
                if yhi[ph] > ylo[ph] and xhi[pw] > xlo[pw]:
                    want[k, :, ph, pw] = x[int(roi[0]), :, ylo[ph]:yhi[ph], xlo[pw]:xhi[pw]].amax((1, 2))
                    filled[k, :, ph, pw] = True
    (want * torch.from_numpy(dy)).sum().backward()
    assert np.array_equal(out.astype(np.float64), want.detach().numpy())
    assert np.array_equal(arg >= 0, filled)
    np.testing.assert_allclose(grad, x.grad.numpy(), rtol=0, atol=1e-12)
    assert int(n.sum()) == int(filled.sum()) and np.all(mag >= np.abs(grad) - 1e-12)


@pytest.mark.parametrize("kind", ["normal", "ints", "special"])
def test_restatement_against_the_scan_written_out(kind):
    """The channel-wise form against one comparison per pixel; on integers the winner is the first maximum in row-major order;
    -inf / NaN alone give -FLT_MAX with -1, NaN amid numbers is passed over."""
    B, H, W = rp.A_SHAPE
    feat = rp.seeded_feat((B, 6, H, W), 3, kind)
    for P, scale in rp.A_VARIANTS[:3]:
        out, arg = rp.forward(feat, rp.A_ROIS, P, scale)
        out2, arg2 = rp.forward_scan(feat, rp.A_ROIS, P, scale)
        assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)) and np.array_equal(arg, arg2)
    out, arg = rp.forward(feat, rp.A_ROIS, 7, 1 / 16.0)
    assert not np.isnan(out).any()
    if kind == "ints":
        ties = 0
        for k, roi in enumerate(rp.A_ROIS):
            bn = rp.bins(roi, 1 / 16.0, 7, H, W)
            if bn is None:
                continue
            ylo, yhi, xlo, xhi = bn
            for ph in range(7):
                for pw in range(7):
                    for c in range(6):
                        win = feat[int(roi[0]), c, ylo[ph]:yhi[ph], xlo[pw]:xhi[pw]]
                        if win.size == 0:
                            continue
                        first = np.flatnonzero(win.reshape(-1) == win.max())
                        ties += len(first) > 1
                        y, x = divmod(int(first[0]), win.shape[1])
                        assert arg[k, c, ph, pw] == (ylo[ph] + y) * W + xlo[pw] + x
        assert ties > 50
    if kind == "special":
        lost = out == -rp.FLT_MAX
        assert lost.sum() > 100 and np.all(arg[lost] == -1)
        assert lost[5, 1].all() and not lost[5, 0].any()               # the one-pixel box on the NaN pixel of image 1, channel 1
        assert not np.any(arg[0, 0] == 4 * W + 5)                      # the NaN amid numbers is never the winner


def test_case_table_holds_what_it_claims():
    B, H, W = rp.A_SHAPE
    assert rp.A_ROIS.shape == (8, 5) and set(rp.A_ROIS[:, 0]) == {0.0, 1.0}
    assert rp.census(rp.A_ROIS, 1 / 16.0, 7, H, W)[:3] == (1, 82, 343)
    assert rp.bins(rp.A_ROIS[4], 1 / 16.0, 7, H, W) is None                                     # the malformed one
    # the box at the far corner: at 1/16 it starts inside the last pixel (8.125, 6.25) - four bins of that one pixel, 45 empty -
    # and at 1/8 it lies beyond the map: every bin empty
    ylo, yhi, xlo, xhi = rp.bins(rp.A_ROIS[3], 1 / 16.0, 7, H, W)
    area = (yhi - ylo)[:, None] * (xhi - xlo)[None, :]
    assert int((area > 0).sum()) == 4 and int(area.max()) == 1 and ylo[0] == H - 1 and xlo[0] == W - 1
    ylo, yhi, xlo, xhi = rp.bins(rp.A_ROIS[3], 1 / 8.0, 7, H, W)
    assert np.all((yhi - ylo)[:, None] * (xhi - xlo)[None, :] <= 0)
    ylo, yhi, xlo, xhi = rp.bins(rp.A_ROIS[1], 1 / 16.0, 7, H, W)                               # bins smaller than a pixel overlap
    assert np.all(xhi - xlo <= 2) and len(set(xlo)) == 2 and np.all(xlo[1:] < xhi[:-1])        # (7 bins over 2 pixels: neighbours share one)
    ylo, yhi, xlo, xhi = rp.bins(rp.A_ROIS[2], 1 / 16.0, 7, H, W)                               # clipped at 0
    assert xlo[0] == 0 and xhi[0] == 0 and ylo[0] == 0
    ylo, yhi, xlo, xhi = rp.bins(rp.A_ROIS[0], 1 / 16.0, 7, H, W)                               # past the edge: clamped to W / H
    assert xhi[-1] == W and yhi[-1] == H
    for P, scale in rp.A_VARIANTS:
        bad, empty, total, largest = rp.census(rp.A_ROIS, scale, P, H, W)
        assert bad == 1 and total == 7 * P * P and empty < total and largest >= 4
    assert sorted(set(P for P, _ in rp.A_VARIANTS)) == [1, 7, 14] and sorted(set(s for _, s in rp.A_VARIANTS)) == [1 / 32.0, 1 / 16.0, 1 / 8.0]
    assert rp.A_CHANNELS == (8, 6)
    rois = rp.b_rois()
    bad, empty, total, largest = rp.census(rois, rp.B_SCALE, rp.B_P, *rp.B_SHAPE[1:])
    assert rois.shape == (24, 5) and bad == 0 and total == 24 * 49 and 0 < empty < total // 2 and largest == 6 * 7


# ---- header, binding, operator ----------------------------------------------------------------------------------------------------
def test_header_and_binding():
    from cim_amd import _lib
    assert _lib.ABI_VERSION == 16 and len(_lib.STRUCTS) == 8
    for name in ENTRIES:
        assert name in _lib.FUNCTIONS, name
    assert _lib.FUNCTIONS["cim_roi_pool_bwd_scratch"][0] is ctypes.c_longlong and "cim_roi_pool_bwd_scratch" in _lib.VALUE_RETURNING
    assert all(_lib.FUNCTIONS[n][0] is ctypes.c_int and n not in _lib.VALUE_RETURNING for n in ENTRIES if n != "cim_roi_pool_bwd_scratch")
    lib = _lib.load()
    assert lib.cim_abi_version() == 16
    # the scratch is a function of the shape alone: 0 for one group, whole maps otherwise
    assert lib.cim_roi_pool_bwd_scratch(0, 1, 8, 7, 9, 7) == 0 and lib.cim_roi_pool_bwd_scratch(3, 1, 8, 7, 9, 7) == 0
    nbytes = lib.cim_roi_pool_bwd_scratch(24, 1, 64, 33, 43, 7)
    assert nbytes > 0 and nbytes % (4 * 64 * 33 * 43) == 0
    assert lib.cim_roi_pool_bwd_scratch(24, 0, 64, 33, 43, 7) == -1 and b"cim_roi_pool_bwd_scratch" in lib.cim_last_error()


def test_operator_names_and_constructor():
    from cim_amd import _lib, ops
    from cim_amd.modeling import model_builder
    assert {"RoIPool", "roi_pool", "roi_pool_maskcat", "nms", "soft_nms"} <= set(ops.__all__)
    assert model_builder.RoIPool is ops.RoIPool and issubclass(ops.RoIPool, torch.nn.Module)
    m = ops.RoIPool(7, 1 / 16.)
    assert m.output_size == (7, 7) and m.spatial_scale == 0.0625
    assert repr(m) == "RoIPool(output_size=(7, 7), spatial_scale=0.0625)"
    with pytest.raises(ValueError, match="square"):
        ops.RoIPool((7, 5))
    with pytest.raises(NotImplementedError):
        ops.nms()
    x, rois = torch.zeros(1, 4, 7, 9), torch.tensor([[0., 0., 0., 15., 15.]])
    with pytest.raises(_lib.CimHipError, match="roi_pool"):
        m(x, rois)
    with pytest.raises(_lib.CimHipError, match="roi_pool"):
        ops.roi_pool_maskcat(x, rois, torch.ones(1, 7, 7), 7, 1 / 16.)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
_ORDER = {
    "cim_roi_pool_fwd": ("feat", "rois", "out", "argmax", "B", "C", "H", "W", "K", "P", "scale"),
    "cim_roi_pool_maskcat_fwd": ("feat", "rois", "masks", "out", "argmax", "B", "C", "H", "W", "K", "P", "scale"),
    "cim_roi_pool_bwd": ("grad", "rois", "argmax", "grad_in", "B", "C", "H", "W", "K", "P", "scale", "scratch"),
    "cim_roi_pool_maskcat_bwd": ("grad", "rois", "masks", "argmax", "grad_in", "B", "C", "H", "W", "K", "P", "scale", "scratch"),
}
_POINTERS = ("feat", "rois", "masks", "out", "argmax", "grad", "grad_in", "scratch")
REFUSED = [(entry, {p: None}, p) for entry, order in _ORDER.items() for p in order
           if p in _POINTERS and not (p == "argmax" and entry.endswith("fwd"))]
REFUSED += [(entry, {d: 0}, d) for entry in _ORDER for d in ("B", "C", "H", "W", "P")]
REFUSED += [(entry, {"K": -1}, "K >= 0") for entry in _ORDER]
REFUSED += [(entry, {"H": 65536, "W": 32768}, "H * W") for entry in _ORDER]
REFUSED += [(entry, {"K": 2 ** 20, "C": 2 ** 11 // (2 if "maskcat" in entry else 1), "P": 1}, "K * P * P") for entry in _ORDER]
REFUSED += [(entry, {"K": 2 ** 17, "C": 2 ** 8 // (2 if "maskcat" in entry else 1), "P": 8}, "K * P * P") for entry in _ORDER]


@pytest.mark.parametrize("entry,over,names", REFUSED, ids=["%s-%s" % (e[8:], "-".join("%s=%s" % kv for kv in o.items())) for e, o, _ in REFUSED])
def test_refusals_return_before_device_work(entry, over, names):
    """Null pointers (a NULL argmax in the forward is inference, not an error), a dimension below 1, K < 0, H W or the output's
    element count at 2^31: -1 and a message naming the entry and the argument.  No GPU is touched: this runs on a machine
    without one, with host addresses standing in for device pointers."""
    from cim_amd import _lib
    lib = _lib.load()
    room = (ctypes.c_float * 16)()
    a = dict(B=1, C=8, H=7, W=9, K=24, P=7, scale=1 / 16.0)         # (K 24: several ROI groups, so the scratch is needed)
    a.update({p: ctypes.addressof(room) for p in _POINTERS})
    if entry.endswith("bwd"):
        a["C"], a["H"], a["W"] = 64, 33, 43
    a.update(over)
    rc = getattr(lib, entry)(*(a[k] for k in _ORDER[entry]), None)
    msg = lib.cim_last_error().decode()
    assert rc == -1 and msg.startswith(entry + ":") and names in msg, msg


def test_null_argmax_in_the_forward_is_not_a_refusal():
    """... checked where no launch follows: K == 0 succeeds with every per-ROI pointer NULL."""
    from cim_amd import _lib
    room = (ctypes.c_float * 16)()
    p = ctypes.addressof(room)
    _lib.call("cim_roi_pool_fwd", p, None, None, None, 1, 8, 7, 9, 0, 7, 1 / 16.0, None)
    _lib.call("cim_roi_pool_maskcat_fwd", p, None, None, None, None, 1, 8, 7, 9, 0, 7, 1 / 16.0, None)


# ---- MaskFuse ---------------------------------------------------------------------------------------------------------------------
def test_maskfuse_dispatches_on_the_method():
    from cim_amd import _lib
    from cim_amd.core.config import cfg
    from cim_amd.core.presets import apply_preset
    from cim_amd.modeling.maskfuse import MaskFuse
    apply_preset("resnet50_voc")
    before = cfg.FAST_RCNN.ROI_XFORM_METHOD
    assert before == "RoIAlign"
    head = MaskFuse(64, None, 1 / 16.0)
    x, rois, masks = torch.zeros(1, 64, 7, 9), torch.tensor([[0., 0., 0., 15., 15.]]), torch.ones(1, 7, 7)
    try:
        cfg.FAST_RCNN.ROI_XFORM_METHOD = "RoIPoolF"
        with pytest.raises(_lib.CimHipError, match="roi_pool"):         # the operator's refusal of CPU tensors: the method is served
            head(x, rois, masks)
        cfg.FAST_RCNN.ROI_XFORM_METHOD = "RoICrop"
        with pytest.raises(NotImplementedError, match="RoICrop") as e:
            head(x, rois, masks)
        assert "RoIPoolF" not in str(e.value)
    finally:
        cfg.FAST_RCNN.ROI_XFORM_METHOD = before
