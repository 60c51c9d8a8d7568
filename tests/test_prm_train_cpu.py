"""The PRM training head without a GPU (cim_amd.prm_train, csrc/prm_train.hip): the NumPy restatement
(tests/golden/prm_train_np.py) against the golden captured from the reference (make_golden_prm_train.py), against float64 and
against torch's own float64 operators within the bounds that follow from summation order, the header additions and the
host-side refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prm_train_cases as cases
import prm_train_np as ptn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
EPS = 2.0 ** -24
f32 = np.float32


@pytest.fixture(scope="module")
def golden():
    d = np.load(os.path.join(GOLDEN, "prm_train.npz"))
    return {k: d[k] for k in d.files}


@pytest.fixture(scope="module")
def restated():
    """shape -> the restatement on the crafted maps at factor 1 (computed once)."""
    return {shape: ptn.stimulate(cases.crafted_batch(shape), 1) for shape in cases.SHAPES}


def agg_bound(values, peaks, agg64):
    """2 ((P - 1) 2^-24 sum |v_q| / P + 2^-24 |agg|) per map (NaN where the map has no peak)."""
    p = peaks.sum((2, 3)).astype(np.float64)
    mag = np.where(peaks, np.abs(values.astype(np.float64)), 0.0).sum((2, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        return 2.0 * ((p - 1) * EPS * mag / p + EPS * np.abs(agg64))


# ---- contract 1: the peak set ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_peak_set_is_the_references(shape, golden, restated):
    key, res = "%dx%d" % shape, restated[shape]
    np.testing.assert_array_equal(ptn.peak_list(res["peaks"]), golden[key + "__peak_list"])
    counts = np.zeros((cases.BATCH, cases.CLASSES), dtype=np.int64)
    np.add.at(counts, (golden[key + "__peak_list"][:, 0], golden[key + "__peak_list"][:, 1]), 1)
    np.testing.assert_array_equal(res["count"], counts)
    maps = cases.crafted_batch(shape)
    finite = np.isfinite(maps).all((2, 3))
    np.testing.assert_array_equal(res["up"][finite], maps[finite])                              # factor 1: the identity on finite maps
    by_name = dict(zip(cases.MAP_NAMES, res["peaks"].reshape((-1,) + shape)))
    np.testing.assert_array_equal(np.argwhere(by_name["constant"]), [[0, 0]])
    np.testing.assert_array_equal(np.argwhere(by_name["signed_zeros"]), [[0, 0]])
    h, w = shape
    assert by_name["plateau"][1, 2] and by_name["plateau"][1:h - 1, 2:w - 1].sum() == 1        # of the plateau: its first pixel
    np.testing.assert_array_equal(np.argwhere(by_name["equal_maxima"]), [[1, 1], [h - 3, w - 2], [h - 1, 0]])
    assert by_name["checkerboard"].sum() == ((h + 1) // 2) * ((w + 1) // 2)
    assert by_name["corners_edges"].sum() == 8 and all(by_name["corners_edges"][y, x] for y in (0, h - 1) for x in (0, w - 1))
    status = dict(zip(cases.MAP_NAMES, res["status"].reshape(-1)))
    # the up-sampling turns a -inf tap into NaN (inf x 0, as ATen's does): through it a map of -inf reports the NaN; as a GIVEN map
    # it has no peak
    assert status["neg_inf"] == status["one_nan"] == ptn.STATUS_NAN and sum(status.values()) == 2 * ptn.STATUS_NAN
    assert not by_name["neg_inf"].any() and not by_name["one_nan"].any()
    pk, med, st = ptn.peak_map(cases.crafted(shape)["neg_inf"])
    assert not pk.any() and med == -np.inf and st == ptn.STATUS_NO_PEAK


# ---- contract 3: the restatement against the reference's golden and float64 -------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_aggregation_and_gradient_against_the_reference(shape, golden, restated):
    key, res, maps = "%dx%d" % shape, restated[shape], cases.crafted_batch(shape)
    ok = res["status"] == 0
    with np.errstate(invalid="ignore"):
        agg64 = np.where(res["peaks"], maps.astype(np.float64), 0.0).sum((2, 3)) / res["count"]
    bound = agg_bound(maps, res["peaks"], agg64)
    assert np.isnan(golden[key + "__agg"][~ok]).all() and np.isnan(res["agg"][~ok]).all() and (~ok).sum() == 2
    for got in (res["agg"], golden[key + "__agg"]):
        assert np.all(np.abs(got[ok].astype(np.float64) - agg64[ok]) <= bound[ok])
    # the reference's backward returns peak_map * grad_output (prm_modules.py:50): divided by the count it is the derivative
    g = cases.grad_output(shape)
    dcrm = ptn.backward(g, res["peaks"], shape[0], shape[1], 1)
    d64, k, mag = ptn.backward64(g, res["peaks"], shape[0], shape[1], 1)
    assert np.all((mag > 0) == (res["peaks"] & (g != 0)[:, :, None, None]))                    # factor 1: every other term has weight 0
    np.testing.assert_array_equal(golden[key + "__grad"][ok] != 0, (res["peaks"] & (g != 0)[:, :, None, None])[ok])
    ref = golden[key + "__grad"].astype(np.float64) / np.maximum(res["count"], 1)[:, :, None, None]
    for got in (dcrm.astype(np.float64)[ok], ref[ok]):
        assert np.all(np.abs(got - d64[ok]) <= 2 * (k[ok] + 2) * EPS * mag[ok])
    assert not dcrm[~ok].any()                                                                  # no peak: no gradient


@pytest.mark.parametrize("form", cases.UPSAMPLE_FORMS + cases.DYADIC_FORMS)
def test_restatement_against_float64(form):
    h, w, factor = form
    crm = cases.seeded_crm(h, w, 2, 3, 10 * h + w)
    bias = (np.arange(3) - 1).astype(f32) * f32(0.375)
    res = ptn.stimulate(crm, factor, bias)
    assert np.all(res["status"] == 0) and np.all(res["count"] >= 1)
    agg64 = np.where(res["peaks"], res["up"].astype(np.float64), 0.0).sum((2, 3)) / res["count"]
    assert np.all(np.abs(res["agg"].astype(np.float64) - agg64) <= agg_bound(res["up"], res["peaks"], agg64))
    g = (np.random.RandomState(3).randn(2, 3)).astype(f32)
    dcrm, dbias = ptn.backward(g, res["peaks"], h, w, factor, with_bias=True)
    d64, k, mag = ptn.backward64(g, res["peaks"], h, w, factor)
    assert np.all(np.abs(dcrm.astype(np.float64) - d64) <= 2 * (k + 2) * EPS * mag)
    n = 2 * h * w
    assert np.all(np.abs(dbias.astype(np.float64) - dcrm.astype(np.float64).sum((0, 2, 3))) <= 2 * n * EPS * np.abs(dcrm).astype(np.float64).sum((0, 2, 3)))
    np.testing.assert_array_equal(ptn.unpack_bits(ptn.pack_bits(res["peaks"]), h * factor, w * factor), res["peaks"])


@pytest.mark.parametrize("form", cases.DYADIC_FORMS)
def test_gradient_against_atens_interpolate_backward(form):
    """The second reference of the up-sampling's backward: torch's own F.interpolate(align_corners=True) backward in float64 on
    the dense gradient the peak map implies.  At these forms the scales (n - 1) / (factor n - 1) are dyadic, so the fp32 tap
    weights are exact and equal ATen's float64 ones: the two differ by the rounding of products and sums only, which is what
    the bound covers (elsewhere they also differ by the rounding of the fp32 scale, which no summation-order bound covers)."""
    h, w, factor = form
    crm = cases.seeded_crm(h, w, 2, 3, 77 + factor)
    res = ptn.stimulate(crm, factor)
    g = (np.random.RandomState(4).randn(2, 3)).astype(f32)
    dcrm = ptn.backward(g, res["peaks"], h, w, factor)
    _, k, mag = ptn.backward64(g, res["peaks"], h, w, factor)
    x = torch.from_numpy(crm).double().requires_grad_(True)
    up = F.interpolate(x, scale_factor=factor, mode="bilinear", align_corners=True) if factor > 1 else x * 1
    dense = torch.from_numpy(res["peaks"].astype(np.float64) * (g.astype(np.float64) / res["count"])[:, :, None, None])
    up.backward(dense)
    assert np.all(np.abs(dcrm.astype(np.float64) - x.grad.numpy()) <= 2 * (k + 2) * EPS * mag)
    assert np.abs(x.grad.numpy()).max() > 0


@pytest.mark.parametrize("name", list(cases.loss_cases()))
def test_loss_restatement_against_torch(name):
    x, t = cases.loss_cases()[name]
    loss, dagg = ptn.msm_loss(x, t)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    ref = F.multilabel_soft_margin_loss(xt, torch.from_numpy(t).double())
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    assert np.abs(dagg.astype(np.float64) - xt.grad.numpy()).max() <= 16 * EPS / x.size
    l64, d64 = ptn.msm_loss64(x, t)
    assert abs(l64 - float(ref)) <= 1e-12 * abs(float(ref)) and np.abs(d64 - xt.grad.numpy()).max() <= 1e-15
    assert np.isfinite(loss) and np.isfinite(dagg).all()


def test_exp_and_log1p_pieces():
    a = np.concatenate([np.linspace(0, 80, 4001), [80.0, 80.5, 100.0, 1e-8, 0.34657, 0.34658]]).astype(f32)
    e = ptn.exp_neg(a)
    want = np.exp(-a.astype(np.float64))
    assert np.all(np.abs(e - want) <= 4 * EPS * want + 2e-35)                                   # (beyond 80: 0 for 1.8e-35)
    u = np.concatenate([np.linspace(0, 1, 4001), [1e-30, 1e-8, 1.0]]).astype(f32)
    assert np.all(np.abs(ptn.log1p_unit(u) - np.log1p(u.astype(np.float64))) <= 4 * EPS * np.log1p(u.astype(np.float64)))


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
NEW = ("cim_prmt_stim_forward", "cim_prmt_stim_backward", "cim_prmt_msm_loss")


def test_header_declares_and_lib_binds_the_entries():
    from cim_amd import _lib, build
    build.build()
    lib = _lib.load()
    assert lib.cim_abi_version() == _lib.ABI_VERSION == 16                                      # additive
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name]
        assert _lib.FUNCTIONS[name][0] is ctypes.c_int and name not in _lib.VALUE_RETURNING
    assert 12544 <= _lib.CONSTANTS["CIM_PRM_STIM_MAX_HW"] == 16384
    # the map (4 bytes a pixel), the histogram, the reduction buffer: twice in a CU's 160 KiB of LDS
    assert 2 * (4 * _lib.CONSTANTS["CIM_PRM_STIM_MAX_HW"] + 4096) <= 160 * 1024
    assert os.path.join(build.CSRC, "prm_train.hip") in build.sources()
    assert (ptn.STATUS_NAN, ptn.STATUS_NO_PEAK) == (_lib.CONSTANTS["CIM_PRM_STATUS_NAN"], _lib.CONSTANTS["CIM_PRM_STATUS_NO_PEAK"])


def test_entries_refuse_on_the_host():
    """Sizes and pointers are validated before any launch (the pointers here are not device pointers: a launch would not survive
    them)."""
    from cim_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(64)
    fwd = lambda b, c, h, w, f, crm=fake, out=fake: lib.cim_prmt_stim_forward(crm, None, b, c, h, w, f, out, fake, fake, fake, fake, None)
    bwd = lambda b, c, h, w, f, g=fake, out=fake: lib.cim_prmt_stim_backward(g, fake, fake, b, c, h, w, f, out, None, None)
    for entry in (fwd, bwd):
        for args in ((0, 3, 2, 3, 8), (2, 0, 2, 3, 8), (2, 3, 2, 3, 0), (2, 3, 2, 3, -1), (2, 3, 0, 3, 8), (2, 3, 2, 0, 8), (-1, 3, 2, 3, 8)):
            assert entry(*args) == -1 and b"factor >= 1" in lib.cim_last_error(), args
        assert entry(1, 1, 16, 17, 8) == -1 and b"CIM_PRM_STIM_MAX_HW" in lib.cim_last_error()      # 128 x 136 > 16384
        assert entry(1, 1, 129, 128, 1) == -1 and b"129 x 128" in lib.cim_last_error()             # 16512 pixels at factor 1
        assert entry(1 << 13, 1 << 12, 2, 3, 8) == -1 and b"maps" in lib.cim_last_error()
        assert entry(2, 3, 2, 3, 8, None) == -1 and entry(2, 3, 2, 3, 8, fake, None) == -1
    assert b"cim_prmt_stim_backward" in lib.cim_last_error()
    loss = lambda b, c, x=fake, t=fake, l=fake, d=fake: lib.cim_prmt_msm_loss(x, t, b, c, l, d, None)
    assert loss(0, 3) == -1 and loss(3, 0) == -1 and loss(1 << 13, 1 << 12) == -1
    assert loss(2, 3, None) == -1 and loss(2, 3, fake, None) == -1 and loss(2, 3, fake, fake, None) == -1
    assert loss(2, 3, fake, fake, fake, None) == -1 and b"cim_prmt_msm_loss" in lib.cim_last_error()


def test_python_entry_rejects_cpu_tensors_and_bad_arguments():
    from cim_amd import _lib, prm, prm_train
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        prm_train.peak_stimulation(torch.zeros(1, 2, 3, 4))
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        prm_train.multilabel_soft_margin_loss(torch.zeros(1, 2), torch.zeros(1, 2))
    model = prm.PeakResponseMapping(prm.fc_resnet50(3, width=4))
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        prm_train.loss(model, torch.zeros(1, 3, 32, 32), torch.zeros(1, 3))
    with pytest.raises(ValueError, match="one of 2, 3, 4, 5"):
        prm_train.freeze(model, at=1)
    with pytest.raises(TypeError):
        prm_train.freeze(torch.nn.Sequential())


@pytest.mark.parametrize("at", [2, 3, 4, 5])
def test_freeze_stops_at_the_named_stage(at):
    from cim_amd import prm, prm_train
    model = prm_train.freeze(prm.PeakResponseMapping(prm.fc_resnet50(3, width=4)), at=at)
    trained = {k.split(".")[2] for k, p in model.named_parameters() if p.requires_grad and k.startswith("0.features.")}
    assert trained == {str(i) for i in range(3 + at, 8)}                                        # features.4 = layer1
    assert all(p.requires_grad for p in model[0].classifier.parameters())
    assert list(model.state_dict()) == list(prm.PeakResponseMapping(prm.fc_resnet50(3, width=4)).state_dict())
