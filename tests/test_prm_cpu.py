"""The PRM peak path without a GPU (cim_amd.prm, csrc/prm.hip): the NumPy restatement (tests/golden/prm_np.py)
against every golden captured from the reference (make_golden_prm.py), the lower median against np.partition, the integer point
scaling against the reference's float64 expression, the header additions, and the network's modules on the CPU (state_dict keys,
strict load, class response maps through the ATen branch of the wrappers)."""
import os
import re

import numpy as np
import pytest
import torch

import prm_cases
import prm_np
import proposal_prep_np as ppn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
FACTOR = 8


def load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: d[k] for k in d.files}


def thin_model(golden):
    """cim_amd's PeakResponseMapping at width 16 with the weights the golden's seed gives (regenerated, as the maker does)."""
    from cim_amd import prm
    model = prm.PeakResponseMapping(prm.fc_resnet50(prm_cases.NUM_CLASSES, width=prm_cases.WIDTH))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = prm_cases.seeded_weights(shapes, int(golden["seed"]), float(golden["gain"]))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return model


# ---- restatement == goldens -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(prm_cases.crafted()))
def test_restatement_equals_reference_on_crafted_maps(name):
    g, case = load("prm_peaks"), prm_cases.crafted()[name]
    valid, score, order = g[name + "__valid"], g[name + "__scores"], g[name + "__order"]
    shape = next(iter(case["maps"].values())).shape
    res = prm_np.image_points([case["maps"][c] for c in case["labels"]], case["labels"], shape[0], shape[1], case["threshold"])
    assert res["count"] == len(score)
    for c in case["labels"]:
        assert prm_np.pair_peaks(case["maps"][c], case["threshold"])[1] == int(np.sum(g[name + "__all"][:, 0] == c))
    if name == "many_257":
        assert res["status"] == prm_np.STATUS_TOO_MANY and res["count"] == 257
        return
    assert res["status"] == 0
    # the reference lists the valid peaks pair by pair in row-major order, then sorts by score
    np.testing.assert_array_equal(np.stack([res["classes"], res["ys"], res["xs"]], 1), valid[order])
    np.testing.assert_array_equal(res["scores"], score[order])


def test_crafted_goldens_hold_the_stated_rules():
    g = load("prm_peaks")
    np.testing.assert_array_equal(g["constant__all"], [[0, 0, 0]])                 # a constant map: the single peak (0, 0)
    np.testing.assert_array_equal(g["plateau__all"], [[0, 0, 1]])                  # the first maximum of the window wins
    np.testing.assert_array_equal(g["plateau__valid"], [[0, 0, 1]])                # ... and is the fallback (2 <= 10)
    assert g["at_threshold__scores"].tolist() == [float(np.nextafter(np.float32(10), np.float32(11)))]   # exactly 10 is not valid
    np.testing.assert_array_equal(g["none_above__valid"], [[0, 0, 2]])             # the FIRST peak holding the largest value
    np.testing.assert_array_equal(g["signed_zero_peaks__valid"], [[0, 0, 0]])      # -0.0 == +0.0 for the arg-max
    assert g["two_pairs_out_of_order__valid"][0, 0] == 3                           # pairs in the caller's order, not class order
    assert np.isinf(g["zeros_inf__scores"]).any()                                  # +inf is an ordinary value


def test_restatement_equals_reference_on_the_network_cases():
    g = load("prm_net")
    for i in range(2):
        labels = g["labels"][i].tolist()
        up = prm_np.upsample(g["crm32"][i][None], [(0, c) for c in labels], FACTOR)
        res = prm_np.image_points(list(up), labels, up.shape[1], up.shape[2], prm_cases.THRESHOLD)
        order = g["order_%d" % i]
        np.testing.assert_array_equal(np.stack([res["classes"], res["ys"], res["xs"]], 1), g["valid_%d" % i][order])
        # (the reference's scores are ATen's up-sampled values: the last bits differ)
        np.testing.assert_allclose(res["scores"], g["scores_%d" % i][order], rtol=1e-5, atol=1e-5)
        assert np.all(np.diff(g["scores_%d" % i][order]) > 0)
    m = g["margins"]                                                               # delta, window, median, threshold, score gap, others
    assert np.all(m[:, 1:5] >= m[:, :1]) and np.all(m[:, 5] >= m[:, 0] / 50)
    tops = [prm_np.upsample(g["crm32"][i][None], [(0, c) for c in g["labels"][i]], FACTOR).reshape(3, -1).max(1) for i in range(2)]
    assert any((t > 10).any() for t in tops) and any((t < 10).any() for t in tops)  # peaks above the threshold, and the fallback


def test_restatement_reaches_the_reference_mat():
    g = load("prm_e2e")
    counts = []
    for i in range(3):
        labels = g["labels_%d" % i].tolist()
        masks = ppn.unpack_bits(g["mask_bits_%d" % i], g["mask_shape_%d" % i])
        up = prm_np.upsample(g["crm32_%d" % i][None], [(0, c) for c in labels], FACTOR)
        assert up.shape[1:] == (112, 112)
        res = prm_np.image_points(list(up), labels, masks.shape[1], masks.shape[2], prm_cases.THRESHOLD)
        order = g["order_%d" % i]
        np.testing.assert_array_equal(np.stack([res["classes"], res["ys"], res["xs"]], 1), g["valid_%d" % i][order])
        mat = ppn.assign_clusters(masks, res["rows"], res["cols"], res["classes"], 20)
        np.testing.assert_array_equal(mat, g["mat_%d" % i])
        assert mat.any()
        counts.append(res["count"])
    assert counts[1] == 1 and g["scores_1"][0] < 10                                # the fallback image
    assert len(g["labels_2"]) == 1 and counts[2] >= 3                              # one class, several clusters
    assert len(set(g["valid_0"][:, 0].tolist())) >= 2


# ---- the pieces -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 15, 16, 255, 256, 1001])
def test_lower_median_is_np_partition(n):
    rng = np.random.RandomState(n)
    a = rng.randint(-50, 50, n).astype(np.float32) / 4                             # duplicates
    assert prm_np.lower_median(a) == np.partition(a, (n - 1) // 2)[(n - 1) // 2]
    assert prm_np.lower_median(np.array([4, 1, 3, 2], dtype=np.float32)) == 2      # what torch.median gives
    assert float(torch.median(torch.from_numpy(a))) == float(prm_np.lower_median(a))


def test_lower_median_of_many_duplicates():
    m = prm_cases.duplicates_map()
    k = (m.size - 1) // 2
    assert prm_np.lower_median(m) == np.partition(m.reshape(-1), k)[k]
    keys = m.view(np.uint32).reshape(-1)
    keys = np.where(keys >> 31, ~keys, keys | np.uint32(1 << 31))
    for shift in (24, 16, 8, 0):                                                   # every radix pass meets several bins
        assert len(np.unique((keys >> shift) & 255)) > 4


def test_integer_point_scaling_is_the_float64_expression():
    sides = sorted(set([1, 2, 3, 7, 111, 112, 113, 333, 375, 448, 500, 1000, 4096, 32768, 65534, 65535]
                       + np.random.RandomState(0).randint(1, 65536, 60).tolist()))
    for grid in range(1, 513):
        y = np.arange(grid, dtype=np.int64)
        for side in sides:
            want = (y.astype(np.float64) * side / grid).astype(np.int64)           # int(y * shape / 112), AGPL_label_assign.py:158
            np.testing.assert_array_equal((y * side) // grid, want, err_msg="grid %d side %d" % (grid, side))
    assert prm_np.scale_point(111, 375, 112) == int(111 * 375 / 112)


def test_upsample_restatement_is_close_to_aten_and_not_identical():
    """The contract is the stated arithmetic; ATen's is another one (its CPU kernel differs in the last bit on part of the
    elements).  The distance bounds what `close` means for the golden inputs."""
    import torch.nn.functional as F
    rng = np.random.RandomState(3)
    crm = (rng.randn(1, 4, 14, 14) * 10).astype(np.float32)
    up = prm_np.upsample(crm, [(0, c) for c in range(4)], FACTOR)
    aten = F.interpolate(torch.from_numpy(crm), scale_factor=FACTOR, mode="bilinear", align_corners=True).numpy()[0]
    exact = F.interpolate(torch.from_numpy(crm).double(), scale_factor=FACTOR, mode="bilinear", align_corners=True).numpy()[0]
    assert np.abs(up - aten).max() <= 8e-6
    assert np.abs(up - exact).max() <= 2 * max(np.abs(aten - exact).max(), 4e-6)
    np.testing.assert_array_equal(prm_np.upsample(crm, [(0, 2)], 1)[0], crm[0, 2])  # factor 1 is the identity
    one = prm_np.upsample(crm[:, :, :1, :1], [(0, 1)], 3)
    assert np.all(one == crm[0, 1, 0, 0])                                          # a 1 x 1 map: scale 0


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_prm_entries():
    from cim_amd import _abi, _lib, build, prm
    header = open(os.path.join(REPO, "include", "cim_hip.h")).read()
    declared = set(re.findall(r"\b(cim_prm_[a-z0-9_]+)\s*\(", header))
    assert declared == {"cim_prm_ws_bytes", "cim_prm_upsample", "cim_prm_peaks", "cim_prm_points"}
    functions, structs, constants = _abi.parse(header)
    assert len(structs) == 8                                                       # no new struct
    import ctypes
    assert functions["cim_prm_ws_bytes"][0] is ctypes.c_longlong and functions["cim_prm_points"][0] is ctypes.c_int
    assert constants["CIM_PRM_MAX_HW"] == 1 << 22 and constants["CIM_PRM_MAX_PEAKS"] == constants["CIM_PROP_MAX_POINTS"] == 256
    assert (prm.MAX_PEAKS, prm.STATUS_TOO_MANY, prm.STATUS_NAN, prm.STATUS_NO_PEAK) == (256, 1, 2, 4)
    assert (prm_np.MAX_PEAKS, prm_np.STATUS_TOO_MANY, prm_np.STATUS_NAN, prm_np.STATUS_NO_PEAK) == (256, 1, 2, 4)
    build.build()
    lib = _lib.load()
    assert lib.cim_abi_version() == _lib.ABI_VERSION == 16                         # additive
    for name in declared:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    assert os.path.join(build.CSRC, "prm.hip") in build.sources()


def test_ws_bytes_is_monotone_and_refuses():
    from cim_amd import _lib
    ws = lambda m, hw: _lib.call("cim_prm_ws_bytes", m, hw)
    assert ws(1, 0) > 0
    for m in (1, 2, 3, 60, 640):
        for hw in (0, 1, 384, 112 * 112, (1 << 22) - 1):
            assert ws(m + 1, hw) > ws(m, hw) and ws(m, hw + 1) >= ws(m, hw) and ws(m, hw) >= m * hw * 4
    assert ws(0, 16) == -1 and ws(1, (1 << 22) + 1) == -1 and ws(1, -1) == -1
    assert b"cim_prm_ws_bytes" in _lib.load().cim_last_error()


def test_entries_refuse_bad_descriptions_on_the_host():
    """M < 1, H W beyond the limit, factor < 1, a class outside 0..C-1, unsorted image indices: -1 before anything touches the
    device (the pointers here are not device pointers: a launch would not survive them)."""
    import ctypes
    from cim_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(64)

    def desc(img, cls, hs, ws):
        a = np.ascontiguousarray(np.array(list(img) + list(cls) + list(hs) + list(ws), dtype=np.int32))
        return a, a.ctypes.data_as(ctypes.c_void_p)

    def points(d, b, c, h, w, factor, m):
        return lib.cim_prm_points(fake, None, b, c, h, w, factor, m, d, fake, 10.0, fake, fake, fake, fake, fake, fake, None)

    keep, good = desc([0, 0, 1], [2, 0, 1], [10, 10], [10, 10])
    assert points(good, 2, 3, 2, 3, 0, 3) == -1 and b"factor" in lib.cim_last_error()
    assert points(good, 2, 3, 2, 3, 8, 0) == -1 and b"M >= 1" in lib.cim_last_error()
    assert points(good, 2, 3, 1024, 1024, 4, 3) == -1                              # 4096 x 4096 up-sampled pixels
    assert points(good, 2, 2, 2, 3, 8, 3) == -1 and b"class 2" in lib.cim_last_error()
    k2, unsorted = desc([1, 0, 1], [2, 0, 1], [10, 10], [10, 10])
    assert points(unsorted, 2, 3, 2, 3, 8, 3) == -1 and b"ascending" in lib.cim_last_error()
    k3, outside = desc([0, 0, 2], [2, 0, 1], [10, 10], [10, 10])
    assert points(outside, 2, 3, 2, 3, 8, 3) == -1
    k4, side = desc([0, 0, 1], [2, 0, 1], [10, 70000], [10, 10])
    assert points(side, 2, 3, 2, 3, 8, 3) == -1 and b"65535" in lib.cim_last_error()
    assert lib.cim_prm_peaks(fake, 3, 2048, 2049, 2, 3, good, fake, 10.0, fake, fake, fake, fake, fake, fake, None) == -1
    assert lib.cim_prm_upsample(fake, None, 2, 3, 2, 3, -1, 3, good, fake, fake, None) == -1


# ---- the network's modules on the CPU ---------------------------------------------------------------------------------------
def test_state_dict_keys_are_the_references_and_load_strictly():
    from cim_amd import prm
    g = load("prm_net")
    model = prm.PeakResponseMapping(prm.fc_resnet50(prm_cases.NUM_CLASSES, width=prm_cases.WIDTH))
    assert list(model.state_dict()) == g["keys"].tolist()
    assert "0.features.0.weight" in g["keys"] and "0.classifier.0.bias" in g["keys"] and "0.features.7.2.bn3.running_var" in g["keys"]
    thin_model(g)                                                                  # strict=True inside
    full = prm.fc_resnet50(20)
    assert full.classifier[0].weight.shape == (20, 2048, 1, 1) and full.features[7][0].conv2.stride == (2, 2)
    assert not model.training and all(not m.training for m in model.modules())


def test_network_on_the_cpu_gives_the_reference_maps():
    """The architecture, through the ATen branch the wrappers take for CPU tensors: the same layers in the same order as the
    reference's, so the class response maps agree to rounding (the bound of the device test: 4 x the reference's own fp32 error)."""
    g = load("prm_net")
    model = thin_model(g)
    h, w = prm_cases.NET_SHAPE
    x = torch.from_numpy(prm_cases.normalise(prm_cases.seeded_images(int(g["seed"]), 2, h, w)))
    crm = model(x).numpy()
    assert crm.shape == g["crm32"].shape == (2, 20, 2, 3) and not model(x).requires_grad
    for i in range(2):
        for c in range(20):
            scale = np.abs(g["crm64"][i, c]).max()
            ref_err = np.abs(g["crm32"][i, c].astype(np.float64) - g["crm64"][i, c]).max() / scale
            assert np.abs(crm[i, c].astype(np.float64) - g["crm32"][i, c]).max() / scale <= 4 * ref_err + 1e-12, (i, c)


def test_what_is_not_part_of_this_package_says_so():
    from cim_amd import prm
    model = prm.peak_response_mapping(prm.fc_resnet50(3, width=4))
    assert model.inference() is model and model.sub_pixel_locating_factor == 8
    for call in (lambda: model.train(), lambda: model.instance_seg(None, None, None, None), lambda: model.instance_nms([]),
                 lambda: prm.PeakResponseMapping(prm.fc_resnet50(3, width=4), filter_type="mean"),
                 lambda: prm.PeakResponseMapping(prm.fc_resnet50(3, width=4), filter_type=5),
                 lambda: prm.PeakResponseMapping(prm.fc_resnet50(3, width=4), win_size=5),
                 lambda: prm.peak_response_mapping(prm.fc_resnet50(3, width=4), enable_peak_backprop=False),
                 lambda: prm.peak_response_mapping_aff(), lambda: prm.peak_response_mapping_aff_vis()):
        with pytest.raises(NotImplementedError, match="cim_amd.prm.peaks"):
            call()
    assert model.eval() is model                                                   # train(False) stays allowed
    from cim_amd import _lib
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        prm.peaks(model, torch.zeros(1, 3, 32, 32), [[0]])
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        prm.peaks_from_maps(torch.zeros(1, 4, 4), [[0]])
