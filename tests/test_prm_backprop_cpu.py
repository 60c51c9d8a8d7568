"""The PRM peak back-propagation on the host (no GPU): the restatement tests/golden/prm_backprop_np.py against the peak response
maps captured from the reference (tests/golden/prm_backprop.npz, make_golden_prm_backprop.py), the C ABI's new entries, and the
refusals of cim_amd.prm.backprop / peak_response_maps, which all come before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import prm_backprop_np as bp
import prm_cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
ENTRIES = {"cim_prmb_min_parts", "cim_prmb_min", "cim_prmb_shift", "cim_prmb_gate", "cim_prmb_scale", "cim_prmb_seed",
           "cim_prmb_stem_workspace", "cim_prmb_stem"}


def load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: d[k] for k in d.files}


def thin_model(golden, edit=None):
    from cim_amd import prm
    model = prm.PeakResponseMapping(prm.fc_resnet50(prm_cases.NUM_CLASSES, width=prm_cases.WIDTH))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = prm_cases.seeded_weights(shapes, int(golden["seed"]), float(golden["gain"]))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    if edit is not None:
        edit(model)
    return model


def images(golden):
    h, w = prm_cases.NET_SHAPE
    return torch.from_numpy(prm_cases.normalise(prm_cases.seeded_images(int(golden["seed"]), 2, h, w)))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return load("prm_backprop")


@pytest.mark.parametrize("i", [0, 1])
def test_restatement_in_float64_equals_the_reference(golden, i):
    """Layer by layer, without autograd, on this package's own modules (the reference's state_dict): prm64 to 1e-12 of each map's
    maximum."""
    g = golden
    model = thin_model(g)
    net = bp.Network(model[0].features, model[0].classifier[0], torch.float64)
    maps = net.maps(images(g)[i:i + 1], g["peaks_%d" % i], int(g["factor"]))
    want = g["prm64_%d" % i]
    assert maps.shape == want.shape and maps.dtype == np.float64
    for k in range(len(want)):
        assert np.abs(maps[k] - want[k]).max() / want[k].max() <= 1e-12, (i, k)
        assert abs(maps[k].sum() - 1.0) <= 1e-12 and (maps[k] >= 0).all()


def test_restatement_gives_nan_for_a_class_without_a_positive_weight(golden):
    g = golden
    c_nan = int(g["nan_class"])

    def edit(m):
        with torch.no_grad():
            wt = m[0].classifier[0].weight
            wt[c_nan] = -wt[c_nan].abs()
    model = thin_model(g, edit)
    net = bp.Network(model[0].features, model[0].classifier[0], torch.float64)
    with np.errstate(invalid="ignore"):
        maps = net.maps(images(g)[0:1], g["nan_peaks"], int(g["factor"]))
    for k, pk in enumerate(g["nan_peaks"].tolist()):
        if pk[0] == c_nan:
            assert np.isnan(maps[k]).all() and np.isnan(g["nan_prm32"][k]).all()
        else:
            j = g["peaks_0"].tolist().index(pk)
            assert np.abs(maps[k] - g["prm64_0"][j]).max() / g["prm64_0"][j].max() <= 1e-12
            assert np.array_equal(g["nan_prm32"][k], g["prm32_0"][j])          # the reference's neighbours are untouched too


def test_golden_holds_what_its_generator_states(golden):
    g = golden
    net = load("prm_net")
    assert int(g["seed"]) == int(net["seed"]) and float(g["gain"]) == float(net["gain"]) and int(g["factor"]) == 8
    for i in range(2):
        assert np.array_equal(g["peaks_%d" % i], net["valid_%d" % i]) and 1 <= len(g["peaks_%d" % i]) <= 6
        assert g["prm32_%d" % i].dtype == np.float32 and g["prm64_%d" % i].dtype == np.float64
        assert g["prm32_%d" % i].shape == (len(g["peaks_%d" % i]),) + prm_cases.NET_SHAPE
        assert np.allclose(g["prm64_%d" % i].reshape(len(g["peaks_%d" % i]), -1).sum(1), 1.0, atol=1e-12)
    assert g["pool_margins"].shape == (2, 2) and (g["pool_margins"] > 0).all()
    assert os.path.getsize(os.path.join(GOLDEN, "prm_backprop.npz")) < 1 << 20


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_new_entries():
    from cim_amd import _abi, _lib, build
    header = open(os.path.join(REPO, "include", "cim_hip.h")).read()
    assert set(re.findall(r"\b(cim_prmb_[a-z0-9_]+)\s*\(", header)) == ENTRIES
    functions, structs, constants = _abi.parse(header)
    assert len(structs) == 8                                                       # no new struct
    assert ENTRIES <= set(_lib.SIGNATURES)
    assert functions["cim_prmb_stem_workspace"][0] is ctypes.c_longlong and functions["cim_prmb_gate"][0] is ctypes.c_int
    assert constants["CIM_PRMB_MIN_MAX_PARTS"] == 1024
    build.build()
    lib = _lib.load()
    assert lib.cim_abi_version() == _lib.ABI_VERSION == 16                         # additive
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    assert os.path.join(build.CSRC, "prm_backprop.hip") in build.sources()


def test_entries_refuse_on_the_host():
    """-1 before anything touches the device (the pointers here are not device pointers: a launch would not survive them)."""
    from cim_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(64)
    assert lib.cim_prmb_min_parts(0) == -1 and lib.cim_prmb_min_parts(1) == 1 and lib.cim_prmb_min_parts(257) == 2
    assert lib.cim_prmb_min_parts(1 << 40) == 1024
    assert lib.cim_prmb_min(fake, 0, fake, fake, None) == -1 and b"cim_prmb_min" in lib.cim_last_error()
    assert lib.cim_prmb_min(None, 4, fake, fake, None) == -1
    assert lib.cim_prmb_shift(fake, None, fake, 4, None) == -1
    assert lib.cim_prmb_shift(fake, fake, fake, 1 << 31, None) == -1                                # one lane per element: one launch's grid
    assert lib.cim_prmb_seed(fake, fake, fake, 1 << 16, 1 << 8, 8, 16, 8, None) == -1                # P C h w = 2^31
    assert lib.cim_prmb_gate(fake, None, None, None, None, fake, None, 1, 4, 16, None) == -1       # n is not optional
    assert lib.cim_prmb_gate(fake, None, None, None, fake, fake, None, 0, 4, 16, None) == -1
    assert lib.cim_prmb_gate(fake, None, None, None, fake, fake, None, 1, 1 << 16, 1 << 16, None) == -1
    assert lib.cim_prmb_scale(fake, fake, None, None, 1, 16, None) == -1
    assert lib.cim_prmb_seed(fake, fake, fake, 1, 3, 2, 3, 0, None) == -1
    assert lib.cim_prmb_seed(fake, fake, fake, 1, 3, 1024, 1024, 4, None) == -1                    # 4096 x 4096 up-sampled pixels
    assert lib.cim_prmb_stem_workspace(0, 8, 8) == -1 and lib.cim_prmb_stem_workspace(2, 9, 33) == 8 * 2 * 2 * 2
    assert lib.cim_prmb_stem(fake, fake, fake, fake, fake, 1, 257, 8, 8, 1, None) == -1 and b"cout" in lib.cim_last_error()
    assert lib.cim_prmb_stem(fake, fake, fake, fake, ctypes.c_void_p(68), 1, 16, 8, 8, 1, None) == -1     # workspace not 8-byte aligned
    assert lib.cim_prmb_stem(fake, fake, fake, fake, None, 1, 16, 8, 8, 1, None) == -1


# ---- refusals of the public entries: all on CPU tensors, before any launch --------------------------------------------------------
def test_public_entries_are_reexported_and_refuse():
    from cim_amd import _lib, prm, prm_backprop
    assert prm.backprop is prm_backprop.backprop and prm.peak_response_maps is prm_backprop.peak_response_maps
    model = prm.peak_response_mapping(prm.fc_resnet50(3, width=4))
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        prm.backprop(model, torch.zeros(1, 3, 32, 32), [[0, 0, 0]])
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        prm.peak_response_maps(model, torch.zeros(1, 3, 32, 32), [[0]])
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        prm.backprop(model, np.zeros((1, 3, 32, 32), dtype=np.float32), [[0, 0, 0]])


def test_refusals_come_before_any_launch():
    from cim_amd import prm
    model = prm.peak_response_mapping(prm.fc_resnet50(3, width=4))
    x = torch.zeros(1, 3, 64, 96)                                                 # CPU tensors: that refusal is the last one asked
    with pytest.raises(ValueError, match="one image at a time, got a batch of 2"):
        prm.backprop(model, torch.zeros(2, 3, 64, 96), [[0, 0, 0]])
    with pytest.raises(ValueError, match=r"\[1, 3, H, W\] float32"):
        prm.backprop(model, torch.zeros(1, 4, 64, 96), [[0, 0, 0]])
    with pytest.raises(ValueError, match="class 3, outside 0..2"):
        prm.backprop(model, x, [[3, 0, 0]])
    with pytest.raises(ValueError, match="class -1"):
        prm.backprop(model, x, np.array([[0, 0, 0], [-1, 0, 0]]))
    for bad in ([0, 16, 0], [0, 0, 24], [0, -1, 0]):                                # the up-sampled grid of 64 x 96 is 16 x 24
        with pytest.raises(ValueError, match="outside the 16 x 24 up-sampled grid"):
            prm.backprop(model, x, [bad])
    with pytest.raises(ValueError, match=r"integers \[P, 3\]"):
        prm.backprop(model, x, [[0.5, 0, 0]])
    with pytest.raises(ValueError, match=r"integers \[P, 3\]"):
        prm.backprop(model, x, [[0, 0]])
    with pytest.raises(ValueError, match="2 class lists for 1 images"):
        prm.peak_response_maps(model, x, [[0], [1]])
    from cim_amd import _lib
    for peaks in ([[2, 15, 23]], np.zeros((0, 3), dtype=np.int64)):                 # nothing else to refuse: the CPU tensor is
        with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
            prm.backprop(model, x, peaks)


def test_a_body_not_built_from_resnetbody_is_refused():
    import torch.nn as nn
    from cim_amd import prm
    x = torch.zeros(1, 3, 64, 96)
    with pytest.raises(TypeError, match="PeakResponseMapping"):
        prm.backprop(prm.fc_resnet50(3, width=4), x, [[0, 0, 0]])

    class Other(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1, self.bn1, self.relu = nn.Conv2d(3, 8, 7, 2, 3, bias=False), nn.BatchNorm2d(8), nn.ReLU()
            self.maxpool = nn.MaxPool2d(3, 2, 1)
            self.layer1 = self.layer2 = self.layer3 = nn.Sequential(nn.Conv2d(8, 8, 1))
            self.layer4 = nn.Sequential(nn.Conv2d(8, 8, 1), nn.Conv2d(8, 8, 1))
            self.layer4[1].conv1 = nn.Conv2d(8, 8, 1)

    foreign = prm.PeakResponseMapping(prm.FC_ResNet(Other(), 3))
    for entry in (lambda: prm.backprop(foreign, x, [[0, 0, 0]]), lambda: prm.peak_response_maps(foreign, x, [[0]])):
        with pytest.raises(TypeError, match="built from cim_amd.prm.ResNetBody"):
            entry()
    # the same Bottleneck class in a geometry the walk does not cover: the stride on the first 1 x 1 (a stride_1x1 body), a dilated
    # 3 x 3, a projection that does not stride with the 3 x 3
    def stride_1x1(m):
        blk = m[0].features[5][0]
        blk.conv1.stride, blk.conv2.stride = (2, 2), (1, 1)

    def dilated(m):
        blk = m[0].features[7][1]
        blk.conv2.dilation, blk.conv2.padding = (2, 2), (2, 2)

    def projection(m):
        m[0].features[6][0].downsample[0].stride = (1, 1)
    for edit in (stride_1x1, dilated, projection):
        other = prm.peak_response_mapping(prm.fc_resnet50(3, width=4))
        edit(other)
        with pytest.raises(TypeError, match="built from cim_amd.prm.ResNetBody"):
            prm.backprop(other, x, [[0, 0, 0]])
    stem5 = prm.peak_response_mapping(prm.fc_resnet50(3, width=4))
    stem5[0].features[0] = nn.Conv2d(3, 4, 5, 2, 2, bias=False)
    with pytest.raises(TypeError, match="built from cim_amd.prm.ResNetBody"):
        prm.backprop(stem5, x, [[0, 0, 0]])


def test_default_chunk_keeps_the_largest_gradient_under_its_budget():
    from cim_amd import prm_backprop as pb
    assert pb.CHUNK_BYTES == 256 << 20
    assert 4 * 64 * 112 * 112 * 4 == 12845056                                      # one peak's layer1 gradient at width 64, 448 x 448
    assert pb.default_chunk(64, 448, 448, 100) == 20 and pb.default_chunk(64, 448, 448, 3) == 3
    assert pb.default_chunk(16, 64, 96, 1000) == pb.CHUNK_MAX and pb.default_chunk(256, 2048, 2048, 5) == 1
    for p in (1, 7, 50):
        c = pb.default_chunk(64, 448, 448, p)
        assert 1 <= c <= p and c * 12845056 <= pb.CHUNK_BYTES


def test_unchanged_behaviour_of_the_inference_object():
    from cim_amd import prm
    model = prm.peak_response_mapping(prm.fc_resnet50(3, width=4))
    assert model.inference() is model
    with pytest.raises(NotImplementedError):
        model.train()
    for call in (lambda: model.instance_seg(None, None, None, None), lambda: model.instance_nms([])):
        with pytest.raises(NotImplementedError, match="proposal retrieval.*cim_amd.prm.peaks"):
            call()
