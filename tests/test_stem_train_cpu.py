"""The trainable ResNet stem without a GPU: the float64 restatement of the 7 x 7 weight gradient against
torch.nn.grad.conv2d_weight, the new entries of the C header, prm_train.unfreeze / freeze, and the operator's refusal of CPU
tensors."""
import os
from ctypes import c_int, c_longlong, c_void_p

import numpy as np
import pytest
import torch

import prm_cases
import stem_dw_np as sdn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "cim_hip.h")


@pytest.mark.parametrize("shape", sdn.SHAPES)
def test_restatement_equals_torch_float64(shape):
    b, cin, cout, h, w, s = shape
    for integers in (False, True):
        dconv, x = sdn.seeded(shape, 7, integers)
        dw, mag = sdn.dw_and_abs(dconv, x, s)
        ref = torch.nn.grad.conv2d_weight(torch.from_numpy(x).double(), (cout, cin, 7, 7), torch.from_numpy(dconv).double(),
                                          stride=s, padding=3).numpy()
        assert dw.shape == ref.shape == mag.shape == (cout, cin, 7, 7)
        # two float64 summation orders of T terms: T 2^-53 sum |term| apart at the most
        assert np.all(np.abs(dw - ref) <= sdn.terms(shape) * 2.0 ** -52 * mag)
        assert np.all(mag >= np.abs(dw))
        if integers:
            assert np.array_equal(dw, np.rint(dw)) and mag.max() <= 4 * sdn.terms(shape) < 2 ** 24
    # the magnitudes are the product of the magnitudes
    dconv, x = sdn.seeded(shape, 8)
    assert np.array_equal(sdn.dw_and_abs(np.abs(dconv), np.abs(x), s)[0], sdn.dw_and_abs(dconv, x, s)[1])


def test_single_tap_by_hand():
    # one output pixel (1, 2) of a 5 x 6 image at stride 2 reaches x[2 + ky - 3][4 + kx - 3]
    x = np.arange(30, dtype=np.float64).reshape(1, 1, 5, 6)
    dconv = np.zeros((1, 1, 3, 3))
    dconv[0, 0, 1, 2] = 2.0
    dw, mag = sdn.dw_and_abs(dconv, x, 2)
    for ky in range(7):
        for kx in range(7):
            iy, ix = 2 + ky - 3, 4 + kx - 3
            want = 2.0 * x[0, 0, iy, ix] if 0 <= iy < 5 and 0 <= ix < 6 else 0.0
            assert dw[0, 0, ky, kx] == want == mag[0, 0, ky, kx]


def test_new_entries_parse_from_the_header():
    from cim_amd import _abi, _lib
    functions, _, _ = _abi.parse(open(HEADER).read())
    shape = [c_int] * 6
    assert functions["cim_conv7x7_dw_workspace"] == (c_longlong, shape)
    assert functions["cim_conv7x7_dw_splits"] == (c_int, shape)
    # (dconv, x, dw, six integers, workspace, stream: the binding passes every pointer as void*)
    assert functions["cim_conv7x7_dw_f32"] == (c_int, [c_void_p] * 3 + shape + [c_void_p] * 2)
    assert _lib.FUNCTIONS["cim_conv7x7_dw_f32"] == functions["cim_conv7x7_dw_f32"]
    assert "cim_conv7x7_dw_workspace" in _lib.VALUE_RETURNING and _lib.ABI_VERSION == 16
    assert not [n for n in functions if n.startswith("cim_prm_") and "conv7x7" in n]


def _thin_model():
    from cim_amd import prm
    return prm.PeakResponseMapping(prm.fc_resnet50(prm_cases.NUM_CLASSES, width=prm_cases.WIDTH))


def test_unfreeze_trains_every_parameter_and_keeps_the_checkpoint_surface():
    from cim_amd import prm_train
    model = _thin_model()
    keys = list(model.state_dict().keys())
    prm_train.freeze(model, at=4)
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    assert any(n.startswith("0.features.0") for n in frozen) and any(n.startswith("0.features.5") for n in frozen)
    assert prm_train.unfreeze(model) is model
    assert all(p.requires_grad for p in model.parameters())
    assert list(model.state_dict().keys()) == keys
    assert not any(m.training for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d))      # statistics stay frozen
    # freeze keeps its contract: default = stem + layer1, `at` outside 2..5 refused
    prm_train.freeze(model)
    names = [n for n, p in model.named_parameters() if not p.requires_grad]
    assert names and all(n.startswith(("0.features.0", "0.features.1", "0.features.4")) for n in names)
    for at in (0, 1, 6):
        with pytest.raises(ValueError, match="one of 2, 3, 4, 5"):
            prm_train.freeze(model, at=at)
    with pytest.raises(TypeError):
        prm_train.unfreeze(torch.nn.Sequential(torch.nn.Conv2d(3, 4, 1)))


def test_training_stem_refuses_cpu_tensors():
    from cim_amd.ops import conv7x7_bn_act_train
    conv = torch.nn.Conv2d(3, 8, 7, stride=2, padding=3, bias=False)
    bn = torch.nn.BatchNorm2d(8).eval()
    with pytest.raises(ValueError, match="no CPU path"):
        conv7x7_bn_act_train(torch.zeros(1, 3, 16, 16), conv, bn)
