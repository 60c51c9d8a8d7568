"""No GPU: the float64 restatement of batch-statistics BatchNorm (tests/golden/bn_train_np.py) against torch's own
F.batch_norm(training=True) + autograd in float64, the new entry points in the header and the binding, and the operator's
refusals that need no device."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_train_np as bnp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cim_bn_train_workspace", "cim_bn_train_chunks", "cim_bn_train_fwd", "cim_bn_train_bwd")


@pytest.mark.parametrize("relu,with_res", [(True, False), (False, False), (True, True), (False, True)])
@pytest.mark.parametrize("shape", [s for s in bnp.SHAPES if s[0] * s[1] * s[2] <= 60000])
def test_restatement_against_torch_float64(shape, relu, with_res):
    n, c, hw = shape
    eps = 1e-5
    rs = np.random.RandomState(sum(shape))
    x = bnp.seeded(shape, 3 + hw, "a").astype(np.float64)
    gamma, beta = (a.astype(np.float64) for a in bnp.seeded_affine(c, 5))
    res = rs.standard_normal(shape) if with_res else None
    dy = rs.standard_normal(shape)

    y, mean, var = bnp.forward(x, gamma, beta, eps, res, relu)
    got = bnp.backward(dy, x, y, gamma, mean, var, eps, relu)

    tx = torch.from_numpy(x).reshape(n, c, hw, 1).requires_grad_(True)
    tg, tb = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
    tr = torch.from_numpy(res).reshape(n, c, hw, 1).requires_grad_(True) if with_res else None
    out = F.batch_norm(tx, None, None, tg, tb, True, 0.1, eps)
    if with_res:
        out = out + tr
    if relu:
        out = F.relu(out)
    out.backward(torch.from_numpy(dy).reshape(n, c, hw, 1))

    def close(a, b, what):
        a, b = np.asarray(a).reshape(-1), b.detach().numpy().reshape(-1)
        assert np.abs(a - b).max() <= 1e-10 * max(1.0, np.abs(b).max()), what

    close(y, out, "y")
    close(got["dx"], tx.grad, "dx")
    close(got["dgamma"], tg.grad, "dgamma")
    close(got["dbeta"], tb.grad, "dbeta")
    if with_res:
        close(got["dres"], tr.grad, "dres")
    assert np.all(got["mag1"] >= np.abs(got["S1"]) - 1e-12) and np.all(got["mag2"] >= np.abs(got["S2"]) - 1e-12)


@pytest.mark.parametrize("momentum", [0.1, None])
def test_running_buffers_over_two_calls(momentum):
    shape = (3, 5, 49)
    bn = torch.nn.BatchNorm2d(5, momentum=momentum).double().train()
    with torch.no_grad():
        bn.running_mean.uniform_(-0.3, 0.3)
        bn.running_var.uniform_(0.5, 2.0)
    rm, rv, batches = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy(), 0
    for call in range(2):
        x = bnp.seeded(shape, 20 + call, "a").astype(np.float64)
        bn(torch.from_numpy(x).reshape(3, 5, 7, 7))
        mean, var, _ = bnp.stats(x)
        rm, rv, batches = bnp.running_update(rm, rv, batches, mean, var, 3 * 49, momentum)
        assert int(bn.num_batches_tracked) == batches == call + 1
        assert np.abs(rm - bn.running_mean.numpy()).max() <= 1e-12 and np.abs(rv - bn.running_var.numpy()).max() <= 1e-12


def test_chunks_of_the_listed_shapes():
    """The chunk rule restated (the GPU test compares it with cim_bn_train_chunks): the boundary shapes are boundaries."""
    want = {(1, 1, 4095): 1, (1, 2, 4096): 1, (1, 1, 4097): 2, (2, 3, 9000): 6, (3, 2, 2049): 3, (5, 2, 1025): 2, (9, 2, 1024): 3,
            (200, 2, 41): 3, (70, 1, 4096): 70, (16, 4, 3136): 16, (2, 64, 784): 1}
    for shape, k in want.items():
        assert shape in bnp.SHAPES and bnp.chunks(shape) == k, shape


def test_entry_points_are_declared_and_bound():
    from cim_amd import _lib
    assert _lib.ABI_VERSION == 16
    with open(os.path.join(REPO, "include", "cim_hip.h")) as f:
        header = f.read()
    for name in ENTRIES:
        assert name + "(" in header and name in _lib.FUNCTIONS, name
    assert len(_lib.SIGNATURES["cim_bn_train_fwd"]) == 19 and len(_lib.SIGNATURES["cim_bn_train_bwd"]) == 16
    assert {"cim_bn_train_workspace", "cim_bn_train_chunks"} <= _lib.VALUE_RETURNING
    assert "CIM_ABI_VERSION" not in _lib.CONSTANTS or _lib.CONSTANTS["CIM_ABI_VERSION"] == 16
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.cim_abi_version() == 16
        for name in ENTRIES:
            assert getattr(lib, name).argtypes == _lib.FUNCTIONS[name][1]
        # host-only entries: the chunk rule and the refusals need no device
        for shape in bnp.SHAPES:
            k = lib.cim_bn_train_chunks(*shape)
            assert k == bnp.chunks(shape), shape
            assert lib.cim_bn_train_workspace(*shape) == (shape[1] * k + shape[1]) * 16
        for bad, names in (((1, 1, 1), "N * HW"), ((2, 0, 4), "C"), ((0, 1, 4), "N"), ((65536, 65536, 1), "N * C * HW")):
            assert lib.cim_bn_train_chunks(*bad) == -1 and lib.cim_bn_train_workspace(*bad) == -1
            assert names in lib.cim_last_error().decode()


def test_operator_is_exported_and_refuses_on_the_host():
    import cim_amd.ops as ops
    from cim_amd.ops import bn_act_train
    assert "bn_act_train" in ops.__all__
    bn = torch.nn.BatchNorm2d(4)
    x = torch.randn(2, 4, 3, 3)
    with pytest.raises(ValueError, match="no CPU path"):
        bn_act_train(x, bn)
    with pytest.raises(ValueError, match="float32"):
        bn_act_train(x.double(), bn)
    with pytest.raises(ValueError, match="contiguous"):
        bn_act_train(x.permute(0, 1, 3, 2)[:, :, :, ::2], bn)
    with pytest.raises(ValueError, match="4-dimensional"):
        bn_act_train(x.reshape(2, 4, 9), bn)
    with pytest.raises(ValueError, match="affine"):
        bn_act_train(x, torch.nn.BatchNorm2d(4, affine=False))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        bn_act_train(torch.randn(1, 4, 1, 1), bn)
    assert int(bn.num_batches_tracked) == 0


def test_batch_stats_argument_and_train_still_raises():
    import inspect
    from cim_amd import prm, prm_train
    for fn in (prm_train.class_response_maps, prm_train.aggregate, prm_train.loss):
        assert inspect.signature(fn).parameters["batch_stats"].default is False
    model = prm.PeakResponseMapping(prm.fc_resnet50(3, width=4))
    with pytest.raises(NotImplementedError):
        model.train()
