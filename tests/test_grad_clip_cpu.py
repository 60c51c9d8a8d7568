"""Host side of the on-device gradient clipping (no GPU): C ABI, chunk table, dispatch of cim_amd.utils.net.clip_gradient."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _toy():
    torch.manual_seed(4)
    m = torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.ReLU(), torch.nn.Linear(4, 3, bias=False))
    m(torch.randn(6, 5)).square().sum().backward()
    return m


def test_entry_points_are_declared_and_exported():
    from cim_amd import _abi, _lib, build
    build.build()
    header = open(os.path.join(REPO, "include", "cim_hip.h")).read()
    flat = " ".join(re.sub(r"/\*.*?\*/", " ", header, flags=re.S).split())
    assert ("int cim_grad_norm_multi(const uint64_t* grads, const int64_t* numel, int n_tensors, const cim_sgd_chunk* chunks, "
            "int n_chunks, double* partial , double max_norm, float* out , int max_workgroups, void* stream);") in flat
    assert ("int cim_grad_scale_multi(const uint64_t* grads, const int64_t* numel, int n_tensors, const cim_sgd_chunk* chunks, "
            "int n_chunks, const float* out, int max_workgroups, void* stream);") in flat
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert _lib.SIGNATURES["cim_grad_norm_multi"] == [P, P, I, P, I, P, D, P, I, P]
    assert _lib.SIGNATURES["cim_grad_scale_multi"] == [P, P, I, P, I, P, I, P]
    assert _lib.FUNCTIONS["cim_grad_norm_multi"][0] is I and _lib.FUNCTIONS["cim_grad_scale_multi"][0] is I
    assert not {"cim_grad_norm_multi", "cim_grad_scale_multi"} & _lib.VALUE_RETURNING       # a status, not a count
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "cim_grad_norm_multi") and hasattr(lib, "cim_grad_scale_multi")
    assert _lib.load().cim_abi_version() == _lib.ABI_VERSION == 16
    assert len(_abi.parse(header)[1]) == 8                                                   # no new struct


def test_argument_rules_before_any_launch():
    from cim_amd import _lib
    _lib.call("cim_grad_norm_multi", 0, 0, 0, 0, 0, 0, 1.0, 0, 0, 0)                         # no chunks: nothing to do
    with pytest.raises(_lib.CimHipError, match="cim_grad_norm_multi.*bad argument"):
        _lib.call("cim_grad_norm_multi", 0, 0, 0, 0, 1, 0, 1.0, 0, 0, 0)
    _lib.call("cim_grad_scale_multi", 0, 0, 0, 0, 0, 0, 0, 0)
    with pytest.raises(_lib.CimHipError, match="cim_grad_scale_multi.*bad argument"):
        _lib.call("cim_grad_scale_multi", 0, 0, 0, 0, 1, 0, 0, 0)
    for bad in (-1.0, float("nan")):
        with pytest.raises(_lib.CimHipError, match="max_norm"):
            _lib.call("cim_grad_norm_multi", 0, 0, 0, 0, 0, 0, bad, 0, 0, 0)
    _lib.call("cim_grad_norm_multi", 0, 0, 0, 0, 0, 0, float("inf"), 0, 0, 0)                # "norm only"


def test_chunk_table():
    from cim_amd.optim import clip, fused
    sizes = [1, 3, 16384, 16385, 40000]
    tab = clip.chunk_table(sizes)
    assert tab.dtype == fused._CHUNK and tab.dtype.itemsize == 16 and fused.CHUNK == 16384
    assert [int((tab["tensor"] == i).sum()) for i in range(5)] == [1, 1, 1, 2, 3] and len(tab) == 8
    assert tab["tensor"].tolist() == [0, 1, 2, 3, 3, 4, 4, 4]
    assert tab["offset"].tolist() == [0, 0, 0, 0, 16384, 0, 16384, 32768]
    assert tab["n"].tolist() == [1, 3, 16384, 16384, 1, 16384, 16384, 40000 - 32768]
    assert all(o % 4 == 0 for o in tab["offset"].tolist())                                    # what the 16-byte accesses rely on
    for i, n in enumerate(sizes):                                                             # the chunks tile every tensor exactly
        mine = tab[tab["tensor"] == i]
        assert int(mine["n"].sum()) == n and np.array_equal(mine["offset"][1:], np.cumsum(mine["n"])[:-1])
    assert len(clip.chunk_table([])) == 0


def test_clipper_refuses_cpu_gradients():
    from cim_amd import _lib
    from cim_amd.optim import GradClipper
    m = _toy()
    before = [p.grad.clone() for p in m.parameters()]
    c = GradClipper(m.parameters())
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        c.clip(0.5)
    with pytest.raises(_lib.CimHipError, match="no CPU fallback"):
        c.norm()
    assert all(torch.equal(p.grad, b) for p, b in zip(m.parameters(), before))
    assert GradClipper(torch.nn.Linear(3, 2).parameters()).clip(1.0) is None                  # no gradients: no launch


def test_clip_gradient_on_the_cpu_is_the_torch_helper():
    from cim_amd.utils import net
    for clip_norm in (0.01, 1e6):
        a, b = _toy(), _toy()
        assert net.clip_gradient(a, clip_norm) is None
        net._clip_gradient_torch([p.grad for p in b.parameters()], clip_norm)
        for pa, pb in zip(a.parameters(), b.parameters()):
            assert torch.equal(pa.grad, pb.grad)
    small = _toy()
    net.clip_gradient(small, 0.01)
    total = float(torch.sqrt(sum(p.grad.double().square().sum() for p in small.parameters())))
    assert abs(total - 0.01) < 1e-7                                                           # it did clip
    assert not net._CLIPPERS                                                                  # no device clipper for CPU models


def test_model_without_gradients_is_a_no_op():
    from cim_amd.utils import net
    m = torch.nn.Linear(3, 2)
    assert net.clip_gradient(m, 1.0) is None
    assert all(p.grad is None for p in m.parameters())
    frozen = _toy()
    for p in frozen.parameters():
        p.requires_grad_(False)
    before = [p.grad.clone() for p in frozen.parameters()]
    assert net.clip_gradient(frozen, 1e-3) is None                                            # (the reference skips frozen parameters)
    assert all(torch.equal(p.grad, b) for p, b in zip(frozen.parameters(), before))
