"""Host side of cim_amd.optim.Adam (no GPU): dispatch, C ABI, refused configurations, state-dict layout."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _toy():
    return torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.ReLU(), torch.nn.Linear(4, 3, bias=False))


def test_make_optimizer_dispatches_on_solver_type():
    """SOLVER.TYPE Adam: cim_amd.optim.Adam over the two groups of tools/train.py:282-306 (weights; biases without weight
    decay; lr 0 until the schedule sets it) with torch's default betas / eps, as train.py:311; an unknown type still raises."""
    from cim_amd.core.config import cfg, reset_cfg
    from cim_amd.optim import SGD, Adam, make_optimizer
    reset_cfg()
    try:
        model = _toy()
        cfg.SOLVER.TYPE = "Adam"
        opt = make_optimizer(model)
        assert type(opt) is Adam
        ref = torch.optim.Adam(model.parameters())
        assert len(opt.param_groups) == 2
        weights, biases = opt.param_groups
        assert [tuple(p.shape) for p in weights["params"]] == [(4, 5), (3, 4)] and [tuple(p.shape) for p in biases["params"]] == [(4,)]
        assert weights["weight_decay"] == cfg.SOLVER.WEIGHT_DECAY and biases["weight_decay"] == 0
        for grp in opt.param_groups:
            assert grp["lr"] == 0 and grp["betas"] == ref.defaults["betas"] == (0.9, 0.999) and grp["eps"] == ref.defaults["eps"] == 1e-8
            assert set(grp) == set(ref.param_groups[0])
        cfg.SOLVER.TYPE = "SGD"
        assert type(make_optimizer(model)) is SGD
        cfg.SOLVER.TYPE = "RMSprop"
        with pytest.raises(NotImplementedError):
            make_optimizer(model)
    finally:
        reset_cfg()


def test_adam_entry_point_is_declared_and_exported():
    from cim_amd import _lib, build
    build.build()
    header = open(os.path.join(REPO, "include", "cim_hip.h")).read()
    assert re.search(r"\bint cim_adam_multi\s*\(const cim_adam_tensor\* tensors, const cim_sgd_chunk\* chunks, int n_chunks,", header)
    assert "cim_adam_multi" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "cim_adam_multi")
    assert _lib.load().cim_abi_version() == 16
    # the record the optimizer writes is the struct the header declares: 80 bytes, same field order
    from cim_amd.optim import adam
    body = re.search(r"typedef struct cim_adam_tensor \{(.*?)\} cim_adam_tensor;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert fields == list(adam._TENSOR.names) and adam._TENSOR.itemsize == 80
    # null tables with chunks to run are an argument error, reported before any launch
    with pytest.raises(_lib.CimHipError):
        _lib.call("cim_adam_multi", 0, 0, 1, 0.9, 0.999, 1e-8, 0, 0)
    _lib.call("cim_adam_multi", 0, 0, 0, 0.9, 0.999, 1e-8, 0, 0)


def test_adam_refuses_what_it_does_not_provide():
    from cim_amd import _lib
    from cim_amd.optim import Adam
    p = lambda: [torch.zeros(4, requires_grad=True)]
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True), dict(decoupled_weight_decay=True)):
        with pytest.raises(NotImplementedError):
            Adam(p(), **kw)
    with pytest.raises(NotImplementedError):
        Adam([dict(params=p()), dict(params=p(), betas=(0.8, 0.999))])
    with pytest.raises(NotImplementedError):
        Adam([dict(params=p()), dict(params=p(), eps=1e-6)])
    # a group edited after construction is caught at the step, before anything else
    ps = p()
    opt = Adam(ps)
    ps[0].grad = torch.ones(4)
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(NotImplementedError):
        opt.step()
    # CPU parameters: an error, not a fallback - and nothing was counted or created
    ps = p()
    opt = Adam(ps, lr=0.1)
    ps[0].grad = torch.ones(4)
    with pytest.raises(_lib.CimHipError):
        opt.step()
    assert torch.equal(ps[0].detach(), torch.zeros(4)) and len(opt.state) == 0


def test_adam_state_dict_travels_between_torch_and_the_fused_optimizer():
    """torch.optim.Adam stepped twice on CPU tensors -> cim_amd.optim.Adam.load_state_dict, and back: same keys in the same
    order, `step` the same kind of tensor, values carried over (no launch involved)."""
    from cim_amd.optim import Adam
    g = torch.Generator().manual_seed(1)
    mk = lambda: [torch.randn(6, 3, generator=torch.Generator().manual_seed(2)).requires_grad_(True), torch.zeros(5, requires_grad=True)]
    groups = lambda ps: [dict(params=ps[:1], lr=0.05, weight_decay=0.01), dict(params=ps[1:], lr=0.1, weight_decay=0.0)]
    tp, hp = mk(), mk()
    ref, hip = torch.optim.Adam(groups(tp)), Adam(groups(hp))
    for _ in range(2):
        for p in tp:
            p.grad = torch.randn(p.shape, generator=g)
        ref.step()
    sd = ref.state_dict()
    hip.load_state_dict(sd)
    back = hip.state_dict()
    assert [list(grp.keys()) for grp in back["param_groups"]] == [list(grp.keys()) for grp in sd["param_groups"]]
    assert back["param_groups"] == sd["param_groups"]
    assert list(back["state"].keys()) == list(sd["state"].keys()) == [0, 1]
    for k in sd["state"]:
        a, b = sd["state"][k], back["state"][k]
        assert list(a.keys()) == list(b.keys()) == ["step", "exp_avg", "exp_avg_sq"]
        assert type(b["step"]) is type(a["step"]) and b["step"].dtype == a["step"].dtype == torch.float32
        assert b["step"].device == a["step"].device and b["step"].shape == a["step"].shape and float(b["step"]) == 2.0
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
    for p in hp:
        assert set(hip.state[p]) == {"step", "exp_avg", "exp_avg_sq"}
    # and the other way round: torch accepts what the fused optimizer saves, and goes on counting from it
    ref2 = torch.optim.Adam(groups(tp))
    ref2.load_state_dict(back)
    for p in tp:
        p.grad = torch.randn(p.shape, generator=g)
    ref2.step()
    assert all(float(ref2.state[p]["step"]) == 3.0 for p in tp)
