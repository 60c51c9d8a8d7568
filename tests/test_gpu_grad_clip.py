"""Gradient clipping on the device (csrc/grad_clip.hip, cim_amd.optim.GradClipper, cim_amd.utils.net.clip_gradient).

The reference throughout is float64 on the host: norm = sqrt(fsum(float(x)**2)) over the fp32 inputs (every square is exact in
a double, fsum adds them without error, so `ref` is the correctly rounded double).  Tolerances:
  norm  1 fp32 ulp of float32(ref): the kernel's products are exact in fp64 too, its ~120 k fp64 additions stay below
        1.2e5 * 2^-53 = 1.4e-11 relative - far under half an fp32 ulp - so only the final roundings (sqrt in fp64, then to fp32)
        remain, and a double rounding may land on the neighbour;
  coef  1 fp32 ulp of float32(max_norm / ref), by the same argument (one fp64 division, one rounding);
  scaled gradients: bit-equal to float32(g) * coef with the coefficient READ BACK (one fp32 multiplication, nothing to round twice).
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = 0x7FA5A5A5          # a NaN bit pattern: a guard element that is read poisons the norm, one that is written changes its bits
GUARD = 64                   # poison elements on either side of every tensor
SIZES = [1, 3, 4, 5, 16383, 16384, 16385, 40000]
ODD = 6                      # index of the tensor that starts at element offset 1 of a 16-byte boundary (the 16385: two chunks)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ref_norm(arrays):
    return math.sqrt(math.fsum(float(x) ** 2 for a in arrays for x in np.asarray(a, dtype=np.float32).reshape(-1)))


def _ulps(a, b):
    """Distance in fp32 ulps of two finite values of the same sign."""
    a, b = np.float32(a), np.float32(b)
    assert np.isfinite(a) and np.isfinite(b), (a, b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


class Case:
    """Tensors laid out in ONE host image with poison guard bands between them; `spans` = (first element, elements) per tensor."""

    def __init__(self, sizes, odd=(), seed=0, scale=1.0):
        rng = np.random.RandomState(seed)
        self.sizes, self.spans, off = list(sizes), [], 0
        for i, n in enumerate(sizes):
            off = (off + GUARD + 3) & ~3
            if i in odd:
                off += 1
            self.spans.append((off, n))
            off += n
        self.image = np.full(off + GUARD, POISON, dtype=np.uint32)
        self.inside = np.zeros(self.image.shape, dtype=bool)
        for a, n in self.spans:
            self.image[a:a + n] = (rng.randn(n) * scale).astype(np.float32).view(np.uint32)
            self.inside[a:a + n] = True

    def values(self, image=None):
        image = self.image if image is None else image
        return [image[a:a + n].view(np.float32) for a, n in self.spans]

    def run(self, dev, max_norm, scale=True, wgs=0):
        """-> (out float32[2], image after the calls, partial float64[n_chunks]) through the two C entry points."""
        from cim_amd import _lib
        from cim_amd.optim import clip
        buf = torch.from_numpy(self.image.view(np.int32).copy()).to(dev)
        assert buf.data_ptr() % 16 == 0
        n = len(self.sizes)
        table = np.array([buf.data_ptr() + 4 * a for a, _ in self.spans] + self.sizes, dtype=np.uint64)
        assert [int(p) % 16 for p in table[:n]] == [4 if (a & 3) else 0 for a, _ in self.spans]
        table = torch.from_numpy(table.view(np.int64)).to(dev)
        chunks = clip.chunk_table(self.sizes)
        n_chunks = len(chunks)
        chunks = torch.from_numpy(chunks.view(np.uint8).reshape(-1).copy()).to(dev)
        partial = torch.full((8 * n_chunks,), 0xFF, dtype=torch.uint8, device=dev)
        out = torch.full((8,), 0xFF, dtype=torch.uint8, device=dev)
        args = (table.data_ptr(), table.data_ptr() + 8 * n, n, chunks.data_ptr(), n_chunks)
        _lib.call("cim_grad_norm_multi", *args, partial.data_ptr(), float(max_norm), out.data_ptr(), wgs, _lib.stream_ptr())
        if scale:
            _lib.call("cim_grad_scale_multi", *args, out.data_ptr(), wgs, _lib.stream_ptr())
        torch.cuda.synchronize()
        return out.view(torch.float32).cpu().numpy(), buf.cpu().numpy().view(np.uint32), partial.view(torch.float64).cpu().numpy()

    def guards_untouched(self, image):
        return bool(np.all(image[~self.inside] == POISON))


@pytest.fixture(scope="module")
def big():
    rng = np.random.RandomState(11)
    sizes = SIZES + [int(v) for v in rng.randint(7, 301, size=40)]
    case = Case(sizes, odd=(ODD, len(SIZES) + 5), seed=1)
    case.ref = _ref_norm(case.values())
    return case


def test_norm_coefficient_and_scale_at_the_c_abi(dev, big):
    max_norm = 0.5 * big.ref
    out, image, partial = big.run(dev, max_norm)
    print("norm", out[0], "ref", big.ref, "coef", out[1], "ref", max_norm / big.ref)
    assert _ulps(out[0], np.float32(big.ref)) <= 1
    assert _ulps(out[1], np.float32(max_norm / big.ref)) <= 1
    assert np.all(np.isfinite(partial)) and abs(math.fsum(partial) / big.ref ** 2 - 1) < 1e-10       # every slot written
    for i, (g, got) in enumerate(zip(big.values(), big.values(image))):
        assert np.array_equal((g * out[1]).view(np.uint32), got.view(np.uint32)), (i, big.sizes[i])
    assert big.guards_untouched(image)


def test_result_does_not_depend_on_the_grid_or_the_run(dev, big):
    runs = [big.run(dev, 0.25 * big.ref, wgs=wgs) for wgs in (0, 1, 3, 0, 1, 3)]
    out0, image0, partial0 = runs[0]
    for out, image, partial in runs[1:]:
        assert np.array_equal(out.view(np.uint32), out0.view(np.uint32))
        assert np.array_equal(image, image0) and np.array_equal(partial.view(np.uint64), partial0.view(np.uint64))
    assert big.guards_untouched(image0)


def test_below_the_threshold_nothing_is_touched(dev, big):
    out, image, _ = big.run(dev, 2 * big.ref)
    assert out[1].view(np.uint32) == np.float32(1.0).view(np.uint32)
    assert _ulps(out[0], np.float32(big.ref)) <= 1
    assert np.array_equal(image, big.image)


def test_infinite_max_norm_is_norm_only(dev, big):
    out, image, _ = big.run(dev, float("inf"))
    assert out[1].view(np.uint32) == np.float32(1.0).view(np.uint32)
    assert _ulps(out[0], np.float32(big.ref)) <= 1
    assert np.array_equal(image, big.image)


def test_squares_that_overflow_fp32_are_summed_in_fp64(dev):
    case = Case([5, 300, 16385], odd=(1,), seed=2, scale=0.0)
    a, _ = case.spans[2]
    case.image[a + 7] = case.image[a + 16384] = np.float32(3e19).view(np.uint32)       # one in each chunk of the last tensor
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(3e19) * np.float32(3e19))
    ref = _ref_norm(case.values())
    out, image, _ = case.run(dev, 1e19)
    assert np.isfinite(out[0]) and _ulps(out[0], np.float32(ref)) <= 1 and _ulps(out[0], np.float32(3e19 * math.sqrt(2))) <= 1
    assert _ulps(out[1], np.float32(1e19 / ref)) <= 1
    assert image[a + 7] == (np.float32(3e19) * out[1]).view(np.uint32) and case.guards_untouched(image)


@pytest.mark.parametrize("where", [(0, 2), (1, 299), (2, 16384)])
def test_special_values(dev, where):
    ti, ei = where
    nan_case = Case([5, 300, 16385], odd=(1,), seed=3)
    a = nan_case.spans[ti][0]
    nan_case.image[a + ei] = np.float32(np.nan).view(np.uint32)
    out, image, _ = nan_case.run(dev, 1.0)
    assert np.isnan(out[0]) and np.isnan(out[1])
    assert all(np.all(np.isnan(v)) for v in nan_case.values(image)) and nan_case.guards_untouched(image)
    inf_case = Case([5, 300, 16385], odd=(1,), seed=3)
    inf_case.image[a + ei] = np.float32(np.inf).view(np.uint32)
    out, image, _ = inf_case.run(dev, 1.0)
    assert np.isposinf(out[0]) and out[1].view(np.uint32) == 0
    flat = np.concatenate(inf_case.values(image))
    assert int(np.isnan(flat).sum()) == 1 and np.all(flat[~np.isnan(flat)] == 0) and inf_case.guards_untouched(image)    # inf * 0


# ------------------------------------------------------------------ Python: GradClipper, clip_gradient
def _model(dev, seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.ReLU(), torch.nn.Linear(53, 11, bias=False)).to(dev)


def _set_grads(model, seed, in_place=False):
    """Fresh gradient tensors (as autograd hands out every step); -> their host copies."""
    g = torch.Generator().manual_seed(seed)
    host = []
    for p in model.parameters():
        v = torch.randn(p.shape, generator=g)
        if in_place:
            p.grad.copy_(v)
        else:
            p.grad = v.to(p.device)
        host.append(v.numpy().copy())
    return host


def _check_clipped(model, host, clip_norm, out=None):
    """float64 model of lib/utils/net.py:15.  Two fp32 roundings separate it from the device's result - the coefficient and
    the product, 2 * 2^-24 = 1.2e-7 - so rtol 2e-7; below the threshold the gradients are bit-unchanged."""
    ref = _ref_norm(host)
    coef = clip_norm / max(ref, clip_norm)
    for p, h in zip(model.parameters(), host):
        got = p.grad.detach().cpu().numpy()
        if coef == 1.0:
            assert np.array_equal(got, h)
        else:
            np.testing.assert_allclose(got.astype(np.float64), h.astype(np.float64) * coef, rtol=2e-7, atol=0)
    if out is not None:
        o = out.cpu().numpy()
        assert _ulps(o[0], np.float32(ref)) <= 1 and _ulps(o[1], np.float32(coef)) <= 1
    return ref


@pytest.mark.parametrize("factor", [0.3, 3.0])
def test_clip_gradient_and_clipper_match_the_float64_model(dev, factor):
    from cim_amd.optim import GradClipper
    from cim_amd.utils import net
    m = _model(dev)
    host = _set_grads(m, 1)
    clip_norm = factor * _ref_norm(host)
    versions = [p.grad._version for p in m.parameters()]
    assert net.clip_gradient(m, clip_norm) is None
    _check_clipped(m, host, clip_norm)
    assert m in net._CLIPPERS
    assert all(p.grad._version > v for p, v in zip(m.parameters(), versions))          # the raw-pointer write is visible to autograd
    host = _set_grads(m, 2)
    c = GradClipper(m.parameters())
    norm_only = c.norm().clone()
    assert norm_only[1].item() == 1.0 and _ulps(norm_only[0].item(), np.float32(_ref_norm(host))) <= 1
    out = c.clip(factor * _ref_norm(host))
    assert out.dtype == torch.float32 and out.shape == (2,) and out.device == next(m.parameters()).device
    _check_clipped(m, host, factor * _ref_norm(host), out)


@pytest.mark.parametrize("factor", [0.3, 3.0])
def test_clip_through_data_parallel_flat_gradients(dev, factor):
    from cim_amd.nn import DataParallel
    from cim_amd.utils import net
    m = _model(dev)
    dp = DataParallel(m, force_flat_grads=True)
    assert dp.world_size == 1 and dp.flat_grad is not None
    assert all(p.grad.data_ptr() >= dp.flat_grad.data_ptr() for p in m.parameters())   # views of the flat buffer
    host = _set_grads(m, 3, in_place=True)
    clip_norm = factor * _ref_norm(host)
    net.clip_gradient(dp, clip_norm)
    _check_clipped(m, host, clip_norm)
    flat = dp.flat_grad.cpu().numpy()
    np.testing.assert_allclose(math.sqrt(math.fsum(float(x) ** 2 for x in flat)), min(clip_norm, _ref_norm(host)), rtol=1e-6)   # padding stays 0


def test_conflicts_and_refused_gradients(dev, monkeypatch):
    from cim_amd import _lib
    from cim_amd.nn import DataParallel
    from cim_amd.ops import maskfuse_pair
    from cim_amd.optim import SGD, GradClipper
    from cim_amd.utils import net
    monkeypatch.setattr(maskfuse_pair, "DEFER_DW", maskfuse_pair.DEFER_DW)              # (attach_optimizer switches it off)
    m = _model(dev)
    dp = DataParallel(m)
    assert dp.attach_optimizer(SGD(m.parameters(), lr=0.1, momentum=0.9), early_modules=("0",))
    host = _set_grads(m, 4)
    with pytest.raises(_lib.CimHipError, match="attach_optimizer"):
        net.clip_gradient(dp, 1e-3)
    for p, h in zip(m.parameters(), host):
        assert np.array_equal(p.grad.cpu().numpy(), h)
    # a gradient that could only be scaled through a copy
    m = _model(dev)
    _set_grads(m, 5)
    w = m[0].weight
    w.grad = torch.randn(w.shape[1], w.shape[0], device=dev).t()
    assert not w.grad.is_contiguous()
    with pytest.raises(NotImplementedError):
        GradClipper(m.parameters()).clip(1e-3)
    with pytest.raises(NotImplementedError):
        net.clip_gradient(m, 1e-3)
    # CPU and GPU gradients in one model
    m = _model(dev)
    m[2].cpu()
    _set_grads(m, 6)
    assert not m[2].weight.grad.is_cuda and m[0].weight.grad.is_cuda
    with pytest.raises(_lib.CimHipError):
        net.clip_gradient(m, 1e-3)


def test_no_host_wait_and_replaced_gradient_tensors(dev, monkeypatch):
    from cim_amd.optim import GradClipper
    m = _model(dev)
    c = GradClipper(m.parameters())
    first = _set_grads(m, 7)
    c.clip(0.5 * _ref_norm(first))                      # warm-up: builds the tables
    old = [p.grad for p in m.parameters()]              # kept alive: the new tensors live at other addresses
    old_host = [g.cpu().numpy() for g in old]
    host = _set_grads(m, 8)
    assert all(p.grad.data_ptr() != o.data_ptr() for p, o in zip(m.parameters(), old))
    clip_norm = 0.5 * _ref_norm(host)

    def forbidden(*a, **k):
        raise AssertionError("host wait inside GradClipper")

    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "synchronize", forbidden)
        for name in ("item", "cpu", "tolist", "numpy"):
            mp.setattr(torch.Tensor, name, forbidden)
        out = c.clip(clip_norm)
        clipped = out.clone()
        again = c.norm()
    assert again is out                                  # the clipper's own buffer: norm() has overwritten clip()'s result
    _check_clipped(m, host, clip_norm, clipped)          # the NEW tensors were clipped ...
    # (the norm AFTER clipping: the coefficient's, the products' and the norm's own fp32 rounding, 3 * 2^-24 = 1.8e-7)
    assert abs(out[0].item() / clip_norm - 1) <= 1.8e-7 and out[1].item() == 1.0
    for o, h in zip(old, old_host):
        assert np.array_equal(o.cpu().numpy(), h)       # ... and the old ones left alone


@pytest.mark.parametrize("overlap", [False, True])
def test_clip_then_fused_sgd_step(dev, overlap):
    """clip_gradient + cim_amd.optim.SGD.step() against a float64 model of clip-then-SGD, within the bound of
    test_gpu_parity.py::test_fused_sgd_matches_torch_sgd (rtol 1e-5, atol 1e-6)."""
    from cim_amd.optim import SGD
    from cim_amd.utils import net
    m = _model(dev)
    lr, mom, wd = 0.05, 0.9, 0.01
    opt = SGD(m.parameters(), lr=lr, momentum=mom, weight_decay=wd)
    opt.overlap_update = overlap
    p64 = [p.detach().cpu().numpy().astype(np.float64) for p in m.parameters()]
    buf64 = [np.zeros_like(p) for p in p64]
    for step, factor in enumerate((0.4, 5.0, 0.7)):
        host = _set_grads(m, 20 + step)
        ref = _ref_norm(host)
        clip_norm = factor * ref
        net.clip_gradient(m, clip_norm)
        opt.step()
        coef = clip_norm / max(ref, clip_norm)
        for i, h in enumerate(host):
            buf64[i] = mom * buf64[i] + (h.astype(np.float64) * coef + wd * p64[i])
            p64[i] = p64[i] - lr * buf64[i]
    opt.wait_update()
    for p, want, b in zip(m.parameters(), p64, buf64):
        np.testing.assert_allclose(p.detach().cpu().numpy(), want, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(opt.state[p]["momentum_buffer"].cpu().numpy(), b, rtol=1e-5, atol=1e-6)
