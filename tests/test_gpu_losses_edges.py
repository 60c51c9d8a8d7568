"""-m gpu: the fused loss launch (cim_amd/csrc/losses.hip) at the cases of tests/golden/loss_cases.py - every column-pass
layout, row counts around the lane groups and the 64 KiB LDS limit, unlabelled rows, a class without a labelled row, an
unsaturated MIL term, tied maxima, scores on and around the clamp bounds, the PCL cluster shapes and the status word - against
oracle/losses.py (values) and the ATen formulation under autograd on the CPU (gradients), float64 (float32 where the clamps
saturate).  tests/test_loss_cases_cpu.py shows from the references alone that the cases reach what they are named for."""
import numpy as np
import pytest
import torch

import loss_refs
from loss_cases import LOSS_CASES, UP4, UP6, loss_case, status_mats

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from cim_amd import _lib
    _lib.load()          # fail loudly if the HIP extension is missing
    return torch.device("cuda:0")


def _inputs(case, dev, fused=False, mat=None):
    """-> (leaves [pc, pd, rc.., ri..] or the one score matrix, the arguments of heads.fused_losses)."""
    t = lambda a: torch.from_numpy(a).to(dev)
    R = case["R"]
    arrays = [case["pc"], case["pd"]] + case["rc"] + case["ri"]
    if fused:
        base = t(np.concatenate(arrays, axis=1)).requires_grad_(True)
        views = list(base.split(case["C1"], dim=1))
        leaves = [base]
    else:
        views = leaves = [t(a).requires_grad_(True) for a in arrays]
    pseudo = [tuple(t(a) for a in ps) for ps in case["pseudo"]]
    args = (views[0], views[1], views[2:2 + R], views[2 + R:], t(case["labels"]), pseudo, case["scales"],
            t(case["mat"] if mat is None else mat))
    return leaves, args, dict(valid=t(case["valid"]))


def _run(case, dev, up, fused=False):
    """One forward and backward: (outputs as fp32 numpy scalars, input gradients as numpy arrays)."""
    from cim_amd.modeling import heads
    leaves, args, kw = _inputs(case, dev, fused)
    if fused:
        assert heads._fused_base(*args[:4]) is leaves[0]
    out = heads.fused_losses(*args, with_total=len(up) == 6, **kw)
    sum(u * o for u, o in zip(up, out)).backward()
    grads = [torch.zeros_like(x) if x.grad is None else x.grad for x in leaves]
    return [o.detach().cpu().numpy() for o in out], [g.cpu().numpy() for g in grads]


def _check_grads(name, got, ref):
    """The project's criterion for these gradients: max|got - ref| <= 2e-5 max|ref| + 1e-9; exact zeros where the reference
    is exactly zero (skipped layers, gated-off elements, rows in no cluster, columns that are nobody's arg-max)."""
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape and np.isfinite(g).all()
        err, scale = float(np.abs(g - r).max()), float(np.abs(r).max())
        print("%s input %d: max|got - ref| %.3g, max|ref| %.3g, ratio %.3g" % (name, k, err, scale, err / (scale + 1e-300)))
        assert err <= 2e-5 * scale + 1e-9, "%s input %d" % (name, k)
        assert not g[r == 0].any(), "%s input %d: non-zero where the reference is exactly zero" % (name, k)


_RESULTS = {}


def _separate(name, dev):
    """The separate-tensor run of a case with the (0.7, 1.3, 2.0, 0.5) upstream weights, once per module."""
    if name not in _RESULTS:
        _RESULTS[name] = _run(loss_case(name), dev, UP4)
    return _RESULTS[name]


@pytest.mark.parametrize("name", LOSS_CASES)
def test_fused_losses_edge_case_parity(dev, name):
    """The four losses against oracle/losses.py (rtol 2e-5, atol 1e-7: fp32 sums in another order) and every input gradient
    against autograd through the ATen formulation.  Measured on MI355X: the worst gradient ratio is big_n:n15000's, where the
    fp32 rounding of the largest product rc * ri (1 - agg is 2e-4) alone costs the float32 ATen formulation 1.74e-5."""
    out, grads = _separate(name, dev)
    want = loss_refs.oracle_values(name)
    print("%s losses: got %s, reference %s" % (name, [float(x) for x in out], list(want)))
    np.testing.assert_allclose([float(x) for x in out], want, rtol=2e-5, atol=1e-7)
    _check_grads(name, grads, loss_refs.reference_grads(name))


@pytest.mark.parametrize("name", ["ties", "ties:c257"])
def test_tied_maxima_go_to_the_first_row(dev, name):
    """The bag gradient of every column sits exactly at the row np.argmax picks (the first maximum): among the labelled rows
    for a seen class, among all rows otherwise; nowhere for the seen class without a labelled row."""
    from cim_amd.modeling import heads
    case = loss_case(name)
    leaves, args, kw = _inputs(case, dev)
    bag = heads.fused_losses(*args, **kw)[0]
    bag.backward()
    seen = np.concatenate([[1.0], case["labels"].reshape(-1)]) == 1
    R = case["R"]
    for i in range(R):
        u = case["rc"][i] * case["ri"][i]                                  # exact in fp32 by construction
        member = case["pseudo"][i][0] != 0
        fi, ui = (u * member).argmax(0), u.argmax(0)
        for g in (leaves[2 + i].grad.cpu().numpy(), leaves[2 + R + i].grad.cpu().numpy()):
            for c in range(case["C1"]):
                rows = list(np.nonzero(g[:, c])[0])
                if seen[c] and not member[:, c].any():
                    assert rows == []
                else:
                    assert rows == [fi[c] if seen[c] else ui[c]], "layer %d column %d" % (i, c)


@pytest.mark.parametrize("name", ["g32_tail", "g64:c33", "g64:c64", "wave_col:c257", "wave_col:c300"])
def test_fused_score_matrix_layout(dev, name):
    """The eight scores as column blocks of ONE [N, 8 C1] matrix (ld = 8 C1, cim_loss_grad_combine), all six outputs, upstream
    gradients on each: the same kernel with another leading dimension, so bit-equal outputs; 3 iou and the total exact in
    fp32; one gradient matrix."""
    case = loss_case(name)
    sep, _ = _run(case, dev, UP6)
    out, (grad,) = _run(case, dev, UP6, fused=True)
    assert grad.shape == (case["N"], 8 * case["C1"])
    for a, b in zip(out, sep):
        assert a.dtype == F32 and a.tobytes() == b.tobytes()
    bag, pcl, cls, iou = (F32(x) for x in out[:4])
    assert out[4] == F32(3) * iou
    assert out[5] == ((bag + pcl) + cls) + F32(3) * iou
    ref = np.concatenate(loss_refs.reference_grads(name, UP6), axis=1)
    _check_grads(name + " (fused)", [grad], [ref])
    # ... and block by block, so that a small block is not judged by the largest block's scale
    _check_grads(name + " (fused blocks)", np.split(grad, 8, axis=1), np.split(ref, 8, axis=1))


@pytest.mark.parametrize("name", ["ties", "ties:c257", "wave_col:c257", "wave_col:c300"])
def test_two_launches_are_bit_equal(dev, name):
    a_out, a_grads = _separate(name, dev)
    b_out, b_grads = _run(loss_case(name), dev, UP4)
    for a, b in zip(a_out + a_grads, b_out + b_grads):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("bit", [4, 8, 16])
def test_pcl_format_errors_reach_the_status_word(dev, bit):
    """Rows with two non-zeros (4), two ids in column 0 (8), 257 clusters (16): reported through the device status word after
    a normal launch - as CimHipError when fused_losses owns the word, as the bit alone when the caller does."""
    from cim_amd import _lib
    from cim_amd.modeling import heads
    case = loss_case("pcl_shapes:k256")
    mat = status_mats()[bit]
    assert mat.shape == case["mat"].shape
    _, args, kw = _inputs(case, dev, mat=mat)
    with pytest.raises(_lib.CimHipError) as e:
        heads.fused_losses(*args, **kw)
    assert str(e.value) == heads.STATUS_BITS[bit]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = heads.fused_losses(*args, status=status, **kw)
    assert int(status.item()) == bit
    assert all(bool(torch.isfinite(o)) for o in out)
    with pytest.raises(_lib.CimHipError):
        heads.check_status(int(status.item()))


def test_losses_argument_checks(dev):
    """N above the documented cap and C1 = 1: cim_losses_fwd's argument check answers, nothing is launched."""
    from cim_amd import _lib
    from cim_amd.modeling import heads
    for n, c1 in ((15001, 21), (4, 1)):
        z = lambda *shape: torch.zeros(shape, device=dev)
        pseudo = [(z(n, c1), torch.zeros(n, dtype=torch.float16, device=dev), z(n))]
        with pytest.raises(_lib.CimHipError, match="cim_losses_fwd: bad argument"):
            heads.fused_losses(z(n, c1), z(n, c1), [z(n, c1)], [z(n, c1)], z(1, max(c1 - 1, 1)), pseudo, [1], z(n, c1))
    torch.cuda.synchronize()
