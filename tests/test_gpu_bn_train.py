"""-m gpu: batch-statistics BatchNorm.  csrc/bn_train.hip straight at the C ABI - statistics, normalisation,
running buffers and backward against the float64 restatement (tests/golden/bn_train_np.py) inside bounds derived from the number
format, exact on integer data, with poisoned outputs, guard words, determinism, two streams and every refusal - then the operator
`ops.bn_act_train` against the float64 module in train() mode, the thin PRM network one block at a time, and the whole training
step after `prm_train.unfreeze` with `batch_stats=True` relative to what ATen's own fp32 shows."""
import copy
import os
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_train_np as bnp
import prm_cases
from cases import GRAD_RTOL, VANISHING, VANISHING_ATOL, gradient_deviation

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
U = 2.0 ** -24           # unit roundoff of fp32
SENT = 0x7FC0BEEF        # a quiet NaN: what every output and workspace float holds before a call
GUARD = 64
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from cim_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class _Guarded:
    """n floats preset to SENT between two runs of GUARD sentinel words."""

    def __init__(self, n, dev):
        self.n = n
        self.raw = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device=dev)
        self.ptr = self.raw.data_ptr() + 4 * GUARD

    def values(self):
        return self.raw[GUARD:GUARD + self.n].view(torch.float32)

    def untouched(self):
        return bool((self.raw[GUARD:GUARD + self.n] == SENT).all())

    def guards_ok(self):
        return bool((self.raw[:GUARD] == SENT).all()) and bool((self.raw[GUARD + self.n:] == SENT).all())

    def host(self, shape=None):
        got = self.values().clone()
        assert bool(torch.isfinite(got).all()), "an output element was not written (or is not finite)"
        assert self.guards_ok(), "a store outside an output or outside the workspace"
        got = got.cpu().numpy()
        return got if shape is None else got.reshape(shape)


def _ws_floats(shape):
    from cim_amd import _lib
    lib = _lib.load()
    k, nbytes = lib.cim_bn_train_chunks(*shape), lib.cim_bn_train_workspace(*shape)
    assert k == bnp.chunks(shape) and nbytes == (shape[1] * k + shape[1]) * 16
    return nbytes // 4


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run_fwd(dev, shape, x, gamma, beta, res=None, relu=True, momentum=0.1, running=None, stream=None):
    """One cim_bn_train_fwd call on poisoned, guarded buffers.  running: None or [running_mean, running_var, batches] device
    tensors, updated in place.  -> dict of host arrays y, mean, var, rstd."""
    from cim_amd import _lib
    n, c, hw = shape
    xs, rs, g, b = _t(x, dev), _t(res, dev), _t(gamma, dev), _t(beta, dev)
    y, mean, var, rstd, ws = _Guarded(n * c * hw, dev), _Guarded(c, dev), _Guarded(c, dev), _Guarded(c, dev), _Guarded(_ws_floats(shape), dev)
    rm, rv, nb = running if running is not None else (None, None, None)
    _lib.call("cim_bn_train_fwd", xs.data_ptr(), _lib.ptr(rs), g.data_ptr(), b.data_ptr(), EPS, momentum, _lib.ptr(rm), _lib.ptr(rv),
              _lib.ptr(nb), y.ptr, mean.ptr, var.ptr, rstd.ptr, n, c, hw, int(relu), ws.ptr,
              _lib.stream_ptr() if stream is None else stream.cuda_stream)
    (stream or torch.cuda.current_stream()).synchronize()
    assert ws.guards_ok(), "a store outside the workspace"
    return {"y": y.host(shape), "mean": mean.host(), "var": var.host(), "rstd": rstd.host()}


def run_bwd(dev, shape, dy, y, x, gamma, mean, rstd, relu=True, want=("dx", "dres", "affine"), stream=None):
    """One cim_bn_train_bwd call on poisoned, guarded buffers -> dict of host arrays dx, dres, dgamma, dbeta (those wanted)."""
    from cim_amd import _lib
    n, c, hw = shape
    ins = [_t(a, dev) for a in (dy, y, x, gamma, mean, rstd)]
    dx, dres = (_Guarded(n * c * hw, dev) if k in want else None for k in ("dx", "dres"))
    dg, db = (_Guarded(c, dev) if "affine" in want else None for _ in range(2))
    ws = _Guarded(_ws_floats(shape), dev)
    p = lambda gd: None if gd is None else gd.ptr
    _lib.call("cim_bn_train_bwd", *(t.data_ptr() for t in ins), p(dx), p(dres), p(dg), p(db), n, c, hw, int(relu), ws.ptr,
              _lib.stream_ptr() if stream is None else stream.cuda_stream)
    (stream or torch.cuda.current_stream()).synchronize()
    assert ws.guards_ok(), "a store outside the workspace"
    out = {}
    for name, gd, shp in (("dx", dx, shape), ("dres", dres, shape), ("dgamma", dg, None), ("dbeta", db, None)):
        if gd is not None:
            out[name] = gd.host(shp)
    return out


_CASES = {}


def case(shape, kind):
    """Inputs and float64 references of a (shape, data set), computed once and shared (never modified)."""
    key = (shape, kind)
    if key not in _CASES:
        n, c, hw = shape
        seed = 7 + len(_CASES)
        rs = np.random.RandomState(1000 + seed)
        x = bnp.seeded(shape, seed, kind)
        gamma, beta = bnp.seeded_affine(c, seed)
        res = rs.standard_normal(shape).astype(np.float32)
        dy = (rs.randint(-2, 3, shape) if kind == "d" else rs.standard_normal(shape)).astype(np.float32)
        mean, var, mag = bnp.stats(x)
        d = {"x": x, "gamma": gamma, "beta": beta, "res": res, "dy": dy, "mean": mean, "var": var, "mag": mag}
        # the backward is a function of ITS inputs: fp32 mean and rstd (the reference's, rounded) and an fp32 output as the mask
        d["mean32"], d["rstd32"] = mean.astype(np.float32), (1.0 / np.sqrt(var + EPS)).astype(np.float32)
        for relu in (True, False):
            y, _, _ = bnp.forward(x, gamma, beta, EPS, res, relu)
            d["y", relu] = y
            d["bwd", relu] = _backward_of_inputs(dy, x, y.astype(np.float32), gamma, d["mean32"], d["rstd32"], relu)
        _CASES[key] = d
    return _CASES[key]


def _backward_of_inputs(dy, x, y, gamma, mean32, rstd32, relu):
    """bnp.backward with the mean and rstd the call is GIVEN (float32 values, taken exactly)."""
    rstd = rstd32.astype(np.float64)
    return bnp.backward(dy, x, y, gamma, mean32.astype(np.float64), 1.0 / (rstd * rstd) - EPS, EPS, relu)


def mean_bound(m, mag):
    return (m + 1) * U * mag / m


def var_bound(m, mag, var):
    return (m + 4) * U * var + mean_bound(m, mag) ** 2


def _ratio(err, bound):
    return float(np.max(err / np.maximum(bound, 1e-300)))


# ---- 1. statistics, normalisation and backward against float64 ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["a", "b", "c"])
@pytest.mark.parametrize("shape", bnp.SHAPES)
def test_against_float64_within_derived_bounds(dev, shape, kind):
    from cim_amd import _lib
    n, c, hw = shape
    m = n * hw
    d = case(shape, kind)
    relu = (n + c + hw) % 2 == 0                 # (both forms over the shapes; the other tests fix it)
    got = run_fwd(dev, shape, d["x"], d["gamma"], d["beta"], d["res"], relu)

    # mean, variance: any fp32 summation order of m terms, centred
    em, ev = np.abs(got["mean"] - d["mean"]), np.abs(got["var"] - d["var"])
    bm, bv = mean_bound(m, d["mag"]), var_bound(m, d["mag"], d["var"])
    print("shape %s (%s)  m = %d  mean err / bound %.3g   var err / bound %.3g" % (shape, kind, m, _ratio(em, bm), _ratio(ev, bv)))
    assert np.all(em <= bm), "mean"
    assert np.all(ev <= bv), "variance (an uncentred formula fails here on data set b)"
    assert np.all(got["var"] >= 0)
    rstd = 1.0 / np.sqrt(got["var"].astype(np.float64) + EPS)        # (of the device's own variance: var + eps and rsqrtf round)
    assert np.all(np.abs(got["rstd"] - rstd) <= 4 * U * rstd)

    # y: cim_bn_act_fwd on the device's own batch statistics, bit for bit
    y2 = torch.empty(shape, dtype=torch.float32, device=dev)
    ins = [_t(a, dev) for a in (d["x"], d["res"], d["gamma"], d["beta"], got["mean"], got["var"])]       # (kept alive over the call)
    _lib.call("cim_bn_act_fwd", *(t.data_ptr() for t in ins), EPS, y2.data_ptr(), n, c, hw, int(relu), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(got["y"].view(np.uint32), y2.cpu().numpy().view(np.uint32))
    ref = d["y", relu]
    if kind == "a":
        err, top = float(np.abs(got["y"] - ref).max()), float(np.abs(ref).max())
        print("   y err / max |ref| %.3g" % (err / max(top, 1e-300)))
        assert err <= 5e-6 * top
    if kind == "c":
        # the constant channel: its mean is the constant, its variance 0, y = beta (+ res): what is left is the rounding of
        # b = beta - mean a and of the fused multiply-add, a = gamma / sqrt(eps)
        const = d["x"][0, 0, 0]
        assert got["mean"][0] == const and got["var"][0] == 0.0
        a = float(d["gamma"][0]) / np.sqrt(EPS)
        want = d["beta"][0].astype(np.float64) + d["res"][:, 0, :]
        want = np.maximum(want, 0.0) if relu else want
        tol = 4 * U * (abs(float(const)) * a + abs(float(d["beta"][0])) + np.abs(d["res"][:, 0, :]))
        assert np.all(np.abs(got["y"][:, 0, :] - want) <= tol)

    # backward, from the inputs it is given
    y32 = ref.astype(np.float32)
    b = run_bwd(dev, shape, d["dy"], y32, d["x"], d["gamma"], d["mean32"], d["rstd32"], relu)
    r = d["bwd", relu]
    e1, e2 = np.abs(b["dbeta"] - r["dbeta"]), np.abs(b["dgamma"] - r["dgamma"])
    b1, b2 = (m + 1) * U * r["mag1"], (m + 1) * U * r["mag2"] * r["rstd"]
    print("   dbeta (S1) err / bound %.3g   dgamma (rstd S2) err / bound %.3g" % (_ratio(e1, b1), _ratio(e2, b2)))
    assert np.all(e1 <= b1) and np.all(e2 <= b2)
    assert np.array_equal(b["dres"], (d["dy"] * (y32 > 0) if relu else d["dy"]).astype(np.float32))
    assert np.all(np.isfinite(b["dx"])) and np.all(np.isfinite(b["dgamma"]))
    worst, _, van = gradient_deviation({"dx": torch.from_numpy(b["dx"])}, {"dx": torch.from_numpy(r["dx"])})
    print("   dx deviation %.3g (vanishing: %.3g)" % (worst, van))


# ---- 2. exact ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 1), (1, 4, 2), (1, 2, 4096), (2, 2, 8192), (8, 3, 2048), (256, 2, 64), (128, 5, 8), (4, 2, 4096)])
def test_integers_give_the_mean_and_the_sums_exactly(dev, shape):
    """Integers in -2..2, m a power of two: the mean (k / m) and S1 = dbeta are exact whatever the chunking."""
    n, c, hw = shape
    m = n * hw
    assert m & (m - 1) == 0
    d = case(shape, "d")
    got = run_fwd(dev, shape, d["x"], d["gamma"], d["beta"], None, False)
    assert np.array_equal(got["mean"].astype(np.float64), d["mean"])
    assert np.all(np.abs(got["var"] - d["var"]) <= var_bound(m, d["mag"], d["var"]))
    for relu in (False, True):
        y = d["y", relu].astype(np.float32)
        b = run_bwd(dev, shape, d["dy"], y, d["x"], d["gamma"], d["mean32"], d["rstd32"], relu, want=("affine",))
        assert set(b) == {"dgamma", "dbeta"}
        assert np.array_equal(b["dbeta"].astype(np.float64), d["bwd", relu]["S1"])


# ---- 3. running buffers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("momentum", [0.1, None])
@pytest.mark.parametrize("shape", [(3, 5, 49), (2, 3, 9000)])
def test_running_buffers_two_calls_in_a_row(dev, shape, momentum):
    n, c, hw = shape
    m = n * hw
    rs = np.random.RandomState(3)
    rm, rv, batches = rs.uniform(-0.3, 0.3, c), rs.uniform(0.5, 2.0, c), 5
    running = [_t(rm.astype(np.float32), dev), _t(rv.astype(np.float32), dev), torch.full((), batches, dtype=torch.int64, device=dev)]
    rm, rv = rm.astype(np.float32).astype(np.float64), rv.astype(np.float32).astype(np.float64)
    slack_m, slack_v = np.zeros(c), np.zeros(c)
    for call, kind in enumerate(("a", "b")):
        d = case(shape, kind)
        run_fwd(dev, shape, d["x"], d["gamma"], d["beta"], None, True, -1.0 if momentum is None else momentum, running)
        rm, rv, batches = bnp.running_update(rm, rv, batches, d["mean"], d["var"], m, momentum)
        f = 1.0 / batches if momentum is None else momentum
        # what the statistics may be off by, carried through the update, and one rounding of the stored fp32 value per call
        slack_m = (1 - f) * slack_m + f * mean_bound(m, d["mag"]) + U * np.abs(rm)
        slack_v = (1 - f) * slack_v + f * var_bound(m, d["mag"], d["var"]) * m / (m - 1.0) + U * np.abs(rv)
        got_m, got_v = running[0].cpu().numpy().astype(np.float64), running[1].cpu().numpy().astype(np.float64)
        print("call %d momentum %s: running_mean err / bound %.3g  running_var err / bound %.3g"
              % (call, momentum, _ratio(np.abs(got_m - rm), slack_m), _ratio(np.abs(got_v - rv), slack_v)))
        assert int(running[2]) == batches == 6 + call
        assert np.all(np.abs(got_m - rm) <= slack_m) and np.all(np.abs(got_v - rv) <= slack_v)
    # without running buffers: nothing to update, the count may be absent
    d = case(shape, "a")
    run_fwd(dev, shape, d["x"], d["gamma"], d["beta"], None, True, 0.1, None)


# ---- 4. layout, determinism, refusals ------------------------------------------------------------------------------------------------
def _both(dev, shape, stream=None):
    d = case(shape, "a")
    f = run_fwd(dev, shape, d["x"], d["gamma"], d["beta"], d["res"], True, stream=stream)
    b = run_bwd(dev, shape, d["dy"], f["y"], d["x"], d["gamma"], f["mean"], f["rstd"], True, stream=stream)
    return [f[k] for k in ("y", "mean", "var", "rstd")] + [b[k] for k in ("dx", "dres", "dgamma", "dbeta")]


def _same_bits(a, b):
    return all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, b))


def test_two_calls_and_two_streams_give_the_same_bits(dev):
    shapes = [(2, 3, 9000), (200, 2, 41)]
    single = []
    for shape in shapes:
        a, b = _both(dev, shape), _both(dev, shape)
        assert _same_bits(a, b)
        single.append(a)
    torch.cuda.synchronize()
    errors = []

    def worker(k):
        try:
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                for it in range(4):
                    assert _same_bits(_both(dev, shapes[k], stream), single[k]), (k, it)
        except BaseException as e:                                    # noqa: BLE001 - reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_unaligned_tensors_take_the_scalar_form(dev):
    """A base 4 bytes off a 16-byte boundary: no 16-byte access may be issued; same results as the aligned call."""
    from cim_amd import _lib
    shape = (3, 5, 49)
    n, c, hw = shape
    d = case(shape, "a")
    want = run_fwd(dev, shape, d["x"], d["gamma"], d["beta"], None, True)
    buf = torch.zeros(n * c * hw + 1, dtype=torch.float32, device=dev)
    buf[1:] = _t(d["x"], dev).reshape(-1)
    g, b = _t(d["gamma"], dev), _t(d["beta"], dev)
    y, mean, var, rstd, ws = _Guarded(n * c * hw, dev), _Guarded(c, dev), _Guarded(c, dev), _Guarded(c, dev), _Guarded(_ws_floats(shape), dev)
    _lib.call("cim_bn_train_fwd", buf.data_ptr() + 4, None, g.data_ptr(), b.data_ptr(), EPS, 0.1, None, None, None, y.ptr, mean.ptr,
              var.ptr, rstd.ptr, n, c, hw, 1, ws.ptr, _lib.stream_ptr())
    torch.cuda.synchronize()
    m = n * hw
    assert np.all(np.abs(mean.host() - d["mean"]) <= mean_bound(m, d["mag"]))
    assert np.all(np.abs(var.host() - d["var"]) <= var_bound(m, d["mag"], d["var"]))
    assert float(np.abs(y.host(shape) - want["y"]).max()) <= 5e-6 * float(np.abs(want["y"]).max())


_FWD = ("x", "res", "gamma", "beta", "eps", "momentum", "running_mean", "running_var", "num_batches_tracked", "y", "mean", "var", "rstd",
        "N", "C", "HW", "relu", "workspace")
_BWD = ("dy", "y", "x", "gamma", "mean", "rstd", "dx", "dres", "dgamma", "dbeta", "N", "C", "HW", "relu", "workspace")
REFUSED = {
    # name -> (entry, argument overrides, what the message must name)
    "fwd-x": ("fwd", {"x": None}, "x"),
    "fwd-gamma": ("fwd", {"gamma": None}, "gamma"),
    "fwd-beta": ("fwd", {"beta": None}, "beta"),
    "fwd-y": ("fwd", {"y": None}, "y"),
    "fwd-mean": ("fwd", {"mean": None}, "mean"),
    "fwd-var": ("fwd", {"var": None}, "var"),
    "fwd-workspace": ("fwd", {"workspace": None}, "workspace"),
    "fwd-running-half": ("fwd", {"running_var": None}, "running_var"),
    "fwd-count-missing": ("fwd", {"momentum": -1.0, "num_batches_tracked": None}, "num_batches_tracked"),
    "fwd-C0": ("fwd", {"C": 0}, "C"),
    "fwd-N0": ("fwd", {"N": 0}, "N"),
    "fwd-HW0": ("fwd", {"HW": 0}, "HW"),
    "fwd-m1": ("fwd", {"N": 1, "HW": 1}, "N * HW"),
    "fwd-overflow": ("fwd", {"N": 65536, "C": 65536, "HW": 1}, "N * C * HW"),
    "bwd-dy": ("bwd", {"dy": None}, "dy"),
    "bwd-x": ("bwd", {"x": None}, "x"),
    "bwd-gamma": ("bwd", {"gamma": None}, "gamma"),
    "bwd-mean": ("bwd", {"mean": None}, "mean"),
    "bwd-rstd": ("bwd", {"rstd": None}, "rstd"),
    "bwd-y-with-relu": ("bwd", {"y": None}, "y"),
    "bwd-workspace": ("bwd", {"workspace": None}, "workspace"),
    "bwd-affine-half": ("bwd", {"dbeta": None}, "dbeta"),
    "bwd-C0": ("bwd", {"C": 0}, "C"),
    "bwd-m1": ("bwd", {"N": 1, "HW": 1}, "N * HW"),
    "bwd-overflow": ("bwd", {"N": 32768, "C": 32768, "HW": 2}, "N * C * HW"),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_refusals_launch_nothing(dev, what):
    from cim_amd import _lib
    lib = _lib.load()
    entry, over, names = REFUSED[what]
    n, c, hw = 2, 3, 5
    ins = {k: torch.ones(n * c * hw if k in ("x", "res", "dy", "y") else c, device=dev) for k in ("x", "res", "dy", "y", "gamma", "beta", "mean", "rstd")}
    outs = {k: _Guarded(n * c * hw if k in ("y", "dx", "dres") else c, dev)
            for k in ("y", "mean", "var", "rstd", "dx", "dres", "dgamma", "dbeta", "running_mean", "running_var")}
    ws = _Guarded(_ws_floats((n, c, hw)), dev)
    count = torch.full((), 7, dtype=torch.int64, device=dev)
    a = {"eps": EPS, "momentum": 0.1, "N": n, "C": c, "HW": hw, "relu": 1, "workspace": ws.ptr, "num_batches_tracked": count.data_ptr()}
    if entry == "fwd":
        a.update({k: ins[k].data_ptr() for k in ("x", "res", "gamma", "beta")})
        written = ("y", "mean", "var", "rstd", "running_mean", "running_var")
    else:
        a.update({k: ins[k].data_ptr() for k in ("dy", "y", "x", "gamma", "mean", "rstd")})
        written = ("dx", "dres", "dgamma", "dbeta")
    a.update({k: outs[k].ptr for k in written})
    a.update(over)
    order = _FWD if entry == "fwd" else _BWD
    rc = getattr(lib, "cim_bn_train_" + entry)(*(a[k] for k in order), _lib.stream_ptr())
    torch.cuda.synchronize()
    msg = lib.cim_last_error().decode()
    assert rc == -1 and "cim_bn_train_" + entry in msg and names in msg, msg
    assert all(outs[k].untouched() and outs[k].guards_ok() for k in outs) and ws.untouched() and ws.guards_ok()
    assert int(count) == 7


# ---- 5. the operator -----------------------------------------------------------------------------------------------------------------
def _deviation(name, got, want):
    got, want = got.detach().cpu().double(), want.detach().double()
    err, norm = float((got - want).norm()), float(want.norm())
    print("%-40s |g| %.3e  err / |g| %.2e" % (name, norm, err / max(norm, 1e-300)))
    if norm / np.sqrt(want.numel()) < VANISHING:
        assert err / np.sqrt(want.numel()) <= VANISHING_ATOL, name
    else:
        assert err <= GRAD_RTOL * norm, name


def _bn(c, seed, momentum=0.1):
    torch.manual_seed(seed)
    bn = torch.nn.BatchNorm2d(c, momentum=momentum)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-0.3, 0.3)
        bn.running_var.uniform_(0.5, 2.0)
    return bn


def _buffers_close(bn, rbn, x64):
    """The module's running buffers against the float64 module's, inside what the statistics' bounds leave: every update is a
    convex combination of the old value and the batch's statistic, so the statistic's bound holds for the buffer after any
    number of calls on the same batch - plus the roundings of the stored fp32 values."""
    m = x64.numel() // x64.shape[1]
    mag = x64.abs().sum((0, 2, 3)).numpy()
    var = x64.var((0, 2, 3), unbiased=False).numpy()
    rm, rv = rbn.running_mean.numpy(), rbn.running_var.numpy()
    assert int(bn.num_batches_tracked) == int(rbn.num_batches_tracked)
    assert np.all(np.abs(bn.running_mean.cpu().numpy() - rm) <= mean_bound(m, mag) + 4 * U * (np.abs(rm) + 1.0))
    assert np.all(np.abs(bn.running_var.cpu().numpy() - rv) <= var_bound(m, mag, var) * m / (m - 1.0) + 4 * U * (np.abs(rv) + 1.0))


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("shape", [(3, 5, 7, 7), (2, 64, 28, 28)])
def test_operator_against_the_float64_module_in_train_mode(dev, shape, with_res, relu):
    from cim_amd import _lib
    from cim_amd.ops import bn_act, bn_act_train, fallback
    momentum = 0.1 if relu else None
    bn = _bn(shape[1], 3 + shape[1], momentum)
    rbn = copy.deepcopy(bn).double().train()
    bn = bn.to(dev).eval()                       # the operator does not look at bn.training
    torch.manual_seed(11)
    x, res, weight = torch.randn(shape) * 1.5 + 0.3, torch.randn(shape), torch.randn(shape, dtype=torch.float64)
    x64, res64 = x.double().requires_grad_(True), res.double().requires_grad_(True)
    ref = rbn(x64) + (res64 if with_res else 0.0)
    ref = F.relu(ref) if relu else ref
    (ref * weight).sum().backward()

    fallback.reset()
    xd, rd = x.to(dev).requires_grad_(True), res.to(dev).requires_grad_(True)
    y = bn_act_train(xd, bn, residual=rd if with_res else None, relu=relu)
    (y * weight.float().to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert fallback.counts() == {}
    ref = ref.detach()
    assert float((y.detach().cpu().double() - ref).abs().max()) <= 5e-6 * float(ref.abs().max())
    _deviation("dx", xd.grad, x64.grad)
    if with_res:
        _deviation("dres", rd.grad, res64.grad)
    else:
        assert rd.grad is None
    _deviation("bn.weight", bn.weight.grad, rbn.weight.grad)
    _deviation("bn.bias", bn.bias.grad, rbn.bias.grad)
    _buffers_close(bn, rbn, x64.detach())

    # under no_grad the buffers move all the same; a second call
    with torch.no_grad():
        y2 = bn_act_train(xd.detach(), bn, residual=rd.detach() if with_res else None, relu=relu)
        rbn(x64.detach())
    assert torch.equal(y2, y.detach()) and not y2.requires_grad
    _buffers_close(bn, rbn, x64.detach())

    # refusals on the device; the frozen-statistics operator keeps refusing a module in training mode
    with pytest.raises(ValueError, match="contiguous"):
        bn_act_train(xd.detach().permute(0, 1, 3, 2)[:, :, :, ::2], bn)
    with pytest.raises(ValueError, match="float32"):
        bn_act_train(xd.detach().double(), bn)
    bn.train()
    with pytest.raises(_lib.CimHipError, match="BatchNorm in training mode"):
        bn_act(xd.detach(), bn)
    assert any(k == ("bn_act", "BatchNorm in training mode") for k in fallback.counts())
    fallback.reset()


def test_operator_without_running_statistics(dev):
    from cim_amd.ops import bn_act_train
    bn = torch.nn.BatchNorm2d(5, track_running_stats=False).to(dev)
    rbn = copy.deepcopy(bn).cpu().double()
    x = torch.randn(3, 5, 7, 7)
    y = bn_act_train(x.to(dev), bn, relu=False)
    ref = rbn(x.double())
    assert float((y.detach().cpu().double() - ref).abs().max()) <= 5e-6 * float(ref.abs().max())
    assert bn.running_mean is None and bn.num_batches_tracked is None


# ---- 6. the thin PRM network -----------------------------------------------------------------------------------------------------------
def _thin_model(seed_offset=0):
    from cim_amd import prm
    d = np.load(os.path.join(GOLDEN, "prm_net.npz"))
    seed, gain = int(d["seed"]) + seed_offset, float(d["gain"])
    model = prm.PeakResponseMapping(prm.fc_resnet50(prm_cases.NUM_CLASSES, width=prm_cases.WIDTH))
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = prm_cases.seeded_weights(shapes, seed, gain / 10.0)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return model, seed


def _train_mode_copy(model, dtype):
    """A CPU copy in `dtype` with every BatchNorm in train() mode (the container itself refuses train())."""
    ref = copy.deepcopy(model).cpu().to(dtype)
    for mod in ref.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.training = True
    return ref


def _images(seed, count, side):
    return prm_cases.normalise(prm_cases.seeded_images(seed, count, side, side))


def test_network_one_block_at_a_time(dev):
    """The stem and each of the 16 bottlenecks of the thin network on the float64 copy's own input and upstream gradient: the
    output inside 5e-6 of its maximum per fused layer, summed and doubled; every parameter gradient under the project's rule.
    (ATen's fp32 stays at or below 1.1e-6 here; the whole network does not - see the end-to-end test.)"""
    from cim_amd import prm_train
    from cim_amd.ops import fallback
    model, seed = _thin_model()
    prm_train.unfreeze(model)
    ref = _train_mode_copy(model, torch.float64)
    model = model.to(dev)
    images = torch.from_numpy(_images(seed, 4, 128)).double()

    # the float64 pass, keeping every block's input and output
    f = ref[0].features
    stem_out = f[2](f[1](f[0](images)))
    stem_out.retain_grad()
    x = f[3](stem_out)
    x.retain_grad()
    record = []
    for i in range(4, 8):
        for j, block in enumerate(f[i]):
            out = block(x)
            out.retain_grad()
            record.append((i, j, x, out))
            x = out
    crm = ref[0].classifier(x)
    torch.manual_seed(1)
    (crm * torch.randn(crm.shape, dtype=torch.float64)).sum().backward()
    assert len(record) == 16

    fallback.reset()
    df = model[0].features
    worst_out = 0.0

    def params(dmods, rmods, prefix):
        for dm, rm in zip(dmods, rmods):
            for (name, p), (_, q) in zip(dm.named_parameters(), rm.named_parameters()):
                assert p.grad is not None and q.grad is not None, prefix + name
                _deviation(prefix + name, p.grad, q.grad)

    out = prm_train._stem_batch_stats(images.float().to(dev), df[0], df[1])
    out.backward(stem_out.grad.float().to(dev))
    torch.cuda.synchronize()
    err = float((out.detach().cpu().double() - stem_out.detach()).abs().max()) / float(stem_out.abs().max())
    print("stem: output err / max %.3g" % err)
    assert err <= 2 * 1 * 5e-6
    params((df[0], df[1]), (f[0], f[1]), "stem.")
    for i, j, xin, xout in record:
        dblock, rblock = df[i][j], f[i][j]
        layers = 3 if rblock.downsample is None else 4
        xd = xin.detach().float().to(dev).requires_grad_(True)
        out = prm_train._bottleneck_batch_stats(dblock, xd)
        out.backward(xout.grad.float().to(dev))
        torch.cuda.synchronize()
        err = float((out.detach().cpu().double() - xout.detach()).abs().max()) / float(xout.abs().max())
        worst_out = max(worst_out, err / (2 * layers * 5e-6))
        print("layer%d[%d]: output err / max %.3g (bound %.1e)" % (i - 3, j, err, 2 * layers * 5e-6))
        assert err <= 2 * layers * 5e-6
        params((dblock,), (rblock,), "layer%d.%d." % (i - 3, j))
        _deviation("layer%d.%d.dx" % (i - 3, j), xd.grad, xin.grad)
    assert fallback.counts() == {}
    print("worst output err / bound over the blocks: %.3g" % worst_out)


def _reference_step(ref, images, target, mask):
    """loss.backward() of a CPU copy through torch with the device's peak map as a constant mask -> (loss, {name: grad})."""
    dt = next(ref.parameters()).dtype
    crm = ref[0](images.to(dt))
    up = F.interpolate(crm, scale_factor=8, mode="bilinear", align_corners=True)
    mask = mask.to(dt)
    loss = F.multilabel_soft_margin_loss((up * mask).sum((2, 3)) / mask.sum((2, 3)), target.to(dt))
    loss.backward()
    return float(loss.detach()), {k: p.grad for k, p in ref.named_parameters()}


def _relative(got, want):
    got, want = got.detach().cpu().double(), want.detach().double()
    return float((got - want).norm()) / max(float(want.norm()), 1e-300)


def _stat_deviation(model, ref):
    worst = 0.0
    want = dict(ref.named_buffers())
    for k, b in model.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(want[k]), k
        else:
            w = want[k].double()
            worst = max(worst, float((b.detach().cpu().double() - w).abs().max()) / float(w.abs().max()))
    return worst


def test_unfrozen_training_step_with_batch_statistics_relative_to_aten(dev):
    """prm_train.unfreeze, then one prm_train.loss(..., batch_stats=True).backward() of the thin network: no fallback, every
    parameter a finite gradient, and - against the float64 copy with every BatchNorm in train(), the device's peak map as a
    constant mask - a loss error, a worst and a median parameter-gradient deviation and a worst running-statistic deviation
    within 4 times what an fp32 CPU copy run through torch shows against the same float64 copy.  (Under GRAD_RTOL no fp32
    implementation passes at this depth: ATen's worst deviation is 1.2e-2 .. 2.9e-2 over seeds.  Not used here.)"""
    from cim_amd import prm_train
    from cim_amd.ops import fallback
    model, seed = _thin_model()
    prm_train.unfreeze(model)
    ref64, ref32 = _train_mode_copy(model, torch.float64), _train_mode_copy(model, torch.float32)
    model = model.to(dev)
    images = torch.from_numpy(_images(seed, 4, 128))
    target = torch.from_numpy((np.random.RandomState(2).rand(4, prm_cases.NUM_CLASSES) < 0.3).astype(np.float32))

    fallback.reset()
    agg, state = prm_train.aggregate(model, images.to(dev), batch_stats=True)
    loss = prm_train.multilabel_soft_margin_loss(agg, target.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    assert fallback.counts() == {}
    assert int(state.status.abs().sum()) == 0
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name

    mask = state.peak_map().cpu()
    loss64, g64 = _reference_step(ref64, images, target, mask)
    loss32, g32 = _reference_step(ref32, images, target, mask)
    dev_dev = np.array([_relative(p.grad, g64[k]) for k, p in model.named_parameters()])
    dev_aten = np.array([_relative(g32[k], g64[k]) for k, _ in model.named_parameters()])
    rows = (("loss error", abs(float(loss) - loss64), abs(loss32 - loss64)),
            ("worst gradient deviation", dev_dev.max(), dev_aten.max()),
            ("median gradient deviation", float(np.median(dev_dev)), float(np.median(dev_aten))),
            ("worst running-statistic deviation", _stat_deviation(model, ref64), _stat_deviation(ref32, ref64)))
    for what, ours, aten in rows:
        print("%-36s device %.3e   ATen fp32 %.3e   ratio %.2f" % (what, ours, aten, ours / max(aten, 1e-300)))
    for what, ours, aten in rows:
        assert ours <= 4.0 * aten, what


def test_default_path_keeps_its_bits_and_frozen_stages_their_buffers(dev):
    from cim_amd import prm_train
    from cim_amd.ops import conv1x1_bn_act, conv7x7_bn_act, max_pool2d
    model, seed = _thin_model()
    model = model.to(dev)
    prm_train.freeze(model, 2)
    x = torch.from_numpy(_images(seed, 2, 128)).to(dev)
    target = torch.from_numpy((np.random.RandomState(2).rand(2, prm_cases.NUM_CLASSES) < 0.3).astype(np.float32)).to(dev)

    def step(**kw):
        for p in model.parameters():
            p.grad = None
        loss = prm_train.loss(model, x, target, **kw)
        loss.backward()
        torch.cuda.synchronize()
        return [loss.detach().clone()] + [p.grad.clone() for p in model.parameters() if p.requires_grad]

    before = {k: b.clone() for k, b in model.named_buffers()}
    a, b = step(), step(batch_stats=False)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert all(torch.equal(before[k], v) for k, v in model.named_buffers())
    # the composition `class_response_maps` had before the argument existed
    f = model[0].features
    with torch.no_grad():
        y = max_pool2d(conv7x7_bn_act(x, f[0], f[1], relu=True), f[3])
        for i in range(4, 8):
            y = f[i](y)
        conv = model[0].classifier[0]
        old = conv1x1_bn_act(y, conv, prm_train._identity_bn(y.device, conv.out_channels), relu=False)
        assert torch.equal(old, prm_train.class_response_maps(model, x))

    step(batch_stats=True)
    moved = 0
    for k, v in model.named_buffers():
        frozen = k.startswith(("0.features.1.", "0.features.4."))
        if frozen:
            assert torch.equal(before[k], v), k
        elif k.endswith("num_batches_tracked"):
            assert int(v) == int(before[k]) + 1, k
        else:
            moved += int(not torch.equal(before[k], v))
    assert moved == 2 * sum(1 for k in before if k.endswith("running_mean") and not k.startswith(("0.features.1.", "0.features.4.")))
