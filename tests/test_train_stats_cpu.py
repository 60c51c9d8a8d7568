"""cim_amd.utils.training_stats without a GPU: the host path against the golden captured from the reference's own TrainingStats
(tests/golden/make_golden_train_stats.py), the log lines, the header entries and the optional routing of install_as_lib."""
import contextlib
import io
import os
import sys
import types

import numpy as np
import pytest
import torch

import train_stats_cases as tsc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return tsc.load()


@pytest.fixture(autouse=True)
def own_cfg():
    from cim_amd.core import config as own
    own.reset_cfg()
    yield own.cfg
    own.reset_cfg()


@pytest.mark.parametrize("it", [1, 2, 3, 4, 5])
def test_host_path_equals_the_reference_bit_for_bit(golden, it):
    capture = [int(c) for c in golden["capture"]]
    _, totals, stats = tsc.drive(golden, it, lambda a: torch.from_numpy(a.copy()), capture=capture)
    assert all(t.dtype == torch.float32 and t.shape == (1,) for t in totals)
    assert np.array_equal(tsc.bits([t.item() for t in totals]), tsc.bits(golden["total/%d" % it]))
    keys = [str(k) for k in golden["keys"]]
    for i, c in enumerate(capture):
        s = stats[c]
        assert list(s) == ["iter", "time", "eta", "loss", "lr", "head_losses"] and s["iter"] == c
        assert list(s["head_losses"]) == keys
        assert type(s["loss"]) is np.float32
        assert tsc.bits(s["loss"]) == tsc.bits(golden["loss/%d" % it][i]), (it, c)
        assert np.array_equal(tsc.bits([s["head_losses"][k] for k in keys]), tsc.bits(golden["heads/%d" % it][i])), (it, c)


def test_a_supplied_total_loss_is_kept_and_extras_stay_out_of_the_total(golden):
    from cim_amd.utils.training_stats import TrainingStats
    ts = TrainingStats(types.SimpleNamespace(iter_size=1))
    row = golden["values/1"][0]
    mine = torch.tensor([123.0])
    out = dict(losses={k: torch.tensor([row[j]]) for j, k in enumerate(("a", "b", "c", "d"))}, total_loss=mine)
    ts.UpdateIterStats(out, extra={"grad_norm": torch.tensor([1e6])})
    assert out["total_loss"] is mine
    s = ts.GetStats(0, 0.1)
    assert list(s) == ["iter", "time", "eta", "loss", "lr", "head_losses", "grad_norm"] and s["grad_norm"] == np.float32(1e6)
    assert tsc.bits(s["loss"]) == tsc.bits(golden["total/1"][0])            # the statistic is the sum of the four, not 123 + 1e6
    with pytest.raises(ValueError, match="differ from the first"):
        ts.UpdateIterStats(dict(losses={"a": torch.tensor([1.0])}))
    assert ts.nonfinite_step() is None
    ts.UpdateIterStats(dict(losses={k: torch.tensor([float("inf") if k == "c" else 1.0]) for k in "abcd"}),
                       extra={"grad_norm": torch.tensor([1.0])})
    ts.UpdateIterStats(dict(losses={k: torch.tensor([float("nan")]) for k in "abcd"}), extra={"grad_norm": torch.tensor([1.0])})
    assert ts.nonfinite_step() == 2


def test_inner_iter_out_of_range_raises_and_the_gpu_count_is_checked(golden, own_cfg):
    from cim_amd.utils.training_stats import TrainingStats
    ts = TrainingStats(types.SimpleNamespace(iter_size=3))
    out = dict(losses={"a": torch.tensor([1.0])})
    with pytest.raises(AssertionError):
        ts.UpdateIterStats(out, 3)
    with pytest.raises(AssertionError):
        ts.UpdateIterStats(dict(losses={"a": torch.tensor([1.0, 2.0])}), 0)        # shape[0] != cfg.NUM_GPUS
    with pytest.raises(ValueError, match="window"):
        TrainingStats(types.SimpleNamespace(iter_size=1), window=65)


def test_several_gpu_rows_are_reduced_as_the_reference_does(own_cfg):
    from cim_amd.utils.training_stats import TrainingStats
    own_cfg.NUM_GPUS = 2
    ts = TrainingStats(types.SimpleNamespace(iter_size=1))
    rows = {"a": torch.tensor([1.5, 2.25]), "b": torch.tensor([1e-3, 3e3])}
    out = dict(losses=dict(rows), total_loss=torch.tensor([7.0, 7.0]))
    ts.UpdateIterStats(out)
    want = 0
    for v in rows.values():                                                  # training_stats.py:72-83
        want = want + v.mean(dim=0, keepdim=True)
    assert all(out["losses"][k].shape == (1,) and torch.equal(out["losses"][k], rows[k].mean(dim=0, keepdim=True)) for k in rows)
    assert out["total_loss"].shape == (1,) and torch.equal(out["total_loss"], want)
    assert ts.GetStats(0, 0.1)["loss"] == np.float32(want.item())


def test_log_stats_prints_the_reference_lines(golden, own_cfg, capsys):
    from cim_amd.utils import training_stats as mod
    own_cfg.SOLVER.MAX_ITER = int(golden["max_iter"])
    keys = [str(k) for k in golden["keys"]]
    time_s, eta, lr = [str(x) for x in golden["log_clock"]]
    stats = dict(iter=int(golden["log_iter"]), time=float(time_s), eta=eta, loss=golden["loss/5"][-1], lr=float(lr),
                 head_losses=dict(zip(keys, golden["heads/5"][-1])))
    run, cfg_file = [str(x) for x in golden["log_run"]]
    mod.log_stats(stats, types.SimpleNamespace(run_name=run, cfg_filename=cfg_file, iter_size=1))
    assert capsys.readouterr().out == str(golden["log_step"])
    e, s, n = [int(x) for x in golden["log_epoch_args"]]
    mod.log_stats(stats, types.SimpleNamespace(run_name=run, cfg_filename=cfg_file, iter_size=1, epoch=e, step=s, iters_per_epoch=n))
    assert capsys.readouterr().out == str(golden["log_epoch"])


def test_log_iter_stats_follows_the_period_and_the_last_iteration(golden, own_cfg):
    own_cfg.SOLVER.MAX_ITER = 30
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        tsc.drive(golden, 2, lambda a: torch.from_numpy(a.copy()), steps=30, on_step=lambda ts, step: ts.LogIterStats(step, 0.01),
                  log_period=20)
    heads = [ln for ln in buf.getvalue().splitlines() if ln.startswith("[")]
    assert [ln.split("[Step ")[1] for ln in heads] == ["1 / 30]", "21 / 30]", "30 / 30]"]
    assert ("loss: %.6f" % golden["loss/2"][4]) in buf.getvalue()              # the captured step 21


def test_the_header_declares_the_entries():
    from cim_amd import _lib
    text = open(os.path.join(REPO, "include", "cim_hip.h")).read()
    for name in ("cim_stats_bytes", "cim_stats_push", "cim_stats_summary"):
        assert name + "(" in text and name in _lib.SIGNATURES
    assert "cim_stats_bytes" in _lib.VALUE_RETURNING
    assert _lib.CONSTANTS["CIM_STATS_MAX_KEYS"] == 16 and _lib.CONSTANTS["CIM_STATS_MAX_WIN"] == 64
    assert _lib.ABI_VERSION == 16


def test_install_as_lib_routes_training_stats_only_on_request():
    import cim_amd
    name = "utils.training_stats"
    try:
        cim_amd.install_as_lib()
        assert name not in cim_amd.ALIASES and cim_amd._finder.find_spec(name) is None
        cim_amd.install_as_lib(route_training_stats=True)
        spec = cim_amd._finder.find_spec(name)
        mod = spec.loader.create_module(spec)
        assert mod.__name__ == "cim_amd.utils.training_stats" and callable(mod.TrainingStats) and callable(mod.log_stats)
        assert cim_amd._finder.find_spec("ops") is not None
    finally:
        cim_amd.uninstall_as_lib()
    assert cim_amd._finder.find_spec(name) is None
    assert cim_amd._finder.find_spec("ops") is not None                     # (the finder object itself still knows ALIASES)


def test_the_drivers_import_resolves_under_a_package_from_another_tree(tmp_path, monkeypatch):
    """tools/train.py:31 `from utils.training_stats import TrainingStats`: `utils` is the reference's own package, found on
    sys.path; only its sub-module is routed.  A stub package stands in for the reference tree."""
    import cim_amd
    (tmp_path / "utils").mkdir()
    (tmp_path / "utils" / "__init__.py").write_text("")
    (tmp_path / "utils" / "training_stats.py").write_text("TrainingStats = 'the stub tree: not routed'\n")
    (tmp_path / "utils" / "timer.py").write_text("WHO = 'stub'\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "utils" or k.startswith("utils.")}
    try:
        cim_amd.install_as_lib(route_training_stats=True)
        from utils.training_stats import TrainingStats
        import utils.timer
        assert TrainingStats.__module__ == "cim_amd.utils.training_stats" and utils.timer.WHO == "stub"      # (siblings stay the tree's own)
        assert sys.modules["utils.training_stats"].__name__ == "cim_amd.utils.training_stats"
        assert sys.modules["utils"].__file__.startswith(str(tmp_path))
        cim_amd.uninstall_as_lib()
        assert "utils.training_stats" not in sys.modules
        cim_amd.install_as_lib()
        from utils.training_stats import TrainingStats as unrouted
        assert unrouted == 'the stub tree: not routed'
    finally:
        cim_amd.uninstall_as_lib()
        for k in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
            del sys.modules[k]
        sys.modules.update(saved)
