"""-m gpu: the mining launches (cim_amd/csrc/mining.hip) on the cases of tests/golden/mining_cases.py - ties at the top-K
boundary, equality at every threshold, tied arg-maxes, odd N, the largest row-streamed size, the gather forms of the NMS
bit-matrix, many classes, several layers in one launch - through heads.CIM_layer / heads.mine_step, against oracle/mining.py.
Every result is an index or a copy of an input: bit-identical, no tolerances.  tests/test_mining_cases_cpu.py shows from the
oracle alone that each case reaches what it is named for."""
import numpy as np
import pytest
import torch

from mining_cases import LAYER_CASES, SINGLE_CASES, expected, mining_case, reference

pytestmark = pytest.mark.gpu

# which form of the seed phase each case runs, as cim_mining_layout reports it: bit 0 = detector column and flags in LDS, bit 1 =
# the NMS bit-matrix from whole rows streamed through LDS (else K x K gathers)
ROWS, GATHER = 3, 1
FORM = {"ties_n64": ROWS, "ties_n300": ROWS, "ties_n1500": ROWS, "thr_n70": ROWS, "argmax_n200": ROWS, "odd_n301": ROWS,
        "odd_n1001": ROWS, "row_last_n2041": ROWS, "gather_n2043": GATHER, "gather_n2049": GATHER, "gather_kw5_n2561": GATHER,
        "classes_c20_all": ROWS, "classes_c80_40": ROWS, "layers_r3_all": ROWS, "layers_r3_g0": ROWS, "layers_r3_nosample": ROWS,
        "layers_r3_mist": ROWS}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from cim_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _dev_inputs(case, dev):
    t = lambda a: torch.from_numpy(a.copy()).to(dev)
    return t(case["labels"]), t(case["iou"]), t(case["asy"]), [(t(l["cls"]), t(l["det"])) for l in case["layers"]]


def _check_form(case):
    from cim_amd import _lib
    assert int(_lib.call("cim_mining_layout", case["N"], case["K"])) == FORM[case["name"]] == case["layout"]


def _module(l):
    from cim_amd.modeling import heads
    return heads.CIM_layer(0.1, l["cls_thr"], l["iou_thr"], l["con_thr"], Anti_noise_sampling=l["sampling"])


def _np(t):
    return t.cpu().numpy()


def _compare(case, ref, li, got, out):
    """got: topk / seeds / res [n_active, K], n_seeds, gt_class, gt_weight, asy_flag, pre_keep, max_idx as NumPy arrays, in the
    order a mismatch is to be located: the first differing intermediate names the phase."""
    layer, trace, want = case["layers"][li], ref["traces"][li], expected(case, ref, li)
    tag = "%s layer %d: " % (case["name"], li)
    for key in ("topk", "n_seeds", "seeds") + (("res",) if layer["using_cim"] else ()) + ("gt_class", "gt_weight"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=tag + key)
    if layer["using_cim"]:
        np.testing.assert_array_equal(got["asy_flag"].astype(bool), trace["asy_iou_flag"][:, 0], err_msg=tag + "asy_flag")
    g, gk = ref["meta"][li]
    assert (got["G"], got["Gk"]) == (g, gk), tag + "(G, G')"
    if g == 0:
        return
    if layer["sampling"]:
        np.testing.assert_array_equal(got["pre_keep"][:g].astype(bool), trace["sample_keep"], err_msg=tag + "sample_keep")
    np.testing.assert_array_equal(got["max_idx"], trace["max_overlap_idx"], err_msg=tag + "max_overlap_idx")
    assert out[1].dtype == torch.float16
    for k, what in enumerate(("pseudo_labels", "pseudo_iou_labels", "loss_weights")):
        np.testing.assert_array_equal(_np(out[k]), ref["outs"][li][k], err_msg=tag + what)


@pytest.mark.parametrize("name", SINGLE_CASES)
def test_single_layer_case_bit_identical_to_oracle(dev, name):
    case, ref = mining_case(name), reference(name)
    _check_form(case)
    labels, iou, asy, scores = _dev_inputs(case, dev)
    layer = _module(case["layers"][0])
    np.random.seed(case["seed"])
    out = layer(scores[0][0], scores[0][1], None, labels, iou, asy, using_CIM=True)
    probe = np.random.random_sample()
    assert out[0] is not None and ref["outs"][0][0] is not None
    last = layer.last
    got = {k: _np(last[k]) for k in ("topk", "seeds", "res", "n_seeds", "gt_class", "gt_weight", "asy_flag")}
    got.update(G=last["G"], Gk=int(last["gt_idx"].numel()), pre_keep=last["sample_keep"], max_idx=_np(last["max_overlap_idx"]))
    _compare(case, ref, 0, got, out)
    assert probe == ref["probe"], "NumPy's stream position differs from the reference's"


@pytest.mark.parametrize("name", LAYER_CASES)
def test_layers_in_one_launch_bit_identical_to_sequential_oracle(dev, name):
    from cim_amd.modeling import heads
    case, ref = mining_case(name), reference(name)
    _check_form(case)
    labels, iou, asy, scores = _dev_inputs(case, dev)
    layers = [_module(l) for l in case["layers"]]
    np.random.seed(case["seed"])
    res = heads.mine_step(layers, scores, labels, iou, asy, [l["using_cim"] for l in case["layers"]]).commit()
    heads.settle_rng()
    probe = np.random.random_sample()
    torch.cuda.synchronize()
    host = res.host.numpy()
    C, K, active = case["C"], case["K"], case["active"]
    valid = _np(res.valid)
    np.testing.assert_array_equal(valid != 0, [g > 0 for g, _ in ref["meta"]])
    for li, d in enumerate(res.debug):
        got = {k: _np(d[k].view(C, K))[active] for k in ("topk", "seeds", "res")}
        got.update({k: _np(d[k]) for k in ("gt_class", "gt_weight", "pre_keep", "max_idx")})
        got["n_seeds"] = _np(d["n_seeds"])[active]
        got["asy_flag"] = _np(d["asy_flag"]) if d["asy_flag"] is not None else None
        got["G"], got["Gk"] = int(host[2 + 2 * li]), int(host[3 + 2 * li])
        _compare(case, ref, li, got, res.pseudo[li])
    assert [(int(host[2 + 2 * i]), int(host[3 + 2 * i])) for i in range(3)] == ref["meta"]
    assert int(host[0]) == ref["used"] and probe == ref["probe"]
    assert int(host[1]) == 0 and int(res.status.cpu()) == 0
    # the launch's meeting words are left as the caller handed them over (include/cim_hip.h: cim_mining_step)
    scratch = [v for (d, _), v in heads._SYNC.items() if d == dev.index]
    assert scratch and all(int(v.abs().sum()) == 0 for v in scratch)
