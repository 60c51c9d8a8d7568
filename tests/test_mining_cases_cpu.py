"""The cases of tests/golden/mining_cases.py are not vacuous: from oracle/mining.py and the inputs alone (no GPU), every case
reaches the branch of cim_amd/csrc/mining.hip it is named for - a case that stops doing so after a seed changes fails HERE, not
silently on the GPU.  Also pins the oracle's three tie rules against plain NumPy on hand-written examples, so
that the reference of the tied cases is self-evident, and the form cim_mining_layout reports for every case."""
import numpy as np
import pytest

import mining_cases as mc
from mining_cases import CASES, F16, F32, LAYER_CASES, mining_case, reference
from oracle import mining as om

CON_LO, CON_EQ, CON_HI = mc.f16_steps(mc.CON_THR)
NMS_LO, NMS_EQ, NMS_HI = mc.f16_steps(mc.CLS_THR)


def _col(case, q, what="cls", li=0):
    return case["layers"][li][what][:, case["active"][q] + 1]


# ------------------------------------------------------------------ the oracle's tie rules on hand-written examples
def test_rule_stable_descending_sort():
    x = np.array([0.5, 0.75, 0.5, 0.75, 0.25, 0.5, 0.75, 0.25], F32)
    assert list(om.stable_argsort_desc(x)) == [1, 3, 6, 0, 2, 5, 4, 7] == sorted(range(8), key=lambda i: (-x[i], i))
    assert list(mc.topk(x, 4)) == [1, 3, 6, 0]


def test_rule_first_index_argmax():
    row = np.array([[0.25, 0.75, 0.5, 0.75, 0.0, 0.75, 0.25, 0.5]], F16)
    labels = np.eye(8, 9, 1, dtype=F32)
    _, _, w, idx = om.assign(row, labels, np.arange(8, dtype=F32), 0.25, 0.5)
    first = next(j for j in range(8) if row[0, j] == row[0].max())
    assert list(idx) == [first] == [1] and list(w) == [1.0]
    # the containment arg-max (heads.py:393-394): equal detector scores among the containing proposals -> the lowest index
    n = 8
    iou, asy = np.eye(n, dtype=F16), np.eye(n, dtype=F16)
    asy[[2, 5, 6], 0] = 1
    cls, det = np.full((n, 2), 0.5, F32), np.full((n, 2), 0.25, F32)
    cls[0, 1] = 0.75                                                      # proposal 0 is the one seed (K = 1)
    det[[5, 2], 1] = 0.75
    trace = {}
    om.cim_label(cls, det, np.ones((1, 1), F32), iou, asy, 0.1, 0.25, 0.85, trace)
    assert list(trace["keep_nms_idx"][0]) == [0] and list(trace["res_per_seed"][0]) == [2] == list(trace["res_idx"][0])


def test_rule_arbitration_is_strict():
    """Classes in ascending order, `>` deciding: on equal weights the LOWEST class keeps the proposal."""
    preds = np.array([[0.5, 0.5], [0.25, 0.5], [0.5, 0.25], [0.75, 0.75], [0.25, 0.75], [0.5, 0.5], [0.75, 0.25], [0.25, 0.25]], F32)
    trace = {}
    om.mist_label(preds, np.ones((1, 2), F32), np.eye(8, dtype=F16), 1.0, 0.25, trace)
    got = trace["gt_labels_full"].argmax(1) - 1
    assert list(got) == [0, 1, 0, 0, 1, 0, 0, 0] == [int(np.argmax(r)) for r in preds]
    np.testing.assert_array_equal(trace["gt_weights_full"], preds.max(1))


# ------------------------------------------------------------------ every case
@pytest.mark.parametrize("name", list(CASES))
def test_case_inputs_are_what_the_issue_asks_for(name):
    case = mining_case(name)
    n, C, k = case["N"], case["C"], case["K"]
    assert C in (20, 80) and k == int(np.ceil(0.1 * n)) and case["labels"].shape == (1, C)
    assert list(np.nonzero(case["labels"].reshape(-1))[0]) == case["active"]
    iou, asy = case["iou"], case["asy"]
    thrs = {t for l in case["layers"] for t in (l["cls_thr"], l["iou_thr"], l["con_thr"])}
    if name in LAYER_CASES:
        thrs.add(mc.HUGE_CON_THR)                                         # (the four variants share one pair of maps)
    grid = set(mc.value_grid(sorted(thrs))) | {F16(1)}
    for m in (iou, asy):
        assert m.shape == (n, n) and m.dtype == F16 and (np.diagonal(m) == 1).all()
        assert set(np.unique(m)) <= grid                                  # (no NaN: it is not on the grid)
    assert (iou == iou.T).all() and not (asy == asy.T).all()
    for l in case["layers"]:
        for s in (l["cls"], l["det"]):
            assert s.shape == (n, C + 1) and s.dtype == F32 and (s > 0).all() and (s <= 1).all()
        assert (l["cls"] * 32 == np.round(l["cls"] * 32)).all()
        assert "fine_det" in CASES[name]["plants"] or (l["det"] * 32 == np.round(l["det"] * 32)).all()
    ref = reference(name)
    np.random.seed(case["seed"])                                          # the stream ends `used` doubles behind its seed
    np.random.random_sample(ref["used"])
    assert np.random.random_sample() == ref["probe"]


@pytest.mark.parametrize("name", list(CASES))
def test_case_layout(name):
    """row_lds (bit 1) up to and including N = 2041, the gather form from N = 2043 on; det_lds (bit 0) everywhere."""
    from cim_amd import _lib
    case = mining_case(name)
    n, k = case["N"], case["K"]
    want = 3 if n <= 2041 else 1
    assert n != 2042 and case["layout"] == want == int(_lib.call("cim_mining_layout", n, k))


def test_layout_boundaries():
    from cim_amd import _lib
    lay = lambda n, k: int(_lib.call("cim_mining_layout", n, k))
    assert [lay(n, 205) for n in (2040, 2041, 2042, 2043)] == [3, 3, 1, 1]       # 256 / 257 sixteen-byte pieces per row
    assert lay(2000, 256) == 3 and lay(2000, 257) == 1                          # KW = 4 / 5
    assert lay(0, 0) == 0 and lay(64, 7) == 3
    for n in (64, 300, 1000, 2041, 2042, 2049, 2561, 8192):
        for k in (int(np.ceil(0.1 * n)), 256, 257, 1024):
            if k <= n:
                assert lay(n, k) == mc.seed_layout(n, k), (n, k)


# cim_mining_lds_bytes(N, K): the dynamic LDS of the mining launch = max(seed carve, arbitration carve), pinned as literals
LDS_BYTES = {
    # every (N, K) of CASES
    (64, 7): 6912, (70, 7): 7216, (200, 20): 12240, (300, 30): 16320, (301, 31): 16368, (500, 50): 24208, (1001, 101): 44640,
    (1500, 150): 66000, (2041, 205): 89728, (2043, 205): 25779, (2049, 205): 25833, (2561, 257): 31360,
    (2040, 204): 89632,                              # 255 / 256 (above) sixteen-byte pieces per streamed row: the last two row_lds sizes
    (2000, 256): 90640, (2000, 257): 28528,          # KW = 4 / 5
    (2456, 1024): 163840, (2457, 1024): 151552,      # the largest N with the detector column in LDS at K = 1024, and the next
    (8192, 820): 143456, (8192, 1024): 151552,
    (8192, 64): 78864, (4096, 16): 41232,            # the arbitration carve (16 K + 4096 + 9 N + 16) above the seed carve
    (1, 1): 4448,
}


def test_lds_bytes_are_pinned():
    from cim_amd import _lib
    assert {(c["n"], int(np.ceil(0.1 * c["n"]))) for c in CASES.values()} <= set(LDS_BYTES)
    for (n, k), want in LDS_BYTES.items():
        assert int(_lib.call("cim_mining_lds_bytes", n, k)) == want, (n, k)
    arb = lambda n, k: 16 * k + 4096 + 9 * n + 16
    assert LDS_BYTES[8192, 64] == arb(8192, 64) and LDS_BYTES[4096, 16] == arb(4096, 16) and LDS_BYTES[8192, 820] > arb(8192, 820)
    lay = lambda n, k: int(_lib.call("cim_mining_layout", n, k))
    assert [lay(2456, 1024) & 1, lay(2457, 1024) & 1] == [1, 0]


# ------------------------------------------------------------------ ties at the top-K boundary
def _boundary(case, q):
    col, k = _col(case, q), case["K"]
    t = col[mc.topk(col, k)[-1]]
    need = k - int((col > t).sum())
    tied = np.nonzero(col == t)[0]
    return t, need, tied


@pytest.mark.parametrize("name", ["ties_n64", "ties_n300", "ties_n1500"])
def test_ties_more_keys_equal_the_kth_value_than_fit(name):
    case, ref = mining_case(name), reference(name)
    rk = mc.keys_per_lane(case["N"])
    for q in range(len(case["active"])):
        t, need, tied = _boundary(case, q)
        assert t == case["plant"]["tie_value"][q] and 1 <= need < len(tied)
        got = ref["traces"][0]["keep_sort_idx"][q]
        np.testing.assert_array_equal(np.sort(got[_col(case, q)[got] == t]), tied[:need])      # the lowest indices are in
        waves = {int(i) // rk >> 6 for i in tied}
        if name == "ties_n64":
            assert rk == 1 and waves == {0}              # 64 proposals, one key per lane: every key sits in wave 0 (see ties_n300)
        elif name == "ties_n300":
            assert rk == 1 and len(waves) >= 3
        else:
            assert rk == 2 and len(waves) >= 3
            a, b, c = (int(x) for x in tied[need - 1:need + 2])
            assert a % 2 == 0 and b == a + 1             # the cut lies between a lane's own two keys ...
            assert (a // 2) & 63 == 63 and c // 2 >> 6 > a // 2 >> 6      # ... of a wave's last lane: the run goes on in the next wave


# ------------------------------------------------------------------ equality at every threshold
def _row_max(case, ref):
    return ref["traces"][0]["overlaps"].max(axis=1)


def _check_planted_rows(case, ref):
    """One row per value: nothing in common with any pseudo GT (ignore), cls_thr and iou_thr exactly, one step below and above."""
    rows = case["plant"]["rows"]
    out, best = ref["outs"][0], _row_max(case, ref)
    np.testing.assert_array_equal(best[rows], np.array(mc.ROW_VALUES, F16))
    z, c_lo, c_eq, c_hi, i_lo, i_eq, i_hi = rows
    assert not out[0][z].any() and out[2][z] == 0                         # ignore: no label, no weight
    assert out[0][c_lo, 0] == 1 and out[0][c_lo].sum() == 1               # below cls_thr: background
    for r in (c_eq, c_hi, i_lo, i_eq, i_hi):
        assert out[0][r, 0] == 0 and out[0][r].sum() == 1 and out[2][r] > 0        # at cls_thr and above: foreground
    assert [float(out[1][r]) for r in rows] == [0, 0, 0, 0, 0, 0, 1]      # only one step above iou_thr is an IoU label of 1
    # tied maxima across lanes of the assignment (lane = column % 64): the first column wins
    ov, idx = ref["traces"][0]["overlaps"], ref["traces"][0]["max_overlap_idx"]
    for r in rows:
        cols = np.nonzero(ov[r] == best[r])[0]
        assert len(cols) >= 2 and cols[0] % 64 != cols[1] % 64 and idx[r] == cols[0]


def test_thr_case_sits_on_every_threshold():
    case, ref = mining_case("thr_n70"), reference("thr_n70")
    trace, plant, iou, asy = ref["traces"][0], case["plant"], case["iou"], case["asy"]
    n = case["N"]
    # mask-IoU NMS: the leading candidate against the next three
    a, b, c, d = plant["nms"]
    assert list(trace["keep_sort_idx"][0][:4]) == [a, b, c, d]
    assert (iou[a, b], iou[a, c], iou[a, d]) == (NMS_EQ, NMS_LO, NMS_HI) and NMS_LO < NMS_EQ == F16(0.25) < NMS_HI
    seeds = list(trace["keep_nms_idx"][0])
    assert seeds[0] == a and b not in seeds and d not in seeds and seeds[1] == c
    # containment: three proposals with the column's largest detector score at, below and above con_thr
    s, i_lo, i_eq, i_hi = plant["con"]
    det = _col(case, 0, "det")
    assert s == a and i_lo < i_eq < i_hi and (asy[i_lo, s], asy[i_eq, s], asy[i_hi, s]) == (CON_LO, CON_EQ, CON_HI)
    assert CON_LO < CON_EQ == F16(0.85) < CON_HI and trace["asy_iou_flag"][[i_lo, i_eq, i_hi], 0].all()
    assert list(np.nonzero(det == det.max())[0]) == [i_lo, i_eq, i_hi]
    assert trace["res_per_seed"][0][0] == i_hi
    # the flag count at 0.9 N exactly, one less and one more
    assert plant["huge_limit"] == 63 == 0.9 * n
    counts = (asy[plant["huge_rows"]] > CON_EQ).sum(axis=1)
    assert list(counts) == [62, 63, 64] and list(trace["asy_iou_flag"][plant["huge_rows"], 0]) == [True, False, False]
    for r in plant["huge_rows"]:
        assert (asy[r] == CON_EQ).any() and (asy[r] == CON_LO).any()
    _check_planted_rows(case, ref)


def test_argmax_case_has_ties_in_both_argmaxes():
    case, ref = mining_case("argmax_n200"), reference("argmax_n200")
    trace, asy = ref["traces"][0], case["asy"]
    for q, key in ((0, "cross"), (1, "same")):
        s, i_a, i_b = case["plant"]["argmax"][key]
        det = _col(case, q, "det")
        assert trace["keep_nms_idx"][q][0] == s and i_a < i_b
        cand = (asy[:, s] > CON_EQ) & trace["asy_iou_flag"][:, 0]
        assert list(np.nonzero(cand & (det == det[cand].max()))[0]) == [i_a, i_b]
        assert (i_a // 8 != i_b // 8) == (key == "cross")                 # a lane of the containment step holds 8 consecutive proposals
        assert trace["res_per_seed"][q][0] == i_a
    _check_planted_rows(case, ref)                                        # assignment ties across lanes, an ignored row, best == cls_thr


# ------------------------------------------------------------------ odd N, the largest streamed row, the gather forms
@pytest.mark.parametrize("name", ["odd_n301", "odd_n1001", "row_last_n2041", "gather_n2043", "gather_n2049", "gather_kw5_n2561"])
def test_odd_sizes_reach_every_shift_and_the_last_proposal(name):
    case, ref = mining_case(name), reference(name)
    n, k = case["N"], case["K"]
    trace = ref["traces"][0]
    assert n % 2 == 1 and trace["keep_sort_idx"][0][0] == n - 1 == trace["keep_nms_idx"][0][0]
    cand = np.unique(np.concatenate(trace["keep_sort_idx"]))
    assert {int(i) * n & 7 for i in cand} == set(range(8))               # the row's first entry against its 16-byte boundary
    pieces, kw, rk = (2 * n + 14 + 15) // 16, (k + 63) // 64, mc.keys_per_lane(n)
    want = {"odd_n301": (3, 1, 1), "odd_n1001": (3, 1, 2), "row_last_n2041": (3, 2, 4), "gather_n2043": (1, 2, 4),
            "gather_n2049": (1, 3, 4), "gather_kw5_n2561": (1, 3, 5)}[name]
    assert (case["layout"], rk, kw) == want
    assert (pieces <= 256) == (name in ("odd_n301", "odd_n1001", "row_last_n2041")) and (name != "row_last_n2041" or pieces == 256)
    _check_planted_rows(case, ref)


def test_kw5_case_scans_five_blocks_and_sums_above_one_leaf():
    case, ref = mining_case("gather_kw5_n2561"), reference("gather_kw5_n2561")
    trace, iou, k = ref["traces"][0], case["iou"], case["K"]
    assert k == 257                                                       # four full 64-blocks and a fifth with ONE candidate
    last_kept = []
    for q in range(2):
        order, seeds = trace["keep_sort_idx"][q], trace["keep_nms_idx"][q]
        pos = {int(p): j for j, p in enumerate(order)}
        kept = sorted(pos[int(s)] for s in seeds)
        assert {j // 64 for j in kept} >= {0, 1, 2, 3}
        last_kept.append(256 in kept)
        crossing = 0
        for j in sorted(set(range(k)) - set(kept)):                       # a removed candidate's suppressor: the first kept one before it
            i = next(i for i in kept if i < j and not iou[order[i], order[j]] < NMS_EQ)
            crossing += i // 64 != j // 64
        assert crossing >= 3
    assert sorted(last_kept) == [False, True]                            # the fifth block's candidate: kept in one class, removed in the other
    assert max(trace["class_members"]) > 128                             # NumPy's pairwise sum recurses (blocks of 128)
    # ... and its order decides the sample: np.random.choice restated (cdf of p = w / total, searchsorted on the stream's doubles)
    # once with NumPy's total, once with the total of ONE leaf over the whole list (8 accumulators, no halving)
    def one_leaf(w):
        r = [F32(x) for x in w[:8]]
        m = len(w) - len(w) % 8
        for i in range(8, m, 8):
            r = [F32(a + b) for a, b in zip(r, w[i:i + 8])]
        s = F32(F32(F32(r[0] + r[1]) + F32(r[2] + r[3])) + F32(F32(r[4] + r[5]) + F32(r[6] + r[7])))
        for x in w[m:]:
            s = F32(s + x)
        return s

    def keep_mask(total_of):
        u = np.random.RandomState(case["seed"]).random_sample(ref["used"])
        gt_class = trace["gt_labels_full"].argmax(1)[trace["gt_idxs"]] - 1
        keep, o = np.zeros(len(gt_class), bool), 0
        for c, w in zip(case["active"], trace["class_weights"]):
            cdf = (w / total_of(w)).astype(np.float64).cumsum()
            cdf /= cdf[-1]
            keep[np.nonzero(gt_class == c)[0][cdf.searchsorted(u[o:o + len(w)], side="right")]] = True
            o += len(w)
        return keep

    np.testing.assert_array_equal(keep_mask(np.sum), trace["sample_keep"])
    assert (keep_mask(one_leaf) != trace["sample_keep"]).any()
    assert any(len(w) > 128 and w.sum() != one_leaf(w) for w in trace["class_weights"])


# ------------------------------------------------------------------ arbitration between many classes
@pytest.mark.parametrize("name,n_act", [("classes_c20_all", 20), ("classes_c80_40", 40)])
def test_classes_cases_arbitrate_between_many(name, n_act):
    case, ref = mining_case(name), reference(name)
    trace, layer = ref["traces"][0], case["layers"][0]
    assert len(case["active"]) == n_act == len(trace["res_idx"])
    preds = layer["cls"][:, 1:] * layer["det"][:, 1:]
    listed = {}
    for q, c in enumerate(case["active"]):
        for p in trace["res_idx"][q]:
            listed.setdefault(int(p), []).append(c)
    multi = {p: cs for p, cs in listed.items() if len(cs) >= 2}
    assert len(multi) >= 10
    equal = 0
    gt_class = trace["gt_labels_full"].argmax(1) - 1
    for p, cs in multi.items():
        w = preds[p, cs]
        winners = [c for c in cs if preds[p, c] == w.max()]
        assert gt_class[p] == winners[0] and trace["gt_weights_full"][p] == w.max()
        equal += len(winners) >= 2
    assert equal >= 3


# ------------------------------------------------------------------ several layers in one launch
@pytest.mark.parametrize("name", LAYER_CASES)
def test_layer_cases(name):
    case, ref = mining_case(name), reference(name)
    layers, meta = case["layers"], ref["meta"]
    assert len(layers) == 3 and [(l["cls_thr"], l["iou_thr"]) for l in layers] == mc.LAYER_THRESHOLDS
    slots = []
    for l in layers:
        if l["using_cim"] and l["con_thr"] not in slots:
            slots.append(l["con_thr"])
    valid = [g > 0 for g, _ in meta]
    sampling = [l["sampling"] and v for l, v in zip(layers, valid)]
    assert ref["used"] == sum(g for (g, _), s in zip(meta, sampling) if s)
    if name == "layers_r3_all":
        assert all(sampling) and len(slots) == 1 and all(gk < g for g, gk in meta)
    elif name == "layers_r3_g0":
        assert valid == [False, True, True] and sampling == [False, True, True] and len(slots) == 2
        assert not ref["traces"][0]["asy_iou_flag"].any() and ref["outs"][0] == (None, None, None)
        assert all(len(s) > 0 for s in ref["traces"][0]["keep_nms_idx"])       # seeds, but every containing proposal is huge
        assert all((r == -1).all() for r in ref["traces"][0]["res_per_seed"])
    elif name == "layers_r3_nosample":
        assert sampling == [True, False, True] and meta[1][0] == meta[1][1] and "sample_keep" not in ref["traces"][1]
    else:
        assert [l["using_cim"] for l in layers] == [False, True, True] and all(sampling)
        assert "res_per_seed" not in ref["traces"][0] and len(slots) == 1
    assert all(meta[i][0] > 0 for i in (1, 2))                            # the later layers start behind layer 0's share of the stream
