"""Seeded inputs of the mining launches (cim_amd/csrc/mining.hip) at the sizes and values where the kernels take another path,
shared by tests/test_mining_cases_cpu.py and tests/test_gpu_mining_edges.py.  No stored arrays and no masks: the two maps are
synthesised directly from a small fp16 grid - 0, the binary16 value of every threshold in use and its fp16 neighbour on either
side (1 on the diagonals) - and the scores are multiples of 1 / 32 in (0, 1), so ties and equalities are the rule, not an accident.
Integer draws of the legacy RandomState only (no libm call): bit-identical on every host.

`mining_case(name)` -> dict(N, C, K, labels [1, C], iou / asy [N, N] f16, layers = [dict(cls, det [N, C+1] f32, cls_thr, iou_thr,
con_thr, sampling, using_cim)], seed = what np.random is seeded with before the run, layout = the expected cim_mining_layout(N, K),
plant = the indices the case planted on purpose).  `reference(name)` -> the oracle's run of the case (oracle/mining.py)."""
import functools

import numpy as np

F16, F32 = np.float16, np.float32
CLS_THR, IOU_THR, CON_THR = 0.25, 0.5, 0.85                  # CIM_layer's defaults (nms_thr = cls_thr, heads.py:227)
LAYER_THRESHOLDS = [(0.25, 0.5), (0.35, 0.6), (0.45, 0.7)]   # model_builder.py:90-93
HUGE_CON_THR = 2.0 ** -10                                    # layers_r3_g0: nearly every map entry lies above it
LEVELS = 32                                                  # scores are k / 32, k = 1 .. 31; planted maxima are 1.0


def f16_steps(thr):
    """(the fp16 value below, binary16(thr), the fp16 value above) of a positive threshold."""
    bits = int(np.array([F16(thr)]).view(np.uint16)[0])
    return tuple(np.array([bits + d], np.uint16).view(F16)[0] for d in (-1, 0, 1))


def value_grid(thresholds):
    vals = {F16(0)}
    for t in thresholds:
        vals.update(f16_steps(t))
    return np.array(sorted(vals), F16)


def seed_layout(n, k):
    """cim_mining_layout(N, K) restated: bit 0 = detector column and flags in LDS, bit 1 = the NMS matrix from streamed rows."""
    up16 = lambda v: (v + 15) & ~15
    kw = (k + 63) // 64
    o = 4096
    for b in (k * 8, k * kw * 8, k * 4, k * 4):
        o = up16(o + b)
    det = up16(n * 4) + up16(n)
    det_lds = int(o + det <= 160 * 1024)
    if det_lds:
        o += det
    pieces = (2 * n + 14 + 15) // 16
    row_lds = int(pieces <= 256 and kw <= 4 and o + 16 * pieces * 16 <= 156 * 1024)
    return det_lds | row_lds << 1


def keys_per_lane(n):
    return (n + 1023) >> 10


def topk(score, k):
    """Stable descending top-k: ties keep the lower index."""
    return np.argsort(-score, kind="stable")[:k]


# name: N, C, active classes, seed, thresholds on the grid; p0 = per-mille of zeros in (iou, asy); plants
_SINGLE = dict(cls_thr=CLS_THR, iou_thr=IOU_THR, con_thr=CON_THR, sampling=True, using_cim=True)
# What each case reaches (asserted case by case in tests/test_mining_cases_cpu.py):
#   ties_*            more keys equal the K-th score than fit (the select's tie scan); 64 proposals are ONE wave of keys, so the spread
#                     of the tied keys over three waves is ties_n300's; ties_n1500: two keys per lane, the cut between a lane's own two
#   thr_n70           a pair / row exactly at, one fp16 step below and above nms_thr, con_thr, cls_thr, iou_thr; flag counts 0.9 N, +-1
#   argmax_n200       tied containment arg-maxes across lanes and inside one; tied assignment columns; an ignored row; best == cls_thr
#   odd_*             odd N: every shift of a streamed row against its 16-byte boundary, the last proposal among the candidates
#   row_last_n2041    the largest row-streamed size (256 pieces);  gather_n2043 / n2049 / kw5_n2561: the gather form with 2 and 3
#                     keys per lane and with KW = 5 (five 64-blocks in the greedy scan, a class list above one pairwise-sum leaf)
#   classes_*         20 / 40 active classes: proposals listed by several classes, some with equal weights
#   layers_r3_*       three layers in one launch: all sampling / layer 0 without pseudo GT (and a second flag slot) / the middle layer
#                     not sampling / layer 0 as MIST
CASES = {
    "ties_n64": dict(n=64, C=20, active=[3, 11], seed=101, p0=(600, 600), plants=["ties"]),
    "ties_n300": dict(n=300, C=20, active=[3, 11], seed=102, p0=(600, 600), plants=["ties"]),
    "ties_n1500": dict(n=1500, C=20, active=[0, 7, 19], seed=103, p0=(900, 900), plants=["ties"]),
    "thr_n70": dict(n=70, C=20, active=[2, 17], seed=104, p0=(600, 600), plants=["huge3", "rows", "nms3", "con3"]),
    "argmax_n200": dict(n=200, C=20, active=[5, 6], seed=105, p0=(600, 600), plants=["rows", "argmax"]),
    "odd_n301": dict(n=301, C=20, active=[1, 18], seed=106, p0=(600, 600), plants=["last", "rows"]),
    "odd_n1001": dict(n=1001, C=20, active=[4, 9], seed=107, p0=(850, 900), plants=["last", "rows"]),
    "row_last_n2041": dict(n=2041, C=20, active=[0, 19], seed=108, p0=(900, 950), plants=["last", "rows"]),
    "gather_n2043": dict(n=2043, C=20, active=[8, 13], seed=109, p0=(900, 950), plants=["last", "rows"]),
    "gather_n2049": dict(n=2049, C=80, active=[0, 31, 64, 79], seed=110, p0=(900, 950), plants=["last", "rows"]),
    "gather_kw5_n2561": dict(n=2561, C=20, active=[6, 14], seed=411, p0=(996, 996), plants=["last", "rows", "fine_det"],
                             run_seed=165860),       # (a NumPy stream on which one ulp of a class's weight sum changes the sample)
    "classes_c20_all": dict(n=300, C=20, active=list(range(20)), seed=112, p0=(600, 600), plants=[], levels=8),
    "classes_c80_40": dict(n=500, C=80, active=list(range(0, 80, 2)), seed=113, p0=(700, 700), plants=[], levels=8),
}
_R3 = dict(n=300, C=20, active=[2, 9, 15], seed=120, p0=(600, 10), plants=[], r=3, thin=(HUGE_CON_THR,))
LAYER_VARIANTS = {
    "layers_r3_all": {},
    "layers_r3_g0": {0: dict(con_thr=HUGE_CON_THR)},          # every proposal huge under layer 0's own con_thr: G = 0, two flag slots
    "layers_r3_nosample": {1: dict(sampling=False)},
    "layers_r3_mist": {0: dict(using_cim=False)},
}
for _name in LAYER_VARIANTS:
    CASES[_name] = dict(_R3, variant=_name)
SINGLE_CASES = [n for n in CASES if n not in LAYER_VARIANTS]
LAYER_CASES = list(LAYER_VARIANTS)
ROW_VALUES = [F16(0)] + list(f16_steps(CLS_THR)) + list(f16_steps(IOU_THR))      # the planted rows' maxima ("rows")


def _draw_map(rs, n, grid, p0, thin, symmetric):
    """[n, n] f16 of grid values: p0 per mille zeros, the rest uniform over the non-zero grid values - except the `thin` ones
    (and their lower neighbours), which are drawn 20 times more rarely; diagonal 1."""
    weights = np.array([0 if v == 0 else (1 if any(v <= F16(t) for t in thin) else 20) for v in grid])
    table = np.repeat(np.arange(len(grid)), weights).astype(np.uint8)
    idx = table[rs.randint(0, len(table), size=(n, n))]
    idx[rs.randint(0, 1000, size=(n, n)) < p0] = 0
    if symmetric:
        idx = np.triu(idx, 1)
        idx = idx + idx.T
    m = grid[idx]
    m[np.arange(n), np.arange(n)] = F16(1)
    return m


def _scores(rs, n, c1, levels):
    return (rs.randint(1, levels, size=(n, c1)) * (LEVELS // levels)).astype(F32) / F32(LEVELS)


def _plant_ties(rs, cls, k, classes, plant):
    """Each class's column: fewer than K scores above a boundary level T, and more scores EQUAL to T than the places left.  With
    two keys per lane the cut - the last tied key that is in, the first that is out - falls between a lane's own two keys."""
    n = cls.shape[0]
    rk = keys_per_lane(n)
    for q, c in enumerate(classes):
        t_level = 24 - 3 * q
        n_above = k // (2 + q)
        need = k - n_above
        n_tie = need + max(3, k // 2)
        if rk == 2:
            lane = 64 * (2 + q) + 63                                      # the last lane of a wave: the run goes on in the next one
            lo, hi = 2 * lane, 2 * lane + 1
            tied = np.concatenate([rs.permutation(lo)[:need - 1], [lo, hi], hi + 1 + rs.permutation(n - hi - 1)[:n_tie - need - 1]])
        else:
            tied = rs.permutation(n)[:n_tie]
        rest = np.setdiff1d(np.arange(n), tied)
        above = rest[rs.permutation(len(rest))[:n_above]]
        col = rs.randint(1, t_level, size=n)
        col[tied] = t_level
        col[above] = rs.randint(t_level + 1, LEVELS, size=n_above)
        cls[:, c + 1] = col.astype(F32) / F32(LEVELS)
        plant.setdefault("tie_value", []).append(F32(t_level) / F32(LEVELS))


def _build_single(name, spec):
    rs = np.random.RandomState(spec["seed"])
    n, C, active = spec["n"], spec["C"], spec["active"]
    k = int(np.ceil(0.1 * n))
    plants, plant = spec["plants"], {}
    grid = value_grid([CLS_THR, IOU_THR, CON_THR])
    iou = _draw_map(rs, n, grid, spec["p0"][0], (), True)
    asy = _draw_map(rs, n, grid, spec["p0"][1], (), False)
    levels = spec.get("levels", LEVELS)
    cls, det = _scores(rs, n, C + 1, levels), _scores(rs, n, C + 1, levels)
    labels = np.zeros((1, C), F32)
    labels[0, active] = 1
    c0, c1 = active[0], active[1]
    con_lo, con_eq, con_hi = f16_steps(CON_THR)
    nms_lo, nms_eq, nms_hi = f16_steps(CLS_THR)
    if "fine_det" in plants:               # weights with 25 significant bits: the order of NumPy's pairwise sum shows in its result
        det = (rs.randint(1, 1 << 20, size=(n, C + 1)).astype(np.float64) / (1 << 20)).astype(F32)
    if "ties" in plants:
        _plant_ties(rs, cls, k, active, plant)
    if "last" in plants:
        cls[n - 1, c0 + 1] = 1.0                                          # the last proposal leads class c0's candidates
    tops = [topk(cls[:, c + 1], k) for c in active]
    free = np.setdiff1d(np.arange(n), np.concatenate(tops))               # in no class's top K: never a seed
    free = [int(i) for i in free[rs.permutation(len(free))]]
    take = lambda m: sorted(free.pop() for _ in range(m))
    if "huge3" in plants:
        # rows of the containment map with 0.9 N - 1, 0.9 N and 0.9 N + 1 entries above con_thr (the diagonal's 1 among them),
        # the rest AT the threshold or one step below
        rows = take(3)
        limit = int(round(0.9 * n))
        for r, cnt in zip(rows, (limit - 1, limit, limit + 1)):
            others = np.array([j for j in range(n) if j != r])
            asy[r, others] = np.where(np.arange(n - 1) % 2 == 0, con_eq, con_lo)
            asy[r, others[:cnt - 1]] = con_hi
        plant["huge_rows"], plant["huge_limit"] = rows, limit
    if "rows" in plants:
        # one row of the mask-IoU map per value v: v against every other proposal (so v against whichever columns end up as
        # pseudo ground truths), and a containment row that is empty off the diagonal: such a proposal is neither a seed (not in
        # any top K) nor anybody's arg-max, its COLUMN of the mask-IoU map is never read
        rows = take(len(ROW_VALUES))
        for r, v in zip(rows, ROW_VALUES):
            keep = iou[r, rows].copy()
            iou[r, :] = v
            iou[:, r] = v
            iou[r, rows] = iou[rows, r] = np.minimum(keep, v)            # (between two planted rows: no more than either's value)
            iou[r, r] = F16(1)
            asy[r, :] = F16(0)
            asy[r, r] = F16(1)
        plant["rows"] = rows
    if "nms3" in plants:
        # class c0's leading candidate (always kept) against the next three: AT nms_thr (suppressed), below (alive), above
        a, b, c, d = (int(x) for x in tops[0][:4])
        for j, v in ((b, nms_eq), (c, nms_lo), (d, nms_hi)):
            iou[a, j] = iou[j, a] = v
        plant["nms"] = (a, b, c, d)
    if "con3" in plants:
        # class c0's first seed s: three proposals with the column's largest detector score, contained AT con_thr, one step below
        # and one step above, in ascending order of index: only the last one may be taken (a `>=` would take the first)
        s = int(tops[0][0])
        i_lo, i_eq, i_hi = take(3)
        for i, v in ((i_lo, con_lo), (i_eq, con_eq), (i_hi, con_hi)):
            asy[i, s] = v
            det[i, c0 + 1] = 1.0
        plant["con"] = (s, i_lo, i_eq, i_hi)
    if "argmax" in plants:
        # equal (and largest) detector scores among the proposals that contain a class's first seed: at two indices that the
        # containment step gives to different lanes (8 consecutive proposals per lane), and at two that one lane holds
        s_a, s_b = int(tops[0][0]), int(tops[1][0])
        pool = sorted(free)
        i1 = pool[len(pool) // 3]
        i2 = next(i for i in pool if i // 8 > i1 // 8 + 8)
        same = next((a, b) for a, b in zip(pool, pool[1:]) if a // 8 == b // 8 and a not in (i1, i2) and b not in (i1, i2))
        for i in (i1, i2) + same:
            free.remove(i)
        for s, c, pair in ((s_a, c0, (i1, i2)), (s_b, c1, same)):
            for i in pair:
                asy[i, s] = con_hi
                det[i, c + 1] = 1.0
        plant["argmax"] = dict(cross=(s_a, i1, i2), same=(s_b,) + same)
    layer = dict(_SINGLE, cls=cls, det=det)
    return dict(name=name, N=n, C=C, K=k, labels=labels, iou=iou, asy=asy, layers=[layer], seed=spec.get("run_seed", spec["seed"] + 1000),
                layout=seed_layout(n, k), plant=plant, active=active)


def _build_layers(name, spec):
    rs = np.random.RandomState(spec["seed"])
    n, C, active = spec["n"], spec["C"], spec["active"]
    k = int(np.ceil(0.1 * n))
    thrs = sorted({t for pair in LAYER_THRESHOLDS for t in pair} | {CON_THR, HUGE_CON_THR})
    grid = value_grid(thrs)
    iou = _draw_map(rs, n, grid, spec["p0"][0], spec["thin"], True)
    asy = _draw_map(rs, n, grid, spec["p0"][1], spec["thin"], False)
    labels = np.zeros((1, C), F32)
    labels[0, active] = 1
    layers = []
    for li, (cls_thr, iou_thr) in enumerate(LAYER_THRESHOLDS):
        layer = dict(cls=_scores(rs, n, C + 1, LEVELS), det=_scores(rs, n, C + 1, LEVELS), cls_thr=cls_thr, iou_thr=iou_thr,
                     con_thr=CON_THR, sampling=True, using_cim=True)
        layer.update(LAYER_VARIANTS[name].get(li, {}))
        layers.append(layer)
    return dict(name=name, N=n, C=C, K=k, labels=labels, iou=iou, asy=asy, layers=layers, seed=spec["seed"] + 1000,
                layout=seed_layout(n, k), plant={}, active=active)


@functools.lru_cache(maxsize=None)
def mining_case(name):
    spec = CASES[name]
    case = _build_layers(name, spec) if name in LAYER_VARIANTS else _build_single(name, spec)
    for a in [case["iou"], case["asy"], case["labels"]] + [l[x] for l in case["layers"] for x in ("cls", "det")]:
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's run of a case: the layers one after the other on the global NumPy stream seeded with case["seed"] (what the
    reference's sequential CIM_layer calls do).  -> dict(outs = [(pseudo_labels, pseudo_iou, loss_weights) or Nones], traces,
    probe = the stream's next double afterwards, used = doubles drawn, meta = [(G, G')])."""
    from oracle import mining as om
    case = mining_case(name)
    np.random.seed(case["seed"])
    outs, traces, meta, used = [], [], [], 0
    for l in case["layers"]:
        trace = {}
        out = om.cim_layer_forward(l["cls"], l["det"], case["labels"], case["iou"], case["asy"], p_seed=0.1, cls_thr=l["cls_thr"],
                                   iou_thr=l["iou_thr"], con_thr=l["con_thr"], anti_noise_sampling=l["sampling"],
                                   using_cim=l["using_cim"], trace=trace)
        g = int(trace["gt_idxs"].sum())
        gk = int(trace["sample_keep"].sum()) if "sample_keep" in trace else g
        used += g if (l["sampling"] and g) else 0
        outs.append(out)
        traces.append(trace)
        meta.append((g, gk))
    probe = np.random.random_sample()
    return dict(outs=outs, traces=traces, probe=probe, used=used, meta=meta)


def expected(case, ref, li):
    """The oracle's trace of layer li in the shape of the kernel's per-layer outputs: topk / seeds / res [n_active, K] (-1
    tails), n_seeds, gt_class [N] (0 / class + 1), gt_weight [N]."""
    trace, k = ref["traces"][li], case["K"]
    n_act = len(case["active"])
    tk = np.stack(trace["keep_sort_idx"]).astype(np.int32)
    seeds = -np.ones((n_act, k), np.int32)
    res = -np.ones((n_act, k), np.int32)
    n_seeds = np.zeros(n_act, np.int32)
    for q in range(n_act):
        s = trace["keep_nms_idx"][q]
        n_seeds[q] = len(s)
        seeds[q, :len(s)] = s
        if "res_per_seed" in trace:
            res[q, :len(s)] = trace["res_per_seed"][q]
    gl = trace["gt_labels_full"]
    gt_class = np.where(trace["gt_idxs"], gl.argmax(1), 0).astype(np.int32)
    return dict(topk=tk, seeds=seeds, res=res, n_seeds=n_seeds, gt_class=gt_class, gt_weight=trace["gt_weights_full"])
