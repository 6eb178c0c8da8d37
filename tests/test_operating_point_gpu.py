"""The operating point on the device: `ggad_rank_operating_f32` (csrc/rank_metrics.hip), `metrics.operating_point` / `pr_curve`,
`ResidentSweep.operating_point`, config key `thres_select` and `run.py --threshold`.  Every native call runs on a workspace full of -1.

  1. every case of tests/rank_wide_ref.py, all five criteria (`precision` at 0.9 and 0.5, `fpr` at 0.01 and 0.0), against
     tests/operating_point_ref.py: the threshold's bits, the four counts, the number of candidates and the status are equal; out16[13] is
     within 1e-15 relative of the value recomputed from the counts in float64 (one division -- and for G-mean one square root -- of exact
     integers on both sides: at most a few ulp of 1.1e-16 apart); out16[0:8] holds the bits of `ggad_rank_wide_f32`'s out8; all P curve
     entries equal the reference expanded over tie runs and the entries beyond P keep their fill value;
  2. inputs whose labels depend on the scores (normal, quantised to 1/64, saturated sigmoids; P = 600, 8,192, 8,193, 16,385);
  3. the tie rule by hand, alone, under 8,191 more positives, and with the two tied candidates in different tiles of the sorted positives;
  4. one workspace reused across five_tiles -> p8193 -> tiny, twice: bit-equal to fresh workspaces;
  5. the status codes and the refused arguments;
  6. `metrics.operating_point` against `binary_report` at its threshold (the integers and what follows from them are equal; AUROC and AP
     come from the counting kernels here and from two float64 sorts there: 1e-12, the bound of tests/test_rank_wide_gpu.py), `pr_curve`
     against scikit-learn's `precision_recall_curve`, `ResidentSweep.operating_point`, and `scores()` plus the call as one replayed graph;
  7. `ModelHandler.train()` / `score()` with `thres_select` on and off;
  8. `run.py --threshold gmean --save F`, then `--score F`."""
import contextlib
import glob
import io
import json
import math
import os
import random
import re
import struct

import numpy as np
import pytest
import torch

from ggad_amd import synth
import operating_point_ref as OP
import rank_wide_ref as RW

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = [c[0] for c in RW.cases()]
FILL = -7.0


def _lib():
    from ggad_amd import _lib
    return _lib, _lib.load()


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


class Device:
    """The scores and labels of one input on the device, uploaded once; `call` is one `ggad_rank_operating_f32` call."""

    def __init__(self, s, y):
        self.n = len(s)
        self.s, self.y = torch.tensor(np.asarray(s)).to(DEV), torch.tensor(np.asarray(y)).to(DEV)

    def call(self, criterion, param, pos_cap, thres=0.5, ws=None, curve=False):
        """(out16 as a host array, (curve_thres, curve_tp, curve_fp) as host arrays or None)."""
        L, lib = _lib()
        need = int(lib.ggad_rank_operating_workspace_elems(self.n, pos_cap))
        assert need > 0
        if ws is None:
            ws = torch.full((need,), -1, dtype=torch.int32, device=DEV)            # (dirty on purpose)
        assert ws.numel() >= need
        out16 = torch.full((16,), FILL, dtype=torch.float64, device=DEV)
        cur = None
        if curve:
            cur = (torch.full((pos_cap,), FILL, dtype=torch.float32, device=DEV), torch.full((pos_cap,), -7, dtype=torch.int32, device=DEV),
                   torch.full((pos_cap,), -7, dtype=torch.int32, device=DEV))
        L.call("ggad_rank_operating_f32", L.ptr(self.s), L.ptr(self.y), self.n, pos_cap, float(thres), OP.CRITERIA.index(criterion),
               0.0 if param is None else float(param), L.ptr(out16), *((L.ptr(c) for c in cur) if cur else (0, 0, 0)), L.ptr(ws))
        return out16.cpu().numpy(), None if cur is None else tuple(c.cpu().numpy() for c in cur)

    def wide(self, pos_cap, thres):
        L, lib = _lib()
        ws = torch.full((int(lib.ggad_rank_wide_workspace_elems(self.n, pos_cap)),), -1, dtype=torch.int32, device=DEV)
        out8 = torch.full((8,), FILL, dtype=torch.float64, device=DEV)
        L.call("ggad_rank_wide_f32", L.ptr(self.s), L.ptr(self.y), self.n, pos_cap, float(thres), L.ptr(out8), L.ptr(ws))
        return out8.cpu().numpy()


def _check_point(o, want, criterion, param, P, Nn, tag):
    """out16[8..15] of one call against `OP.choose`."""
    print(f"[{tag}] {criterion}:{param} -> status {o[15]:.0f} thres {o[8]!r} tp {o[9]:.0f} fp {o[10]:.0f} value {o[13]!r} "
          f"(reference thres {float(want['thres'])!r} tp {want['tp']} fp {want['fp']} value {want['value']!r}) candidates {o[14]:.0f}")
    assert int(o[15]) == want["status"] and o[7] == 0.0, tag
    assert all(float(v).is_integer() for v in (*o[9:13], o[14], o[15]))
    assert tuple(int(v) for v in o[9:13]) == (want["tp"], want["fp"], want["fn"], want["tn"]), tag
    assert int(o[14]) == want["n_candidates"], tag
    if want["status"] == 5:
        assert o[8] == math.inf and o[13] == 0.0, tag
        return
    assert np.float64(np.float32(o[8])) == o[8]                                    # a float32, widened
    if want["thres"] == 0:                                                         # +-0.0 count as one score: either sign
        assert o[8] == 0.0, tag
    else:
        assert _bits(o[8]) == _bits(want["thres"]), tag
    recomputed = OP.value_from_counts(criterion, int(o[9]), int(o[10]), P, Nn)
    assert abs(o[13] - recomputed) <= 1e-15 * abs(recomputed), (tag, o[13], recomputed)
    if criterion == "f1_macro":
        assert o[13] == want["value"], tag                                         # one float64 formula on both sides


def _check_input(tag, s, y, thres=0.5, combos=OP.COMBOS):
    """Points 1's checks on one input at `pos_cap` = P; returns the number of combos that had no feasible candidate."""
    dev = Device(s, y)
    cached = OP.candidates(s, y)
    P, Nn = cached[3], cached[4]
    out8 = dev.wide(P, thres)
    infeasible = 0
    for k, (criterion, param) in enumerate(combos):
        o, cur = dev.call(criterion, param, P, thres, curve=k == 0)
        np.testing.assert_array_equal(o[:8].view(np.int64), out8.view(np.int64), err_msg=tag)
        want = OP.choose(s, y, criterion, param, cached)
        _check_point(o, want, criterion, param, P, Nn, tag)
        infeasible += want["status"] == 5
        if cur is not None:
            ct, ctp, cfp = OP.curve(s, y)
            assert len(ct) == P and np.array_equal(cur[1][:P], ctp) and np.array_equal(cur[2][:P], cfp), tag
            assert np.array_equal(np.where(cur[0][:P] == 0, np.float32(0), cur[0][:P]).view(np.int32), ct.view(np.int32)), tag
    return infeasible


# ------------------------------------------------------------------ 1: every case of the wide chain
@pytest.mark.parametrize("name", NAMES)
def test_every_case_every_criterion(name):
    _, s, y, thres = next(c for c in RW.cases() if c[0] == name)
    infeasible = _check_input(name, s, y, thres)
    if name in ("heavy_ties", "heavy_ties_wide"):
        assert infeasible >= 1                                                     # precision:0.9 cannot be met there: status 5, +inf


def test_curve_leaves_the_entries_beyond_p_alone():
    _, s, y, thres = next(c for c in RW.cases() if c[0] == "p8193")
    o, cur = Device(s, y).call("f1", None, 9000, thres, curve=True)
    assert o[15] == 0.0 and int(o[6]) == 8193
    assert (cur[0][8193:] == np.float32(FILL)).all() and (cur[1][8193:] == -7).all() and (cur[2][8193:] == -7).all()
    ct, ctp, cfp = OP.curve(s, y)
    assert np.array_equal(cur[0][:8193].view(np.int32), ct.view(np.int32)) and np.array_equal(cur[1][:8193], ctp)
    assert np.array_equal(cur[2][:8193], cfp)


# ------------------------------------------------------------------ 2: labels that depend on the scores
SEPARABLE = OP.separable_cases()


@pytest.mark.parametrize("name", [c[0] for c in SEPARABLE])
def test_separable_inputs(name):
    _, s, y = next(c for c in SEPARABLE if c[0] == name)
    if "sat" in name:
        assert int(((s == 1.0) & (y == 1)).sum()) >= (1000 if "16385" in name else 50)     # exact ties at the top of the ranking
    _check_input(name, s, y)
    best = OP.choose(s, y, "f1")
    assert 0 < best["fp"] and 0 < best["fn"]                                        # an interior maximum, not an end of the curve


# ------------------------------------------------------------------ 3: the tie rule
def test_tie_rule_by_hand():
    s, y = OP.tie_by_hand()
    o, _ = Device(s, y).call("f1", None, 3)
    assert (np.float32(o[8]), int(o[9]), int(o[10]), o[13], int(o[14]), o[15]) == (np.float32(0.9), 1, 0, 0.5, 3, 0.0)
    s, y = OP.tie_by_hand_padded()
    o, _ = Device(s, y).call("f1", None, 8194)
    assert (np.float32(o[8]), int(o[9]), int(o[10]), o[13], int(o[14]), o[15]) == (np.float32(0.9), 8192, 16382, 0.5, 8194, 0.0)
    _check_input("tie_by_hand_padded", s, y)
    s, y = OP.tie_across_sorted_tiles()
    o, _ = Device(s, y).call("gmean", None, 8193)
    assert (np.float32(o[8]), int(o[9]), int(o[10]), int(o[14]), o[15]) == (np.float32(0.9), 1, 0, 8193, 0.0)
    _check_input("tie_across_sorted_tiles", s, y)


# ------------------------------------------------------------------ 4: a reused workspace
def test_one_workspace_reused_shows_nothing_stale():
    _, lib = _lib()
    order = ("five_tiles", "p8193", "tiny")
    inputs = {name: next(c for c in RW.cases() if c[0] == name) for name in order}
    devs = {name: Device(c[1], c[2]) for name, c in inputs.items()}
    caps = {name: int(c[2].sum()) for name, c in inputs.items()}
    need = max(int(lib.ggad_rank_operating_workspace_elems(devs[n].n, caps[n])) for n in order)
    shared = torch.full((need,), -1, dtype=torch.int32, device=DEV)
    for _ in range(2):
        for name in order:
            for criterion, param in (("f1_macro", None), ("fpr", 0.01)):
                fresh, cf = devs[name].call(criterion, param, caps[name], inputs[name][3], curve=True)
                again, ca = devs[name].call(criterion, param, caps[name], inputs[name][3], ws=shared, curve=True)
                np.testing.assert_array_equal(again.view(np.int64), fresh.view(np.int64), err_msg=name)
                for a, b in zip(ca, cf):
                    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32), err_msg=name)
                assert fresh[7] == 0.0


# ------------------------------------------------------------------ 5: status
def test_status_codes_and_refused_arguments():
    L, lib = _lib()
    _, s, y, thres = next(c for c in RW.cases() if c[0] == "p8193")

    def refused(o, dev, pos_cap, status):
        assert o[15] == o[7] == float(status) and np.isnan(o[8:15]).all()
        np.testing.assert_array_equal(o[:8].view(np.int64), dev.wide(pos_cap, thres).view(np.int64))
    bad = s.copy()
    bad[333] = np.nan
    d = Device(bad, y)
    refused(d.call("f1", None, 8193, thres)[0], d, 8193, 3)
    y2 = y.copy()
    y2[77] = 2
    d = Device(s, y2)
    refused(d.call("gmean", None, 8193, thres)[0], d, 8193, 4)
    for const in (0, 1):
        d = Device(s, np.full(len(s), const, dtype=np.uint8))
        refused(d.call("f1_macro", None, len(s), thres)[0], d, len(s), 1)
    d = Device(s, y)
    o, cur = d.call("fpr", 0.5, 8192, thres, curve=True)                            # P = pos_cap + 1
    refused(o, d, 8192, 2)
    assert int(o[6]) == 8193 and (cur[1] == -7).all() and (cur[2] == -7).all()      # ... and nothing of the curve was written
    # refused without a launch: nothing is touched
    out16 = torch.full((16,), FILL, dtype=torch.float64, device=DEV)
    ws = torch.full((int(lib.ggad_rank_operating_workspace_elems(len(s), 8193)) + 4,), -1, dtype=torch.int32, device=DEV)
    c = [torch.full((8193,), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
    f = lib.ggad_rank_operating_f32
    p = L.ptr
    assert p(ws) % 16 == 0
    for crit, param, curve, w in ((5, 0.0, (0, 0, 0), p(ws)), (-1, 0.0, (0, 0, 0), p(ws)), (3, 1.5, (0, 0, 0), p(ws)),
                                  (4, -0.01, (0, 0, 0), p(ws)), (3, float("nan"), (0, 0, 0), p(ws)),
                                  (0, 0.0, (p(c[0]), 0, 0), p(ws)), (0, 0.0, (p(c[0]), p(c[1]), 0), p(ws)),
                                  (0, 0.0, (0, p(c[1]), p(c[2])), p(ws)), (0, 0.0, (0, 0, 0), p(ws) + 4)):
        assert f(p(d.s), p(d.y), len(s), 8193, 0.5, crit, param, p(out16), *curve, w, None) == -1, (crit, param, curve)
    for pos_cap in (0, int(lib.ggad_rank_wide_max_pos()) + 1):
        assert f(p(d.s), p(d.y), len(s), pos_cap, 0.5, 0, 0.0, p(out16), 0, 0, 0, p(ws), None) == -1
    torch.cuda.synchronize()
    assert (out16.cpu().numpy() == FILL).all() and bool((ws == -1).all()) and all(bool((t == -7).all()) for t in c)
    # criteria 0..2 ignore param
    a = d.call("f1", None, 8193, thres)[0]
    out = torch.full((16,), FILL, dtype=torch.float64, device=DEV)
    w2 = torch.full_like(ws, -1)
    assert f(p(d.s), p(d.y), len(s), 8193, float(thres), 0, 123.0, p(out), 0, 0, 0, p(w2), None) == 0
    np.testing.assert_array_equal(out.cpu().numpy().view(np.int64), a.view(np.int64))


# ------------------------------------------------------------------ 6: the public calls
@pytest.mark.parametrize("name", ["sep_p8193", "sep_sat_p16385", "sep_q64_p600"])
def test_operating_point_against_binary_report(name):
    from ggad_amd.metrics import OperatingPoint, binary_report, operating_point
    _, s, y = next(c for c in SEPARABLE if c[0] == name)
    d = Device(s, y)
    cached = OP.candidates(s, y)
    for criterion, param in OP.COMBOS:
        for pos_cap in (None, cached[3]):
            op = operating_point(d.s, d.y, criterion, param, pos_cap=pos_cap)
            want = OP.choose(s, y, criterion, param, cached)
            assert isinstance(op, OperatingPoint) and type(op.thres) is float and op.feasible == (want["status"] == 0)
            assert (op.tp, op.fp, op.fn, op.tn, op.n_candidates) == (want["tp"], want["fp"], want["fn"], want["tn"], want["n_candidates"])
            assert op.thres == float(want["thres"]) and (op.criterion, op.param) == (criterion, param)
            b = binary_report(d.s, d.y, op.thres)
            assert list(op.report) == list(b)
            for k in ("tp", "fp", "fn", "tn", "f1_1", "f1_0", "f1_macro", "gmean"):
                assert op.report[k] == b[k] and type(op.report[k]) is type(b[k]), (criterion, k)
            assert abs(op.report["auc"] - b["auc"]) <= 1e-12 and abs(op.report["ap"] - b["ap"]) <= 1e-12
            if criterion in ("f1_macro", "gmean") and op.feasible:
                assert op.value == op.report[criterion]


def test_operating_point_refuses():
    from ggad_amd.metrics import operating_point
    _, s, y, _ = next(c for c in RW.cases() if c[0] == "p8193")
    d = Device(s, y)
    bad = s.copy()
    bad[5] = np.nan
    y2 = y.copy()
    y2[5] = 3
    for args, text in (((torch.tensor(bad).to(DEV), d.y), "NaN"), ((d.s, torch.tensor(y2).to(DEV)), "neither 0 nor 1"),
                       ((d.s, torch.zeros_like(d.y)), "Only one class"), ((d.s, torch.ones_like(d.y)), "Only one class")):
        with pytest.raises(ValueError, match=text):
            operating_point(*args, "f1")
    with pytest.raises(ValueError, match="pos_cap = 8192"):                         # no silent fallback: the cap is named
        operating_point(d.s, d.y, "f1", pos_cap=8192)
    with pytest.raises(ValueError, match="pos_cap"):
        operating_point(d.s, d.y, "f1", pos_cap=0)
    with pytest.raises(ValueError, match="unknown criterion"):
        operating_point(d.s, d.y, "accuracy")
    for param in (None, -0.5, 1.01):
        with pytest.raises(ValueError, match="param"):
            operating_point(d.s, d.y, "precision", param)


def test_pr_curve_against_sklearn():
    from sklearn.metrics import precision_recall_curve
    from ggad_amd.metrics import pr_curve
    _, s, y, _ = next(c for c in RW.cases() if c[0] == "p8193")
    d = Device(s, y)
    for pos_cap in (None, 8193):
        thres, tp, fp = (t.cpu().numpy() for t in pr_curve(d.s, d.y, pos_cap=pos_cap))
        cand, ctp, cfp, P, _ = OP.candidates(s, y)
        assert thres.dtype == np.float32 and np.array_equal(thres, cand[::-1]) and np.array_equal(tp, ctp[::-1]) and np.array_equal(fp, cfp[::-1])
        prec, rec, sk_thres = precision_recall_curve(y, s)
        at = np.searchsorted(sk_thres, thres)
        assert np.array_equal(sk_thres[at].astype(np.float32), thres)
        assert np.array_equal(prec[at], tp / (tp + fp).astype(np.float64)) and np.array_equal(rec[at], tp / np.float64(P))
    _, s, y = next(c for c in SEPARABLE if c[0] == "sep_sat_p16385")               # tie runs are folded: one entry per distinct score
    d = Device(s, y)
    thres, tp, fp = (t.cpu().numpy() for t in pr_curve(d.s, d.y))
    cand, ctp, cfp, _, _ = OP.candidates(s, y)
    assert len(cand) < 16385 and np.array_equal(thres, cand[::-1]) and np.array_equal(tp, ctp[::-1]) and np.array_equal(fp, cfp[::-1])


N_NODES = 3000


@pytest.fixture(scope="module")
def small_graph():
    rowptr, col = synth.make_graph(N_NODES, 30000, 3, kind="powerlaw", max_degree=200)
    rng = np.random.default_rng(8)
    cases = rng.integers(0, N_NODES, 12000).astype(np.int64)
    lab = np.zeros(len(cases), dtype=np.int64)
    lab[rng.choice(len(cases), 9000, replace=False)] = 1                           # two tiles of positives
    return rowptr, col, cases, lab


def _model(small_graph, f, d, seed=0):
    from ggad_amd.dgraph import normalize_features
    from ggad_amd.graph import DeviceGraph
    from ggad_amd.graphsage import GCN, FeatureTable, GCNAggregator, GCNEncoder
    rowptr, col = small_graph[:2]
    torch.manual_seed(seed)
    graph = DeviceGraph(rowptr, col, DEV)
    feat = normalize_features(synth.make_features(N_NODES, f, 3)).astype(np.float32)
    features = FeatureTable(torch.from_numpy(feat))
    enc = GCNEncoder(features, f, d, graph, GCNAggregator(features, cuda=True), gcn=True, cuda=True)
    model = GCN(2, enc)
    enc.engine.sync_params()
    return model


def _perturb(eng, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        eng.params[:eng.n_train] += 0.05 * torch.randn(eng.n_train, generator=g).to(eng.params.device)
    eng.sync_params()


def test_resident_sweep_operating_point_and_replay(small_graph):
    from ggad_amd import metrics
    from ggad_amd.eval_cache import ResidentSweep
    L, lib = _lib()
    _, _, cases, lab = small_graph
    model = _model(small_graph, 17, 64)
    eng = model.enc.engine
    _perturb(eng, 2)
    sweep = ResidentSweep(model, cases, lab, 150)
    scores = sweep.scores()
    for criterion, param in (("f1_macro", None), ("fpr", 0.05)):
        op = sweep.operating_point(criterion, param)
        assert sweep.n_pos == 9000
        assert op == metrics.operating_point(scores, sweep.labels, criterion, param, pos_cap=9000)
        assert op == sweep.operating_point(criterion, param, scores=scores)
        want = OP.choose(scores.cpu().numpy(), lab, criterion, param)
        assert (op.thres, op.tp, op.fp, op.feasible) == (float(want["thres"]), want["tp"], want["fp"], want["status"] == 0)
        b = metrics.binary_report(scores, sweep.labels, op.thres)
        assert {k: v for k, v in b.items() if k not in ("auc", "ap")} == {k: v for k, v in op.report.items() if k not in ("auc", "ap")}
    with pytest.raises(ValueError, match="without labels"):
        ResidentSweep(model, cases, None, 150).operating_point("f1")
    # scores() plus the call as one graph, replayed after the weights changed
    pos_cap = 9000
    ws = torch.empty(int(lib.ggad_rank_operating_workspace_elems(sweep.n, pos_cap)), dtype=torch.int32, device=DEV)
    out16 = torch.zeros(16, dtype=torch.float64, device=DEV)

    def eager():
        o = torch.zeros(16, dtype=torch.float64, device=DEV)
        w = torch.full_like(ws, -1)
        L.call("ggad_rank_operating_f32", L.ptr(sweep.scores()), L.ptr(sweep.labels), sweep.n, pos_cap, 0.5, 1, 0.0, L.ptr(o), 0, 0, 0, L.ptr(w))
        return o.cpu().numpy()
    first = eager()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        probs = sweep.scores()
        L.call("ggad_rank_operating_f32", L.ptr(probs), L.ptr(sweep.labels), sweep.n, pos_cap, 0.5, 1, 0.0, L.ptr(out16), 0, 0, 0, L.ptr(ws))
    graph.replay()
    np.testing.assert_array_equal(out16.cpu().numpy().view(np.int64), first.view(np.int64))
    assert first[15] == 0.0 and first[6] == 9000.0
    seen = [first]
    for seed in (3, 4):
        _perturb(eng, seed)
        graph.replay()
        got = out16.cpu().numpy()
        np.testing.assert_array_equal(got.view(np.int64), eager().view(np.int64))
        assert not any(np.array_equal(got, s) for s in seen)                       # the replay saw the new weights
        seen.append(got)


# ------------------------------------------------------------------ 7: the handler
def test_model_handler_with_thres_select_on_and_off(tmp_path, capsys):
    from ggad_amd import metrics
    from ggad_amd.model_handler import ModelHandler
    n = 30000
    rowptr, col = synth.make_graph(n, 300000, 3, kind="powerlaw", max_degree=200)
    feat = synth.make_features(n, 17, 3)
    lab = synth.make_labels(n, 0.05, 3)
    rowptr, col, feat = synth.plant_anomalies(rowptr, col, feat, lab, 3, scale=0.25, rewire=0.5)
    runs = {}
    for tag, key, cache in (("off", "", True), ("on", "f1_macro", True), ("on_plain", "f1_macro", False)):
        cfg = dict(data_name="synthetic", data_dir="", data=((rowptr, col), feat, lab), seed=72, model="GCN", multi_relation="GNN",
                   emb_size=64, thres=0.4, lr=0.005, weight_decay=0.007, batch_size=60, num_epochs=2, valid_epochs=1, num_batches=6,
                   n_pseudo=20, save_dir=str(tmp_path / tag) + "/", test_ratio=0.67, device=0, eval_cache=cache)
        if key:
            cfg["thres_select"] = key
        random.seed(72)
        np.random.seed(72)
        torch.manual_seed(72)
        capsys.readouterr()
        h = ModelHandler(cfg)
        res = h.train()
        out = capsys.readouterr().out
        ckpts = glob.glob(str(tmp_path / tag / "*" / "*.pkl"))                     # save_dir + timestamp / <data>_<model>.pkl
        assert len(ckpts) == 1
        runs[tag] = dict(h=h, cfg=cfg, res=res, out=out, ckpt=ckpts[0], losses=np.stack(h.epoch_losses), end=h.end_state, hist=h.valid_history,
                         lines=[ln for ln in out.splitlines() if ln.startswith("   GNN ")])
    off, on, plain = runs["off"], runs["on"], runs["on_plain"]
    assert "[threshold]" not in off["out"] and off["h"].operating_point is None
    assert not os.path.exists(ModelHandler.thres_path(off["ckpt"])) and glob.glob(str(tmp_path / "off" / "*" / "*.json")) == []
    for r in (on, plain):
        np.testing.assert_array_equal(off["losses"].view(np.int64), r["losses"].view(np.int64))
        assert list(off["end"]) == list(r["end"]) and all(torch.equal(off["end"][k], r["end"][k]) for k in off["end"])
        assert len(r["lines"]) == 6 and r["out"].count("[threshold]") == 1            # two lines a sweep: two validations, the closing one
    assert off["hist"] == on["hist"] and off["lines"][:4] == on["lines"][:4]       # the validation sweeps are untouched
    h = on["h"]
    op = h.operating_point
    sweep = h.eval_sweeps[1]
    scores = sweep.scores()
    want = OP.choose(scores.cpu().numpy(), np.asarray(h.dataset["y_test"]), "f1_macro")
    assert (op.thres, op.tp, op.fp, op.fn, op.tn) == (float(want["thres"]), want["tp"], want["fp"], want["fn"], want["tn"])
    assert (plain["h"].operating_point.thres, plain["h"].operating_point.tp) == (op.thres, op.tp)       # the same scores either way
    b = metrics.binary_report(scores, sweep.labels, op.thres)
    assert on["lines"][5] == f"   GNN TP: {b['tp']}\tTN: {b['tn']}\tFN: {b['fn']}\tFP: {b['fp']}" == plain["lines"][5]
    assert (b["tp"], b["fp"], b["fn"], b["tn"]) == (op.tp, op.fp, op.fn, op.tn)
    assert (on["res"][0], on["res"][1], on["res"][2], on["res"][4]) == (b["f1_macro"], b["f1_1"], b["f1_0"], b["gmean"])
    assert on["res"][0] == op.value                                                # the closing report's macro-F1 is the chosen maximum
    line = next(ln for ln in on["out"].splitlines() if ln.startswith("[threshold]"))
    assert line.startswith(f"[threshold] f1_macro: threshold {op.thres!r}\tvalue {op.value!r}\tTP: {op.tp}\tFP: {op.fp}")
    # the side file: settings only, next to a plain state dict; score() reads it
    with open(ModelHandler.thres_path(on["ckpt"])) as fh:
        doc = json.load(fh)
    assert doc == {"criterion": "f1_macro", "param": None, "thres": op.thres, "thres_bits": _bits(op.thres), "value": op.value,
                   "tp": op.tp, "fp": op.fp, "fn": op.fn, "tn": op.tn, "epoch": doc["epoch"]} and doc["epoch"] in (0, 1)
    state = torch.load(on["ckpt"])
    assert all(isinstance(v, torch.Tensor) for v in state.values()) and list(state) == list(torch.load(off["ckpt"]))
    capsys.readouterr()
    h2 = ModelHandler(on["cfg"])
    got_scores, _ = h2.score(on["ckpt"])
    out2 = capsys.readouterr().out
    assert torch.equal(got_scores, scores) and h2.metrics == on["res"] and h2.thres_doc == doc
    assert [ln for ln in out2.splitlines() if ln.startswith("   GNN ")] == on["lines"][4:]
    h3 = ModelHandler(on["cfg"])
    with pytest.raises(ValueError, match=re.escape(ModelHandler.thres_path(off["ckpt"]))):
        h3.score(off["ckpt"])
    h4 = ModelHandler(off["cfg"])                                                  # key off: score() is today's, at thres
    h4.score(on["ckpt"])
    assert h4.metrics == off["res"]


# ------------------------------------------------------------------ 8: run.py
def test_run_py_threshold_save_and_score(tmp_path, capsys):
    import run
    from ggad_amd.metrics import _confusion_scores
    ckpt, plain = str(tmp_path / "w.pt"), str(tmp_path / "plain.pt")
    base = ["--synthetic", "--dataset", "reddit", "--quiet"]
    capsys.readouterr()
    assert run.main(base + ["--num_epoch", "4", "--select", "auroc", "--threshold", "gmean", "--save", ckpt]) is None
    out_train = capsys.readouterr().out
    scores = run.main(base + ["--score", ckpt])
    out_score = capsys.readouterr().out
    args = run.parse(base)
    random.seed(args.seed), np.random.seed(args.seed), torch.manual_seed(args.seed)      # what init_process seeds before the loader runs
    with contextlib.redirect_stdout(io.StringIO()):
        g = run.load_graph(args)
    y = np.asarray(g.ano_label).reshape(-1)
    idx_val, idx_test = np.asarray(g.idx_val, dtype=np.int64), np.asarray(g.idx_test, dtype=np.int64)
    want = OP.choose(scores[idx_val], y[idx_val], "gmean")
    meta = torch.load(ckpt, map_location="cpu", weights_only=True)["meta"]
    assert set(meta) == {"dataset", "n_in", "embedding_dim", "nodes", "seed", "epoch", "select", "value", "thres", "thres_select", "thres_value"}
    assert meta["thres"] == float(want["thres"]) and meta["thres_select"] == "gmean"
    assert abs(meta["thres_value"] - want["value"]) <= 1e-15 * want["value"]       # one division and one square root of exact integers
    pred = scores[idx_test] >= np.float32(meta["thres"])
    yt = y[idx_test] == 1
    c = _confusion_scores(int((pred & yt).sum()), int((pred & ~yt).sum()), int((~pred & yt).sum()), int((~pred & ~yt).sum()))
    test_line = "[threshold] test at {!r}: tp {} fp {} fn {} tn {} F1-macro {!r} G-mean {!r}".format(
        meta["thres"], c["tp"], c["fp"], c["fn"], c["tn"], c["f1_macro"], c["gmean"])
    lines_train = [ln for ln in out_train.splitlines() if ln.startswith("[threshold]")]
    assert len(lines_train) == 2 and lines_train[1] == test_line
    assert lines_train[0].startswith("[threshold] gmean on {} validation nodes: threshold {!r} value {!r} tp {} fp {} fn {} tn {} ".format(
        idx_val.size, meta["thres"], meta["thres_value"], want["tp"], want["fp"], want["fn"], want["tn"]))
    lines_score = [ln for ln in out_score.splitlines() if ln.startswith(("[threshold]", "alerts:"))]
    assert lines_score == [test_line, "alerts: {} of {} test nodes".format(c["tp"] + c["fp"], idx_test.size)]
    # without the option: the saved dict and the prints are those of before
    assert run.main(base + ["--num_epoch", "2", "--save", plain]) is None
    out_plain = capsys.readouterr().out
    assert set(torch.load(plain, map_location="cpu", weights_only=True)["meta"]) == {"dataset", "n_in", "embedding_dim", "nodes", "seed", "epoch",
                                                                                   "select", "value"}
    run.main(base + ["--score", plain])
    assert "[threshold]" not in out_plain and "[threshold]" not in capsys.readouterr().out
