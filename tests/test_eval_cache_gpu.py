"""Config key `eval_cache`: the resident validation sweep (ggad_amd/eval_cache.py) and the rank metrics in HIP
(csrc/rank_metrics.hip, `metrics.rank_report`).

  1-3. `ResidentSweep.scores()` is `torch.equal` to `score_nodes(..., device=True)` at (F, D) = (17, 64), (9, 24) and (17, 128: the
       wide path), for 1,000 ids in slices of 150 (a short last slice, one id in two slices, the hub row among them), with the cache
       stitched from one chunk and from many (`batches_per_launch=2`), and again after the weights changed -- with no plan built
       in between;
  4.   `rank_report` against tests/rank_metrics_ref.py (exact counts), `math.fsum` and scikit-learn on the smallest inputs at which
       each branch can go wrong.  Bounds: the confusion counts and n_pos are integers; AUROC is ONE float64 division of exact
       integers, so it equals the float of the exact fraction; AP is a float64 sum of at most 8,192 terms in (0, 1], whose error is
       far below 1e-12 (8,192 x 2^-53 = 9e-13 is the crude bound of ANY summation order; tree sums stay near 1e-16);
  5.   `test_sage(..., resident=sweep)` against `test_sage(...)`;
  6.   `scores()` plus the native metrics call captured in one graph and replayed after the weights changed;
  7.   `ModelHandler.train()` with the key on against off."""
import math
import random
import re

import numpy as np
import pytest
import torch
from sklearn.metrics import average_precision_score, roc_auc_score

from ggad_amd import synth
import rank_metrics_ref as RM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_NODES = 3000


@pytest.fixture(scope="module")
def small_graph():
    rowptr, col = synth.make_graph(N_NODES, 30000, 3, kind="powerlaw", max_degree=200)
    deg = np.diff(rowptr)
    hub = int(np.argmax(deg))
    assert deg[hub] >= 100                                        # a hub row
    cases = np.random.default_rng(5).choice(N_NODES, 1000, replace=False).astype(np.int64)
    if hub not in cases:
        cases[3] = hub
    cases[500] = cases[10]                                         # one id in two slices (0 and 3)
    lab = (np.random.default_rng(6).random(len(cases)) < 0.1).astype(np.int64)
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


# ------------------------------------------------------------------ 1-3: the scores
@pytest.mark.parametrize("f,d", [(17, 64), (9, 24), (17, 128)])
def test_resident_scores_equal_the_sweep_bit_for_bit(small_graph, f, d, monkeypatch):
    from ggad_amd.eval_cache import ResidentSweep
    from ggad_amd.minibatch import BatchChunk
    from ggad_amd.sage_utils import score_nodes
    _, _, cases, lab = small_graph
    model = _model(small_graph, f, d)
    eng = model.enc.engine
    assert eng.wide == (d > 64)
    one = ResidentSweep(model, cases, lab, 150)
    many = ResidentSweep(model, cases, lab, 150, batches_per_launch=2)           # 7 slices: the cache stitched from four chunks
    assert (one.builds, many.builds) == (1, 4)
    want = score_nodes(model, cases, 150, device=True)
    assert want.dtype == torch.float32 and want.shape == (1000,) and want.is_cuda
    assert 0.0 < float(want.min()) and float(want.max()) < 1.0 and float(want.std()) > 0.0
    assert torch.equal(one.scores(), want)
    assert torch.equal(many.scores(), want)
    assert torch.equal(one.x1, many.x1)
    # other weights, no plan built in between
    _perturb(eng, 1)
    calls = []
    real = BatchChunk.build
    monkeypatch.setattr(BatchChunk, "build", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    got_one, got_many = one.scores(), many.scores()
    assert calls == []
    want2 = score_nodes(model, cases, 150, device=True)
    assert len(calls) == 1                                        # (the uncached sweep plans again)
    assert not torch.equal(want2, want)
    assert torch.equal(got_one, want2) and torch.equal(got_many, want2)
    # invalidate: the rows are rebuilt by the next sweep, and equal
    one.invalidate()
    assert torch.equal(one.scores(), want2) and len(calls) == 2


def test_empty_sweep(small_graph):
    from ggad_amd.eval_cache import ResidentSweep
    model = _model(small_graph, 17, 64)
    sweep = ResidentSweep(model, [], [], 150)
    out = sweep.scores()
    assert out.shape == (0,) and out.dtype == torch.float32 and sweep.builds == 0


# ------------------------------------------------------------------ 4: the metrics
def _native(s, y, thres):
    from ggad_amd import _lib
    lib = _lib.load()
    sd, yd = torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV)
    ws = torch.full((int(lib.ggad_rank_metrics_workspace_elems(len(s))),), -1, dtype=torch.int32, device=DEV)      # (dirty on purpose)
    out8 = torch.full((8,), -7.0, dtype=torch.float64, device=DEV)
    _lib.call("ggad_rank_metrics_f32", _lib.ptr(sd), _lib.ptr(yd), len(s), float(thres), _lib.ptr(out8), _lib.ptr(ws))
    return out8.cpu().numpy()


def _cap():
    from ggad_amd import _lib
    return int(_lib.load().ggad_rank_metrics_max_pos())


def test_cap_is_exported():
    assert _cap() >= 8192


@pytest.mark.parametrize("case", RM.cases(8192), ids=lambda c: c[0])
def test_rank_report_against_exact_counts_and_sklearn(case):
    from ggad_amd.metrics import binary_report, rank_report
    name, s, y, thres = case
    if name == "at_cap":
        assert int(y.sum()) == _cap()
    o = _native(s, y, thres)
    auroc_exact = float(RM.auroc_fraction(s, y))
    ap_fsum = RM.average_precision(s, y)
    sk = RM.finite_image(s)
    print(f"\n[{name}] n {len(s)} P {int(y.sum())}: auroc {o[0]!r} (exact {auroc_exact!r}), ap - fsum {o[1] - ap_fsum:.3g}, "
          f"auroc - sklearn {o[0] - roc_auc_score(y, sk):.3g}, ap - sklearn {o[1] - average_precision_score(y, sk):.3g}")
    assert o[7] == 0.0
    assert tuple(int(v) for v in o[2:6]) == RM.confusion(s, y, thres) and all(float(v).is_integer() for v in o[2:7])
    assert int(o[6]) == int(y.sum())
    assert o[0] == auroc_exact
    assert abs(o[1] - ap_fsum) <= 1e-12
    assert abs(o[0] - roc_auc_score(y, sk)) <= 1e-12 and abs(o[1] - average_precision_score(y, sk)) <= 1e-12
    # the public call: the same numbers under the keys of binary_report
    r = rank_report(torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV), thres)
    b = binary_report(torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV), thres)
    assert list(r) == list(b)
    assert (r["auc"], r["ap"]) == (o[0], o[1])
    for k in ("tp", "fp", "fn", "tn", "f1_1", "f1_0", "f1_macro", "gmean"):
        assert r[k] == b[k] and type(r[k]) is type(b[k]), k
    assert abs(r["auc"] - b["auc"]) <= 1e-12 and abs(r["ap"] - b["ap"]) <= 1e-12


def test_rank_report_above_the_cap_falls_back(monkeypatch):
    from ggad_amd import metrics
    cap = _cap()
    rng = np.random.default_rng(3)
    n = cap + 1 + 2000
    y = np.zeros(n, dtype=np.uint8)
    y[rng.choice(n, cap + 1, replace=False)] = 1
    s = rng.random(n).astype(np.float32)
    o = _native(s, y, 0.5)
    assert o[7] == 2.0 and int(o[6]) == cap + 1 and tuple(int(v) for v in o[2:6]) == RM.confusion(s, y, 0.5)
    sd, yd = torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV)
    want = metrics.binary_report(sd, yd, 0.5)
    calls = []
    real = metrics.binary_report
    monkeypatch.setattr(metrics, "binary_report", lambda *a: (calls.append(1), real(*a))[1])
    got = metrics.rank_report(sd, yd, 0.5)
    assert calls == [1] and got == want


def test_rank_report_refuses_nan_bad_labels_and_one_class():
    from ggad_amd.metrics import binary_report, rank_report
    rng = np.random.default_rng(4)
    s = rng.random(700).astype(np.float32)
    y = (rng.random(700) < 0.3).astype(np.uint8)
    dev = lambda a: torch.from_numpy(a).to(DEV)                    # noqa: E731
    bad = s.copy()
    bad[333] = np.nan
    assert _native(bad, y, 0.5)[7] == 3.0
    with pytest.raises(ValueError, match="NaN"):
        rank_report(dev(bad), dev(y), 0.5)
    y2 = y.copy()
    y2[77] = 2
    assert _native(s, y2, 0.5)[7] == 4.0
    with pytest.raises(ValueError, match="neither 0 nor 1"):
        rank_report(dev(s), dev(y2), 0.5)
    for const in (0, 1):
        y1 = np.full(700, const, dtype=np.uint8)
        o = _native(s, y1, 0.5)
        assert o[7] == 1.0 and int(o[6]) == 700 * const and math.isnan(o[0]) and o[1] == float(const)
        assert tuple(int(v) for v in o[2:6]) == RM.confusion(s, y1, 0.5)
        with pytest.raises(ValueError) as want:
            binary_report(dev(s), dev(y1), 0.5)
        with pytest.raises(ValueError) as got:
            rank_report(dev(s), dev(y1), 0.5)
        assert str(got.value) == str(want.value)


# ------------------------------------------------------------------ 5: test_sage
def test_test_sage_with_a_resident_sweep(small_graph, capsys):
    from ggad_amd.eval_cache import ResidentSweep
    from ggad_amd.sage_utils import test_sage as run_sweep
    _, _, cases, lab = small_graph
    model = _model(small_graph, 17, 64)
    _perturb(model.enc.engine, 2)
    sweep = ResidentSweep(model, cases, lab, 150)
    capsys.readouterr()
    a = run_sweep(cases, lab, model, 150, 0.5)
    ap_a, out_a = run_sweep.last_ap, capsys.readouterr().out.splitlines()
    b = run_sweep(cases, lab, model, 150, 0.5, resident=sweep)
    ap_b, out_b = run_sweep.last_ap, capsys.readouterr().out.splitlines()
    assert len(a) == len(b) == 5 and len(out_a) == len(out_b) == 3
    # the printed lines: F1 / G-mean / AUC (4 decimals) and the confusion integers as they are; the AP line prints a float64 in full,
    # which the two paths compute in different summation orders -- its number is compared like `last_ap`
    assert out_a[0] == out_b[0] and out_a[2] == out_b[2]
    assert re.fullmatch(r"   GNN TP: \d+\tTN: \d+\tFN: \d+\tFP: \d+", out_b[2])
    assert out_a[1].startswith("Testing AP: ") and out_b[1].startswith("Testing AP: ")
    assert abs(float(out_a[1].split(": ")[1]) - float(out_b[1].split(": ")[1])) <= 1e-12
    f1_mac_a, f1_1_a, f1_0_a, auc_a, gm_a = a
    f1_mac_b, f1_1_b, f1_0_b, auc_b, gm_b = b
    assert (f1_mac_a, f1_1_a, f1_0_a, gm_a) == (f1_mac_b, f1_1_b, f1_0_b, gm_b)
    assert abs(auc_a - auc_b) <= 1e-12 and abs(ap_a - ap_b) <= 1e-12


# ------------------------------------------------------------------ 6: capture
def test_scores_and_metrics_replay_as_one_graph(small_graph):
    from ggad_amd import _lib
    from ggad_amd.eval_cache import ResidentSweep
    _, _, cases, lab = small_graph
    model = _model(small_graph, 17, 64)
    eng = model.enc.engine
    sweep = ResidentSweep(model, cases, lab, 150)
    lib = _lib.load()
    ws = torch.empty(int(lib.ggad_rank_metrics_workspace_elems(sweep.n)), dtype=torch.int32, device=DEV)
    out8 = torch.zeros(8, dtype=torch.float64, device=DEV)

    def eager():
        o = torch.zeros(8, dtype=torch.float64, device=DEV)
        w = torch.empty_like(ws)
        _lib.call("ggad_rank_metrics_f32", _lib.ptr(sweep.scores()), _lib.ptr(sweep.labels), sweep.n, 0.5, _lib.ptr(o), _lib.ptr(w))
        return o.cpu().numpy()

    first = eager()                                                # (also: every kernel has run once before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                  # one chain: params sync -> score -> the four metric launches
        probs = sweep.scores()
        _lib.call("ggad_rank_metrics_f32", _lib.ptr(probs), _lib.ptr(sweep.labels), sweep.n, 0.5, _lib.ptr(out8), _lib.ptr(ws))
    graph.replay()
    np.testing.assert_array_equal(out8.cpu().numpy(), first)
    assert first[7] == 0.0 and first[2] + first[3] + first[4] + first[5] == sweep.n
    seen = [first]
    for seed in (3, 4):
        _perturb(eng, seed)
        graph.replay()
        got = out8.cpu().numpy()
        np.testing.assert_array_equal(got, eager())
        assert not any(np.array_equal(got, s) for s in seen)      # the replay saw the new weights
        seen.append(got)


# ------------------------------------------------------------------ 7: the handler
def test_model_handler_with_eval_cache_on_and_off(tmp_path, capsys):
    from ggad_amd.model_handler import ModelHandler
    rowptr, col = synth.make_graph(N_NODES, 30000, 3, kind="powerlaw", max_degree=200)
    feat = synth.make_features(N_NODES, 17, 3)
    lab = synth.make_labels(N_NODES, 0.05, 3)
    runs = {}
    for key in (False, True):
        cfg = dict(data_name="synthetic", data_dir="", data=((rowptr, col), feat, lab), seed=72, model="GCN",
                   multi_relation="GNN", emb_size=64, thres=0.4, lr=0.005, weight_decay=0.007, batch_size=60, num_epochs=3,
                   valid_epochs=2, num_batches=6, n_pseudo=20, save_dir=str(tmp_path / f"run{int(key)}") + "/", test_ratio=0.67,
                   device=0, eval_cache=key)
        random.seed(72)
        np.random.seed(72)
        torch.manual_seed(72)
        capsys.readouterr()
        h = ModelHandler(cfg)
        res = h.train()
        out = capsys.readouterr().out
        assert (h.eval_sweeps[0] is not None) == key and h.eval_sweeps[0] is h.eval_sweeps[1]      # one list, one sweep
        if key:
            assert h.eval_sweeps[0].builds >= 1 and getattr(h.model, "_eval_chunks", None) is None
            builds = h.eval_sweeps[0].builds
            assert builds == -(-h.eval_sweeps[0].n // (60 * 2048))                               # built once for three sweeps
        runs[key] = dict(res=res, losses=np.stack(h.epoch_losses), end={k: v.cpu().numpy() for k, v in h.end_state.items()},
                         hist=h.valid_history, ap=h.sweep_ap, restore=re.findall(r"Restore model from epoch (\d+)", out),
                         lines=[ln for ln in out.splitlines() if ln.startswith("   GNN ")])
    off, on = runs[False], runs[True]
    np.testing.assert_array_equal(off["losses"].view(np.int64), on["losses"].view(np.int64))
    assert off["end"].keys() == on["end"].keys()
    for k in off["end"]:
        np.testing.assert_array_equal(off["end"][k].view(np.int32), on["end"][k].view(np.int32))
    assert off["restore"] == on["restore"] and len(on["restore"]) == 1
    assert [e for e, _ in off["hist"]] == [e for e, _ in on["hist"]] == [0, 2]
    for (_, a), (_, b) in zip(off["hist"], on["hist"]):
        assert (a[0], a[1], a[2], a[4]) == (b[0], b[1], b[2], b[4])                                # F1 x 3 and G-mean: from integers
        assert abs(a[3] - b[3]) <= 1e-12
    assert off["lines"] == on["lines"] and len(on["lines"]) == 6                                     # F1 / AUC to 4 decimals, TP / TN / FN / FP
    assert len(on["ap"]) == 3 and all(abs(x - z) <= 1e-12 for x, z in zip(off["ap"], on["ap"]))
    assert all(x == z for x, z in zip((off["res"][i] for i in (0, 1, 2, 4)), (on["res"][i] for i in (0, 1, 2, 4))))
    assert abs(off["res"][3] - on["res"][3]) <= 1e-12
