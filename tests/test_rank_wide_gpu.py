"""Exact rank metrics above 8,192 positives on the device: csrc/rank_metrics.hip, `metrics.rank_report_wide`, `ResidentSweep(rank_wide=True)`
and config key `rank_wide`.

  1. every case of tests/rank_wide_ref.py through `ggad_rank_wide_f32` with `pos_cap` = P exactly and a workspace full of -1, against
     tests/rank_metrics_ref.py (exact counts), `math.fsum` and scikit-learn.  Bounds (those of tests/test_eval_cache_gpu.py): the
     confusion counts and n_pos are integers; AUROC is ONE float64 division of exact integers (numerator <= 2 P Nn < 2^53), so it
     equals the float of the exact fraction; AP is a float64 sum of P <= 2^20 terms in (0, 1] made as <= 8 terms per thread, a tree
     over 1,024 threads and a tree over <= 128 workgroups -- 8 + 10 + 7 additions deep, each within 2^-53 relative, so the sum over P is
     within 25 x 1.1e-16 = 3e-15 relative and AP within 3e-15: far inside the 1e-12 that is asserted;
  2. the same cases with `pos_cap = min(n, max_pos)`, and ONE workspace reused across five_tiles -> p8193 -> tiny: bit-equal out8;
  3. the status codes and the refused arguments;
  4. `rank_report_wide` against `binary_report` and `rank_report`, and its status-2 fallback;
  5. `ResidentSweep(rank_wide=True)` on a list with more than 8,192 positives, with and without the flag, and through `test_sage`;
  6. `scores()` plus the wide call captured in one graph and replayed after the weights changed;
  7. `ModelHandler.train()` with `rank_wide` on against off."""
import math
import random
import re

import numpy as np
import pytest
import torch

from ggad_amd import synth
import rank_metrics_ref as RM
import rank_wide_ref as RW

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_NODES = 3000
NAMES = [c[0] for c in RW.cases()]


def _case(name):
    return next(c for c in RW.cases() if c[0] == name)


def _lib():
    from ggad_amd import _lib
    return _lib, _lib.load()


def _native(s, y, thres, pos_cap, ws=None):
    """out8 of one `ggad_rank_wide_f32` call as a host array; `ws`: a workspace to reuse (default: a fresh one full of -1)."""
    L, lib = _lib()
    sd, yd = torch.tensor(s).to(DEV), torch.tensor(y).to(DEV)
    need = int(lib.ggad_rank_wide_workspace_elems(len(s), pos_cap))
    assert need > 0
    if ws is None:
        ws = torch.full((need,), -1, dtype=torch.int32, device=DEV)                # (dirty on purpose)
    assert ws.numel() >= need
    out8 = torch.full((8,), -7.0, dtype=torch.float64, device=DEV)
    L.call("ggad_rank_wide_f32", L.ptr(sd), L.ptr(yd), len(s), pos_cap, float(thres), L.ptr(out8), L.ptr(ws))
    return out8.cpu().numpy()


@pytest.fixture(scope="module")
def exact_cap():
    """out8 of every case at `pos_cap` = P, computed once (test 2 compares against it bit for bit)."""
    return {}


# ------------------------------------------------------------------ 1: every case, pos_cap = P
@pytest.mark.parametrize("name", NAMES)
def test_wide_call_against_exact_counts_and_sklearn(name, exact_cap):
    _, s, y, thres = _case(name)
    auroc_exact, ap_fsum, sk_auroc, sk_ap, conf, p = RW.expected(name)
    o = _native(s, y, thres, p)
    exact_cap[name] = o
    print(f"\n[{name}] n {len(s)} P {p}: auroc {o[0]!r} (exact {auroc_exact!r}), ap - fsum {o[1] - ap_fsum:.3g}, "
          f"auroc - sklearn {o[0] - sk_auroc:.3g}, ap - sklearn {o[1] - sk_ap:.3g}")
    assert o[7] == 0.0
    assert tuple(int(v) for v in o[2:6]) == conf and all(float(v).is_integer() for v in o[2:7])
    assert int(o[6]) == p
    assert o[0] == auroc_exact
    assert abs(o[1] - ap_fsum) <= 1e-12
    assert abs(o[0] - sk_auroc) <= 1e-12 and abs(o[1] - sk_ap) <= 1e-12


# ------------------------------------------------------------------ 2: a loose bound, a reused workspace
@pytest.mark.parametrize("name", NAMES)
def test_wide_call_with_a_loose_bound(name, exact_cap):
    _, lib = _lib()
    _, s, y, thres = _case(name)
    auroc_exact, ap_fsum, sk_auroc, sk_ap, conf, p = RW.expected(name)
    o = _native(s, y, thres, min(len(s), int(lib.ggad_rank_wide_max_pos())))
    assert o[7] == 0.0 and tuple(int(v) for v in o[2:6]) == conf and int(o[6]) == p
    assert o[0] == auroc_exact
    assert abs(o[1] - ap_fsum) <= 1e-12 and abs(o[1] - sk_ap) <= 1e-12 and abs(o[0] - sk_auroc) <= 1e-12
    if name in exact_cap:                                          # the numerator is exact either way; AP is summed per tile of 8,192
        assert o[0] == exact_cap[name][0]                          # either way, so the bound does not move its bits either
        assert o[1] == exact_cap[name][1]


def test_one_workspace_reused_shows_no_stale_keys():
    _, lib = _lib()
    order = ("five_tiles", "p8193", "tiny")
    cap = {name: min(len(_case(name)[1]), int(lib.ggad_rank_wide_max_pos())) for name in order}
    for caps in ({name: RW.expected(name)[5] for name in order}, cap):
        need = max(int(lib.ggad_rank_wide_workspace_elems(len(_case(name)[1]), caps[name])) for name in order)
        shared = torch.full((need,), -1, dtype=torch.int32, device=DEV)
        for name in order:
            _, s, y, thres = _case(name)
            fresh = _native(s, y, thres, caps[name])
            again = _native(s, y, thres, caps[name], ws=shared)
            np.testing.assert_array_equal(again.view(np.int64), fresh.view(np.int64), err_msg=name)
            assert fresh[7] == 0.0 and fresh[0] == RW.expected(name)[0]
        for name in order:                                         # and a second round over the now thoroughly used block
            _, s, y, thres = _case(name)
            np.testing.assert_array_equal(_native(s, y, thres, caps[name], ws=shared).view(np.int64),
                                          _native(s, y, thres, caps[name]).view(np.int64), err_msg=name)


# ------------------------------------------------------------------ 3: status
def test_status_codes_and_refused_arguments():
    L, lib = _lib()
    _, s, y, thres = _case("p8193")
    conf = RM.confusion(s, y, thres)
    o = _native(s, y, thres, 8192)                                 # P = pos_cap + 1
    assert o[7] == 2.0 and int(o[6]) == 8193 and tuple(int(v) for v in o[2:6]) == conf
    assert math.isnan(o[0]) and math.isnan(o[1])
    _, s5, y5, t5 = _case("five_tiles")
    o = _native(s5, y5, t5, 39999)
    assert o[7] == 2.0 and int(o[6]) == 40000 and tuple(int(v) for v in o[2:6]) == RM.confusion(s5, y5, t5) and math.isnan(o[0])
    bad = s.copy()
    bad[333] = np.nan
    o = _native(bad, y, thres, 8193)
    assert o[7] == 3.0 and math.isnan(o[0]) and math.isnan(o[1])
    y2 = y.copy()
    y2[77] = 2
    o = _native(s, y2, thres, 8193)
    assert o[7] == 4.0 and math.isnan(o[0]) and math.isnan(o[1])
    for const in (0, 1):
        y1 = np.full(len(s), const, dtype=np.uint8)
        o = _native(s, y1, thres, len(s))
        assert o[7] == 1.0 and int(o[6]) == len(s) * const and math.isnan(o[0]) and o[1] == float(const)
        assert tuple(int(v) for v in o[2:6]) == RM.confusion(s, y1, thres)
    # a bound above n is as good as n; no elements at all is "one class only" with zero counts
    _, st, yt, tt = _case("tiny")
    o = _native(st, yt, tt, int(lib.ggad_rank_wide_max_pos()))
    assert o[7] == 0.0 and o[0] == RW.expected("tiny")[0] and abs(o[1] - RW.expected("tiny")[1]) <= 1e-12
    o = _native(np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.uint8), 0.5, 5)
    assert o[7] == 1.0 and math.isnan(o[0]) and o[1] == 0.0 and (o[2:7] == 0.0).all()
    # refused without a launch: the outputs are untouched
    sd, yd = torch.tensor(s).to(DEV), torch.tensor(y).to(DEV)
    out8 = torch.full((8,), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.full((4096,), -1, dtype=torch.int32, device=DEV)
    for pos_cap in (0, int(lib.ggad_rank_wide_max_pos()) + 1):
        assert int(lib.ggad_rank_wide_workspace_elems(len(s), pos_cap)) == 0
        assert lib.ggad_rank_wide_f32(L.ptr(sd), L.ptr(yd), len(s), pos_cap, 0.5, L.ptr(out8), L.ptr(ws), None) == -1
    torch.cuda.synchronize()
    assert (out8.cpu().numpy() == -7.0).all() and bool((ws == -1).all())


# ------------------------------------------------------------------ 4: the public call
@pytest.mark.parametrize("name", ["p8193", "five_tiles"])
def test_rank_report_wide_against_binary_report(name):
    from ggad_amd.metrics import binary_report, rank_report_wide
    _, s, y, thres = _case(name)
    sd, yd = torch.tensor(s).to(DEV), torch.tensor(y).to(DEV)
    b = binary_report(sd, yd, thres)
    for pos_cap in (None, RW.expected(name)[5]):
        r = rank_report_wide(sd, yd, thres, pos_cap=pos_cap)
        assert list(r) == list(b)
        for k in ("tp", "fp", "fn", "tn", "f1_1", "f1_0", "f1_macro", "gmean"):
            assert r[k] == b[k] and type(r[k]) is type(b[k]), k
        assert abs(r["auc"] - b["auc"]) <= 1e-12 and abs(r["ap"] - b["ap"]) <= 1e-12
        assert r["auc"] == RW.expected(name)[0]


@pytest.mark.parametrize("name", ["at_cap", "pad_p1025", "tiny", "heavy_ties"])
def test_rank_report_wide_equals_rank_report_under_the_narrow_cap(name):
    from ggad_amd.metrics import rank_report, rank_report_wide
    _, s, y, thres = _case(name)
    sd, yd = torch.tensor(s).to(DEV), torch.tensor(y).to(DEV)
    a, b = rank_report(sd, yd, thres), rank_report_wide(sd, yd, thres)
    assert list(a) == list(b) and a["auc"] == b["auc"]             # bit for bit: the same exact fraction, divided once
    assert abs(a["ap"] - b["ap"]) <= 1e-12
    assert {k: a[k] for k in a if k not in ("auc", "ap")} == {k: b[k] for k in b if k not in ("auc", "ap")}


def test_rank_report_wide_falls_back_on_status_2_and_raises_like_rank_report(monkeypatch):
    from ggad_amd import metrics
    _, s, y, thres = _case("p8193")
    sd, yd = torch.tensor(s).to(DEV), torch.tensor(y).to(DEV)
    want = metrics.binary_report(sd, yd, thres)
    calls = []
    real = metrics.binary_report
    monkeypatch.setattr(metrics, "binary_report", lambda *a: (calls.append(1), real(*a))[1])
    assert metrics.rank_report_wide(sd, yd, thres, pos_cap=8193)["auc"] == RW.expected("p8193")[0] and calls == []
    got = metrics.rank_report_wide(sd, yd, thres, pos_cap=8192)
    assert calls == [1] and got == want
    monkeypatch.undo()
    bad = s.copy()
    bad[5] = np.nan
    y2 = y.copy()
    y2[5] = 3
    for args in ((torch.tensor(bad).to(DEV), yd), (sd, torch.tensor(y2).to(DEV)), (sd, torch.zeros_like(yd)), (sd, torch.ones_like(yd))):
        with pytest.raises(ValueError) as a:
            metrics.rank_report(*args, thres)
        with pytest.raises(ValueError) as b:
            metrics.rank_report_wide(*args, thres)
        assert str(a.value) == str(b.value)
    with pytest.raises(ValueError, match="pos_cap"):
        metrics.rank_report_wide(sd, yd, thres, pos_cap=0)


# ------------------------------------------------------------------ 5: the resident sweep
@pytest.fixture(scope="module")
def small_graph():
    rowptr, col = synth.make_graph(N_NODES, 30000, 3, kind="powerlaw", max_degree=200)
    rng = np.random.default_rng(8)
    cases = rng.integers(0, N_NODES, 12000).astype(np.int64)       # (ids come several times: slices normalise on their own)
    lab = np.zeros(len(cases), dtype=np.int64)
    lab[rng.choice(len(cases), 9000, replace=False)] = 1           # more positives than the narrow kernels take
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


def test_resident_sweep_with_rank_wide(small_graph, monkeypatch, capsys):
    from ggad_amd import metrics
    from ggad_amd.eval_cache import ResidentSweep
    from ggad_amd.sage_utils import test_sage as run_sweep
    _, _, cases, lab = small_graph
    model = _model(small_graph, 17, 64)
    _perturb(model.enc.engine, 2)
    wide = ResidentSweep(model, cases, lab, 150, rank_wide=True)
    plain = ResidentSweep(model, cases, lab, 150)
    assert wide.n_pos == 9000 and wide.rank_wide and not plain.rank_wide
    scores = wide.scores()
    assert torch.equal(scores, plain.scores())
    want = metrics.rank_report_wide(scores, wide.labels, 0.5, pos_cap=9000)
    calls = []
    real = metrics.binary_report
    monkeypatch.setattr(metrics, "binary_report", lambda *a: (calls.append(1), real(*a))[1])
    got = wide.report(0.5)
    assert calls == [] and got == want                             # the counting route, not the two sorts
    old = plain.report(0.5)
    assert calls == [1]                                            # without the flag: today's fallback
    assert list(old) == list(got)
    for k in ("tp", "fp", "fn", "tn", "f1_1", "f1_0", "f1_macro", "gmean"):
        assert old[k] == got[k], k
    assert abs(old["auc"] - got["auc"]) <= 1e-12 and abs(old["ap"] - got["ap"]) <= 1e-12
    sy = scores.cpu().numpy()
    assert got["auc"] == float(RM.auroc_fraction(sy, lab)) and abs(got["ap"] - RM.average_precision(sy, lab)) <= 1e-12
    monkeypatch.undo()
    # a list under the cap takes plain rank_report, flag or not
    few = lab.copy()
    few[np.flatnonzero(few)[8000:]] = 0
    under = ResidentSweep(model, cases, few, 150, rank_wide=True)
    seen = []
    real_wide = metrics.rank_report_wide
    monkeypatch.setattr(metrics, "rank_report_wide", lambda *a, **k: (seen.append(1), real_wide(*a, **k))[1])
    assert under.n_pos == 8000 and under.report(0.5) == metrics.rank_report(scores, under.labels, 0.5) and seen == []
    monkeypatch.undo()
    # test_sage: the same three lines in the same formats
    capsys.readouterr()
    a = run_sweep(cases, lab, model, 150, 0.5)
    ap_a, out_a = run_sweep.last_ap, capsys.readouterr().out.splitlines()
    b = run_sweep(cases, lab, model, 150, 0.5, resident=wide)
    ap_b, out_b = run_sweep.last_ap, capsys.readouterr().out.splitlines()
    assert len(a) == len(b) == 5 and len(out_a) == len(out_b) == 3
    assert out_a[0] == out_b[0] and out_a[2] == out_b[2]
    assert re.fullmatch(r"   GNN TP: \d+\tTN: \d+\tFN: \d+\tFP: \d+", out_b[2])
    assert out_a[1].startswith("Testing AP: ") and out_b[1].startswith("Testing AP: ")
    assert abs(float(out_a[1].split(": ")[1]) - float(out_b[1].split(": ")[1])) <= 1e-12
    assert (a[0], a[1], a[2], a[4]) == (b[0], b[1], b[2], b[4])
    assert abs(a[3] - b[3]) <= 1e-12 and abs(ap_a - ap_b) <= 1e-12


# ------------------------------------------------------------------ 6: capture
def test_scores_and_wide_metrics_replay_as_one_graph(small_graph):
    from ggad_amd.eval_cache import ResidentSweep
    L, lib = _lib()
    _, _, cases, lab = small_graph
    model = _model(small_graph, 17, 64)
    eng = model.enc.engine
    sweep = ResidentSweep(model, cases, lab, 150, rank_wide=True)
    pos_cap = sweep.n_pos
    ws = torch.empty(int(lib.ggad_rank_wide_workspace_elems(sweep.n, pos_cap)), dtype=torch.int32, device=DEV)
    out8 = torch.zeros(8, dtype=torch.float64, device=DEV)

    def eager():
        o = torch.zeros(8, dtype=torch.float64, device=DEV)
        w = torch.empty_like(ws)
        L.call("ggad_rank_wide_f32", L.ptr(sweep.scores()), L.ptr(sweep.labels), sweep.n, pos_cap, 0.5, L.ptr(o), L.ptr(w))
        return o.cpu().numpy()

    first = eager()                                                # (also: every kernel has run once before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                  # one chain: params sync -> score -> the wide metric launches
        probs = sweep.scores()
        L.call("ggad_rank_wide_f32", L.ptr(probs), L.ptr(sweep.labels), sweep.n, pos_cap, 0.5, L.ptr(out8), L.ptr(ws))
    graph.replay()
    np.testing.assert_array_equal(out8.cpu().numpy(), first)
    assert first[7] == 0.0 and first[6] == 9000.0 and first[2] + first[3] + first[4] + first[5] == sweep.n
    seen = [first]
    for seed in (3, 4):
        _perturb(eng, seed)
        graph.replay()
        got = out8.cpu().numpy()
        np.testing.assert_array_equal(got, eager())
        assert not any(np.array_equal(got, s) for s in seen)      # the replay saw the new weights
        seen.append(got)


# ------------------------------------------------------------------ 7: the handler
def test_model_handler_with_rank_wide_on_and_off(tmp_path, capsys, monkeypatch):
    from ggad_amd import metrics
    from ggad_amd.model_handler import ModelHandler
    n = 30000
    rowptr, col = synth.make_graph(n, 300000, 3, kind="powerlaw", max_degree=200)
    feat = synth.make_features(n, 17, 3)
    lab = synth.make_labels(n, 0.6, 3)
    sorts = []
    real = metrics.binary_report
    monkeypatch.setattr(metrics, "binary_report", lambda *a: (sorts.append(1), real(*a))[1])
    runs = {}
    for key in (False, True):
        cfg = dict(data_name="synthetic", data_dir="", data=((rowptr, col), feat, lab), seed=72, model="GCN",
                   multi_relation="GNN", emb_size=64, thres=0.4, lr=0.005, weight_decay=0.007, batch_size=60, num_epochs=3,
                   valid_epochs=2, num_batches=6, n_pseudo=20, save_dir=str(tmp_path / f"run{int(key)}") + "/", test_ratio=0.67,
                   device=0, eval_cache=True, rank_wide=key)
        random.seed(72)
        np.random.seed(72)
        torch.manual_seed(72)
        capsys.readouterr()
        del sorts[:]
        h = ModelHandler(cfg)
        assert int(np.sum(h.dataset["y_test"])) > 8192
        res = h.train()
        out = capsys.readouterr().out
        assert h.eval_sweeps[0] is h.eval_sweeps[1] and h.eval_sweeps[0].rank_wide == key
        assert len(sorts) == (0 if key else 3)                     # two validations and the test sweep: off = the fallback, on = none
        runs[key] = dict(res=res, losses=np.stack(h.epoch_losses), hist=h.valid_history, ap=h.sweep_ap,
                         lines=[ln for ln in out.splitlines() if ln.startswith("   GNN ")])
    off, on = runs[False], runs[True]
    np.testing.assert_array_equal(off["losses"].view(np.int64), on["losses"].view(np.int64))
    assert [e for e, _ in off["hist"]] == [e for e, _ in on["hist"]] == [0, 2]
    for (_, a), (_, b) in zip(off["hist"], on["hist"]):
        assert (a[0], a[1], a[2], a[4]) == (b[0], b[1], b[2], b[4])                                # F1 x 3 and G-mean: from integers
        assert abs(a[3] - b[3]) <= 1e-12
    assert off["lines"] == on["lines"] and len(on["lines"]) == 6
    assert len(on["ap"]) == 3 and all(abs(x - z) <= 1e-12 for x, z in zip(off["ap"], on["ap"]))
    assert all(x == z for x, z in zip((off["res"][i] for i in (0, 1, 2, 4)), (on["res"][i] for i in (0, 1, 2, 4))))
    assert abs(off["res"][3] - on["res"][3]) <= 1e-12
