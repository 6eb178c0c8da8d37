"""Top-k above 16,384 ranks on the device: `ggad_topk_wide_f32` (csrc/topk.hip), `metrics.top_k(wide=True)`,
`ResidentSweep.top_k(wide=True)`, config key `top_k_wide`, `score_from_checkpoint` with `--top_k_wide`.  Everything is exact: integers
compared with ==, floats bit for bit.

  a. every case of `topk_ref.cases(16384)` through the wide call: all outputs bit-equal to `ggad_topk_f32` on the same inputs;
  b. every case of `topk_wide_ref.cases_wide` against `padded(reference(...))`, with and without labels;
  c. workspace and outputs dirty (tests/dirty.py), the same workspace used again for a second, different input;
  d. the call captured once and replayed twice after the scores were overwritten in place;
  e. `ResidentSweep.top_k(20000, wide=True)`; without `wide` it raises as before;
  f. `ModelHandler.score` with `top_k: 20000`, `top_k_wide: true`: the `.npz`, twice, and an unlabelled id list;
  g. `fullgraph_script.score_from_checkpoint` with the wide flag: the printed precision / recall and the written list."""
import re
import types

import numpy as np
import pytest
import torch

from ggad_amd import synth
import dirty as D
import topk_ref as TK
import topk_wide_ref as TW

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _lib():
    from ggad_amd import _lib
    return _lib


def _caps():
    lib = _lib().load()
    return int(lib.ggad_topk_max_k()), int(lib.ggad_topk_wide_max_k())


def _call(entry, sd, yd, k, pos, val, cum, meta, ws):
    L = _lib()
    L.call(entry + "_f32", L.ptr(sd), L.ptr(yd), sd.numel(), k, L.ptr(pos), L.ptr(val), L.ptr(cum), L.ptr(meta), L.ptr(ws))


def _native(entry, s, y, k, fill=-1, cum_out=True):
    """(pos, score, cumpos or None, meta) of one call; workspace and outputs dirty on purpose.  `y` None: a NULL label pointer."""
    lib = _lib().load()
    sd = torch.from_numpy(s).to(DEV)
    yd = torch.from_numpy(y).to(DEV) if y is not None else None
    ws = torch.full((int(getattr(lib, entry + "_workspace_elems")(len(s), k)),), fill, dtype=torch.int32, device=DEV)
    pos = torch.full((k,), -7, dtype=torch.int32, device=DEV)
    val = torch.full((k,), -7.0, dtype=torch.float32, device=DEV)
    cum = torch.full((k,), -7, dtype=torch.int32, device=DEV) if cum_out else None
    meta = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    _call(entry, sd, yd, k, pos, val, cum, meta, ws)
    torch.cuda.synchronize()
    return pos.cpu().numpy(), val.cpu().numpy(), None if cum is None else cum.cpu().numpy(), meta.cpu().numpy()


def _same(a, b):
    assert len(a) == len(b)
    for x, z in zip(a, b):
        assert (x is None) == (z is None)
        if x is not None:
            assert x.dtype == z.dtype and x.tobytes() == z.tobytes()


def _check(got, ref, k, n_pos=None, cum_zero=False):
    """The outputs of one call against a `reference` dict."""
    pos, val, cum, meta = got
    want_pos, want_score, want_cum = TW.padded(ref, k)
    assert meta.tolist() == [ref["m"], 0, ref["n_pos"] if n_pos is None else n_pos, ref["tied_left_out"]]
    np.testing.assert_array_equal(pos, want_pos)
    np.testing.assert_array_equal(val.view(np.int32), want_score.view(np.int32))
    if cum is not None:
        np.testing.assert_array_equal(cum, np.zeros_like(want_cum) if cum_zero else want_cum)


# ------------------------------------------------------------------ a: the narrow call's cases, bit for bit
NARROW_NAMES = ["n1", "n63", "n64", "n65", "k1", "k_is_n", "k_above_n", "n0", "all_tied", "tie_across_ranges", "low_byte_only",
                "high_byte_only", "signed_zero", "infinity", "minus_infinity", "saturated", "saturated_small", "at_cap", "large"]


@pytest.fixture(scope="module")
def narrow_cases():
    return {c[0]: c for c in TK.cases(16384)}


def test_the_caps_and_the_narrow_case_list(narrow_cases):
    assert _caps() == (16384, 1 << 22) and sorted(narrow_cases) == sorted(NARROW_NAMES)


@pytest.mark.parametrize("name", NARROW_NAMES)
def test_wide_equals_narrow_bit_for_bit_where_both_serve(narrow_cases, name):
    _, s, y, k = narrow_cases[name]
    _same(_native("ggad_topk_wide", s, y, k), _native("ggad_topk", s, y, k))
    _same(_native("ggad_topk_wide", s, None, k, fill=0x5A5A5A5A, cum_out=False), _native("ggad_topk", s, None, k, cum_out=False))


# ------------------------------------------------------------------ b: the wide cases
WIDE_NAMES = ["m2047", "m2048", "m2049", "runs3", "runs5", "runs9_first_wide_k", "k_is_n", "k_above_n", "all_tied",
              "ties_across_runs_and_cut", "saturated", "zeros_and_infinities", "no_labels", "label_two", "nan_score", "at_cap"]


@pytest.fixture(scope="module")
def wide_cases():
    cases = {c[0]: c for c in TW.cases_wide(*_caps())}
    refs = {}

    def get(name):
        if name not in refs:                                       # one reference per case, shared by the tests and never written to
            _, s, y, k = cases[name]
            refs[name] = TW.reference(s, y, k)
        return cases[name], refs[name]
    get.names = sorted(cases)
    return get


def test_the_wide_case_list_is_complete(wide_cases):
    assert wide_cases.names == sorted(WIDE_NAMES)


@pytest.mark.parametrize("labelled", [True, False], ids=["labels", "no_labels"])
@pytest.mark.parametrize("name", WIDE_NAMES)
def test_wide_topk_equals_the_reference_exactly(wide_cases, name, labelled):
    (_, s, y, k), ref = wide_cases(name)
    if name == "runs9_first_wide_k":
        assert k == _caps()[0] + 1 and _lib().load().ggad_topk_workspace_elems(len(s), k) == 0     # the narrow call refuses it
    if name == "at_cap":
        assert k == _caps()[1] and len(s) == k + 3000
    got = _native("ggad_topk_wide", s, y if labelled else None, k, cum_out=labelled)
    print(f"\n[{name}] n {len(s)} k {k} labelled {labelled}: meta {got[3].tolist()}, reference m {ref['m']} P {ref['n_pos']} "
          f"left out {ref['tied_left_out']}")
    if name == "nan_score" or (name == "label_two" and labelled):
        assert got[3].tolist()[:2] == [ref["m"], TW.STATUS_ONLY[name]]
        return
    if labelled and y is not None:
        _check(got, ref, k)
    else:                                                          # a NULL label pointer: no positives anywhere
        _check(got, ref, k, n_pos=0, cum_zero=True)
    if name == "all_tied":
        assert got[0].tolist() == list(range(25000))


def test_metrics_top_k_wide_and_its_refusals(wide_cases):
    from ggad_amd.metrics import precision_recall_at, top_k
    (_, s, y, k), ref = wide_cases("ties_across_runs_and_cut")
    dev = lambda a: torch.from_numpy(a).to(DEV)                    # noqa: E731
    ids = np.random.default_rng(1).permutation(len(s)).astype(np.int64) + 10 ** 10
    with pytest.raises(ValueError, match=r"ggad_topk_max_k\(\)"):
        top_k(dev(s), k, dev(y))
    r = top_k(dev(s), k, dev(y), dev(ids), wide=True)
    assert (r.m, r.n_pos, r.tied_left_out) == (ref["m"], ref["n_pos"], ref["tied_left_out"])
    np.testing.assert_array_equal(r.pos.cpu().numpy(), ref["pos"])
    np.testing.assert_array_equal(r.ids.cpu().numpy(), ids[ref["pos"]])
    np.testing.assert_array_equal(r.scores.cpu().numpy().view(np.int32), ref["score"].view(np.int32))
    np.testing.assert_array_equal(r.cum_pos.cpu().numpy(), ref["cum_pos"])
    assert precision_recall_at(r, k) == (int(ref["cum_pos"][-1]) / k, int(ref["cum_pos"][-1]) / ref["n_pos"])
    u = top_k(dev(s), k, wide=True)
    assert u.cum_pos is None and u.n_pos == 0 and torch.equal(u.pos, r.pos)
    for name, text in (("nan_score", "NaN"), ("label_two", "neither 0 nor 1")):
        (_, s2, y2, k2), _ = wide_cases(name)
        with pytest.raises(ValueError, match=text):
            top_k(dev(s2), k2, dev(y2), wide=True)
    with pytest.raises(ValueError, match=r"ggad_topk_wide_max_k\(\)"):
        top_k(dev(s), _caps()[1] + 1, wide=True)


# ------------------------------------------------------------------ c: dirty, reused memory
@pytest.mark.parametrize("fill", [D.NAN_BITS, -1, 0x5A5A5A5A], ids=["nan", "ones", "5a"])
def test_a_dirty_workspace_used_twice_changes_nothing(wide_cases, fill):
    lib = _lib().load()
    (_, sa, ya, ka), ref_a = wide_cases("ties_across_runs_and_cut")
    (_, sb, yb, kb), ref_b = wide_cases("runs9_first_wide_k")
    n_ws = int(lib.ggad_topk_wide_workspace_elems(len(sa), ka))
    assert n_ws >= int(lib.ggad_topk_wide_workspace_elems(len(sb), kb))
    ws_block, ws = D.int_like(n_ws, fill)                          # filled once, before the first call only
    for (s, y, k, ref) in ((sa, ya, ka, ref_a), (sb, yb, kb, ref_b), (sa, ya, ka, ref_a)):
        sd, yd = torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV)
        pos_block, pos = D.int_like(k, fill)
        cum_block, cum = D.int_like(k, fill)
        val = D.nan_like(k)
        meta = torch.full((4,), fill, dtype=torch.int64, device=DEV)
        _call("ggad_topk_wide", sd, yd, k, pos, val, cum, meta, ws)
        torch.cuda.synchronize()
        got = (pos.cpu().numpy(), val.cpu().numpy(), cum.cpu().numpy(), meta.cpu().numpy())
        D.dirty_lines()
        _check(got, ref, k)
        _same(got, _native("ggad_topk_wide", s, y, k, fill=0))     # fresh, zeroed memory
        D.guards_intact(val)
        for block in (pos_block, cum_block, ws_block):
            assert (block[:D.GUARD] == fill).all() and (block[-D.GUARD:] == fill).all()


# ------------------------------------------------------------------ d: capture
def test_the_wide_call_replays_as_one_graph():
    lib = _lib().load()
    n, k = 60000, 20000
    rng = np.random.default_rng(9)
    y = (rng.random(n) < 0.02).astype(np.uint8)
    inputs = [TW.sigmoid32(rng.normal(0.0, 6.0, n)) for _ in range(3)]
    sd = torch.from_numpy(inputs[0]).to(DEV)
    yd = torch.from_numpy(y).to(DEV)
    n_ws = int(lib.ggad_topk_wide_workspace_elems(n, k))

    def buffers():
        return (torch.full((k,), -7, dtype=torch.int32, device=DEV), torch.full((k,), -7.0, dtype=torch.float32, device=DEV),
                torch.full((k,), -7, dtype=torch.int32, device=DEV), torch.full((4,), -7, dtype=torch.int64, device=DEV),
                torch.full((n_ws,), -1, dtype=torch.int32, device=DEV))

    def eager():
        b = buffers()
        _call("ggad_topk_wide", sd, yd, k, *b)
        torch.cuda.synchronize()
        return [x.cpu().numpy().tobytes() for x in b[:4]]

    first = eager()                                                # (also: every kernel has run once before the capture)
    held = buffers()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _call("ggad_topk_wide", sd, yd, k, *held)
    graph.replay()
    torch.cuda.synchronize()
    assert [x.cpu().numpy().tobytes() for x in held[:4]] == first
    seen = [first]
    for s in inputs[1:]:
        sd.copy_(torch.from_numpy(s))                              # overwritten in place: the captured launches hold its address
        graph.replay()
        torch.cuda.synchronize()
        got = [x.cpu().numpy().tobytes() for x in held[:4]]
        assert got == eager() and got not in seen
        seen.append(got)
        ref = TW.reference(s, y, k)
        assert held[3].tolist() == [k, 0, ref["n_pos"], ref["tied_left_out"]]
        np.testing.assert_array_equal(held[0].cpu().numpy(), ref["pos"])


# ------------------------------------------------------------------ e: the resident sweep
def _graph(n, seed=3):
    return synth.make_graph(n, 10 * n, seed, kind="powerlaw", max_degree=200)


def test_resident_sweep_top_k_wide():
    from ggad_amd.dgraph import normalize_features
    from ggad_amd.eval_cache import ResidentSweep
    from ggad_amd.graph import DeviceGraph
    from ggad_amd.graphsage import GCN, FeatureTable, GCNAggregator, GCNEncoder
    n, f = 40000, 17
    rowptr, col = _graph(n)
    torch.manual_seed(0)
    graph = DeviceGraph(rowptr, col, DEV)
    features = FeatureTable(torch.from_numpy(normalize_features(synth.make_features(n, f, 3)).astype(np.float32)))
    enc = GCNEncoder(features, f, 64, graph, GCNAggregator(features, cuda=True), gcn=True, cuda=True)
    model = GCN(2, enc)
    enc.engine.sync_params()
    cases = np.random.default_rng(5).choice(n, 30000, replace=False).astype(np.int64)
    lab = (np.random.default_rng(6).random(len(cases)) < 0.05).astype(np.int64)
    sweep = ResidentSweep(model, cases, lab, 150)
    scores = sweep.scores()
    ref = TW.reference(scores.cpu().numpy(), lab, 20000)
    with pytest.raises(ValueError, match=r"ggad_topk_max_k\(\) = 16384"):
        sweep.top_k(20000)
    r = sweep.top_k(20000, wide=True)
    r2 = sweep.top_k(20000, scores=scores, wide=True)
    np.testing.assert_array_equal(r.pos.cpu().numpy(), ref["pos"])
    np.testing.assert_array_equal(r.ids.cpu().numpy(), cases[ref["pos"]])
    np.testing.assert_array_equal(r.scores.cpu().numpy().view(np.int32), ref["score"].view(np.int32))
    np.testing.assert_array_equal(r.cum_pos.cpu().numpy(), ref["cum_pos"])
    assert (r.m, r.n_pos, r.tied_left_out) == (20000, ref["n_pos"], ref["tied_left_out"])
    assert torch.equal(r.pos, r2.pos) and torch.equal(r.scores, r2.scores) and torch.equal(r.cum_pos, r2.cum_pos)


# ------------------------------------------------------------------ f: the handler
def test_model_handler_score_with_top_k_wide(tmp_path, capsys):
    from ggad_amd.model_handler import ModelHandler
    n = 50000
    rowptr, col = _graph(n)
    data = ((rowptr, col), synth.make_features(n, 17, 3), synth.make_labels(n, 0.05, 3))
    cfg = dict(data_name="synthetic", data_dir="", data=data, seed=72, model="GCN", multi_relation="GNN", emb_size=64, thres=0.4, lr=0.005,
               weight_decay=0.007, batch_size=150, num_epochs=1, valid_epochs=1, num_batches=2, n_pseudo=20,
               save_dir=str(tmp_path / "unused") + "/", test_ratio=0.67, device=0, eval_cache=True, top_k=20000, top_k_wide=True,
               top_k_out=str(tmp_path / "a.npz"))
    h = ModelHandler(cfg)
    torch.manual_seed(11)
    ckpt = str(tmp_path / "w.pkl")
    torch.save(h._build_gcn()[3].state_dict(), ckpt)               # untrained weights: a ranking is a ranking
    capsys.readouterr()
    scores, ranked = h.score(ckpt)
    out = capsys.readouterr().out
    idx_test, y_test = np.asarray(h.dataset["idx_test"], dtype=np.int64), np.asarray(h.dataset["y_test"])
    assert len(idx_test) > 20000
    ref = TW.reference(scores.cpu().numpy(), y_test, 20000)
    hits = int(ref["cum_pos"][-1])
    assert out.splitlines()[-1] == (f"Top-20000: precision@K {hits / 20000:.4f}\trecall@K {hits / ref['n_pos']:.4f}\thits {hits} of "
                                    f"{ref['n_pos']}\ttied left out {ref['tied_left_out']}")
    np.testing.assert_array_equal(ranked.pos.cpu().numpy(), ref["pos"])
    z = np.load(cfg["top_k_out"])
    np.testing.assert_array_equal(z["node"], idx_test[ref["pos"]])
    np.testing.assert_array_equal(z["score"].view(np.int32), ref["score"].view(np.int32))
    np.testing.assert_array_equal(z["label"], y_test[ref["pos"]])
    np.testing.assert_array_equal(z["cum_positives"], ref["cum_pos"])
    assert (int(z["n_pos"]), int(z["tied_left_out"])) == (ref["n_pos"], ref["tied_left_out"])
    h2 = ModelHandler(dict(cfg, top_k_out=str(tmp_path / "b.npz")))
    h2.score(ckpt)
    assert open(cfg["top_k_out"], "rb").read() == open(str(tmp_path / "b.npz"), "rb").read()
    # an unlabelled id list: every second node of the graph
    ids = np.arange(0, n, 2, dtype=np.int64)
    h3 = ModelHandler(dict(cfg, top_k_out=str(tmp_path / "c.npz")))
    capsys.readouterr()
    scores3, ranked3 = h3.score(ckpt, ids=ids)
    assert "Top-20000: no labels" in capsys.readouterr().out and h3.metrics is None
    ref3 = TW.reference(scores3.cpu().numpy(), None, 20000)
    assert ranked3.cum_pos is None and ranked3.n_pos == 0 and ranked3.tied_left_out == ref3["tied_left_out"]
    z3 = np.load(str(tmp_path / "c.npz"))
    np.testing.assert_array_equal(z3["node"], ids[ref3["pos"]])
    np.testing.assert_array_equal(z3["score"].view(np.int32), ref3["score"].view(np.int32))
    assert z3["cum_positives"].size == 0 and z3["label"].size == 0 and int(z3["n_pos"]) == 0
    # without the key the same K is today's error, before anything is built
    with pytest.raises(ValueError, match=r"ggad_topk_max_k\(\) = 16384"):
        ModelHandler(dict(cfg, top_k_wide=False))


# ------------------------------------------------------------------ g: the full-graph scripts
LINE = re.compile(r"^top (\d+) of (\d+) test nodes: precision@(\d+) (\d\.\d{4}) recall@(\d+) (\d\.\d{4}) \((\d+) positives among the test "
                  r"nodes, (\d+) tied with the last rank left out\)$", re.M)


def test_score_from_checkpoint_with_the_wide_flag(tmp_path, capsys):
    from ggad_amd.fullgraph_script import save_checkpoint, score_from_checkpoint
    n, n_test, k = 30000, 20000, 20000
    rng = np.random.default_rng(12)
    fixed = torch.from_numpy(TW.sigmoid32(rng.normal(0.0, 8.0, n))).to(DEV)
    ano = (rng.random(n) < 0.06).astype(np.int64)
    idx_test = np.sort(rng.choice(n, n_test, replace=False)).astype(np.int64)
    model = torch.nn.Linear(12, 16)
    ckpt, out_npz = str(tmp_path / "w.pt"), str(tmp_path / "r.npz")
    base = dict(dataset="photo", embedding_dim=16, seed=0)
    save_checkpoint(ckpt, model.state_dict(), types.SimpleNamespace(**base), 12, n, epoch=0)
    args = types.SimpleNamespace(score=ckpt, top_k=k, top_k_out=out_npz, top_k_wide=True, **base)
    capsys.readouterr()
    scores, _, _, ranked = score_from_checkpoint(args, model, lambda: fixed, 12, idx_test, ano, torch.device(DEV))
    out = capsys.readouterr().out
    s = fixed.cpu().numpy()[idx_test]
    y = ano[idx_test]
    ref = TW.reference(s, y, k)
    hits = int(ref["cum_pos"][-1])
    m = LINE.search(out)
    assert m, out
    assert [int(m[i]) for i in (1, 2, 3, 5, 7, 8)] == [k, n_test, k, k, ref["n_pos"], ref["tied_left_out"]]
    assert (m[4], m[6]) == (f"{hits / k:.4f}", f"{hits / ref['n_pos']:.4f}")
    np.testing.assert_array_equal(ranked.pos.cpu().numpy(), ref["pos"])
    z = np.load(out_npz)
    np.testing.assert_array_equal(z["node"], idx_test[ref["pos"]])
    np.testing.assert_array_equal(z["score"].view(np.int32), ref["score"].view(np.int32))
    np.testing.assert_array_equal(z["label"], y[ref["pos"]])
    np.testing.assert_array_equal(z["cum_positives"], ref["cum_pos"])
    assert (int(z["n_pos"]), int(z["tied_left_out"])) == (ref["n_pos"], ref["tied_left_out"])
    with pytest.raises(ValueError, match=r"--top_k: k = 20000 is outside 1\.\.ggad_topk_max_k\(\)"):      # without the flag: as before
        score_from_checkpoint(types.SimpleNamespace(score=ckpt, top_k=k, **base), model, lambda: fixed, 12, idx_test, ano, torch.device(DEV))
