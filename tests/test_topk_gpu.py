"""Top-k ranking on the device: `ggad_topk_f32` (csrc/topk.hip), `metrics.top_k`, `ResidentSweep.top_k`, config keys `top_k` /
`top_k_out` and `ModelHandler.score`.

  1. every case of tests/topk_ref.py: positions, running positives and the four meta words equal the numpy statement, the scores
     equal `s[pos]` bit for bit; workspace and outputs are pre-filled with garbage.  Everything is exact: no tolerance anywhere;
  2. refusals: NaN (status 3), a label 2 (status 4), k = 0 and k = cap + 1 (no launch);
  3. without labels (NULL label and NULL out_cumpos);
  4. equal inputs, equal bytes: the `large` case twice, and on a second stream with another dirty workspace;
  5. `ResidentSweep.scores()` plus `ggad_topk_f32` captured in one graph, replayed after the weights changed;
  6. `ResidentSweep.top_k`, labelled and unlabelled, no plan built;
  7. `ModelHandler.train()` with `top_k` 0 against 200, `eval_cache` off and on;
  8. `ModelHandler.score()` from the checkpoint that run saved."""
import contextlib
import glob
import io
import random
import re

import numpy as np
import pytest
import torch

from ggad_amd import synth
import topk_ref as TK

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_NODES = 3000


def _lib():
    from ggad_amd import _lib
    return _lib


def _cap():
    return int(_lib().load().ggad_topk_max_k())


def _native(s, y, k, fill=-1, labelled=True):
    """(pos, score, cumpos or None, meta) of one call on the current stream; workspace and outputs dirty on purpose."""
    L = _lib()
    lib = L.load()
    sd = torch.from_numpy(s).to(DEV)
    yd = torch.from_numpy(y).to(DEV) if labelled else None
    ws = torch.full((int(lib.ggad_topk_workspace_elems(len(s), k)),), fill, dtype=torch.int32, device=DEV)
    pos = torch.full((k,), -7, dtype=torch.int32, device=DEV)
    val = torch.full((k,), -7.0, dtype=torch.float32, device=DEV)
    cum = torch.full((k,), -7, dtype=torch.int32, device=DEV) if labelled else None
    meta = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    torch.cuda.current_stream().wait_stream(torch.cuda.default_stream())
    L.call("ggad_topk_f32", L.ptr(sd), L.ptr(yd), len(s), k, L.ptr(pos), L.ptr(val), L.ptr(cum), L.ptr(meta), L.ptr(ws))
    torch.cuda.current_stream().synchronize()
    return pos.cpu().numpy(), val.cpu().numpy(), None if cum is None else cum.cpu().numpy(), meta.cpu().numpy()


@pytest.fixture(scope="module")
def all_cases():
    return {c[0]: c for c in TK.cases(_cap())}


CASE_NAMES = ["n1", "n63", "n64", "n65", "k1", "k_is_n", "k_above_n", "n0", "all_tied", "tie_across_ranges", "low_byte_only",
              "high_byte_only", "signed_zero", "infinity", "minus_infinity", "saturated", "saturated_small", "at_cap", "large"]


def test_the_case_list_is_complete(all_cases):
    assert sorted(all_cases) == sorted(CASE_NAMES) and _cap() >= 8192


# ------------------------------------------------------------------ 1: the cases
@pytest.mark.parametrize("name", CASE_NAMES)
def test_topk_equals_the_reference_exactly(all_cases, name):
    _, s, y, k = all_cases[name]
    if name == "at_cap":
        assert k == _cap() and len(s) == k + 3000
    ref = TK.reference(s, y, k)
    want_pos, want_score, want_cum = TK.padded(ref, k)
    pos, val, cum, meta = _native(s, y, k)
    print(f"\n[{name}] n {len(s)} k {k}: meta {meta.tolist()}, reference m {ref['m']} P {ref['n_pos']} left out {ref['tied_left_out']}")
    assert meta.tolist() == [ref["m"], 0, ref["n_pos"], ref["tied_left_out"]]
    np.testing.assert_array_equal(pos, want_pos)
    np.testing.assert_array_equal(val.view(np.int32), want_score.view(np.int32))
    np.testing.assert_array_equal(cum, want_cum)
    if name == "all_tied":
        assert pos.tolist() == list(range(700))


# ------------------------------------------------------------------ 2: refusals
def test_topk_refuses_nan_bad_labels_and_k_out_of_bounds():
    from ggad_amd.metrics import top_k
    L = _lib()
    lib = L.load()
    rng = np.random.default_rng(4)
    s = rng.random(700).astype(np.float32)
    y = (rng.random(700) < 0.3).astype(np.uint8)
    dev = lambda a: torch.from_numpy(a).to(DEV)                    # noqa: E731
    bad = s.copy()
    bad[333] = np.nan
    assert _native(bad, y, 50)[3][1] == 3
    with pytest.raises(ValueError, match="NaN"):
        top_k(dev(bad), 50, dev(y))
    with pytest.raises(ValueError, match="NaN"):
        top_k(dev(bad), 50)
    y2 = y.copy()
    y2[77] = 2
    assert _native(s, y2, 50)[3][1] == 4
    with pytest.raises(ValueError, match="neither 0 nor 1"):
        top_k(dev(s), 50, dev(y2))
    cap = _cap()
    sd = dev(s)
    for k in (0, cap + 1):
        assert lib.ggad_topk_workspace_elems(700, k) == 0
        ws = torch.full((1024,), -1, dtype=torch.int32, device=DEV)
        out = torch.full((8,), -7, dtype=torch.int64, device=DEV)
        rc = lib.ggad_topk_f32(L.ptr(sd), None, 700, k, L.ptr(out), L.ptr(out), None, L.ptr(out), L.ptr(ws), L.current_stream())
        torch.cuda.synchronize()
        assert rc == -1 and (out == -7).all() and (ws == -1).all()             # refused, nothing launched
        with pytest.raises(ValueError, match=r"ggad_topk_max_k\(\)"):
            top_k(sd, k)


# ------------------------------------------------------------------ 3: without labels
def test_topk_without_labels(all_cases):
    from ggad_amd.metrics import top_k
    for name in ("tie_across_ranges", "k_above_n"):
        _, s, y, k = all_cases[name]
        ref = TK.reference(s, y, k)
        pos, val, cum, meta = _native(s, y, k, labelled=False)
        assert cum is None and meta.tolist() == [ref["m"], 0, 0, ref["tied_left_out"]]
        np.testing.assert_array_equal(pos, TK.padded(ref, k)[0])
        r = top_k(torch.from_numpy(s).to(DEV), k)
        assert r.cum_pos is None and (r.m, r.n_pos, r.tied_left_out) == (ref["m"], 0, ref["tied_left_out"])
        assert r.pos.dtype == torch.int32 and r.ids.dtype == torch.int64 and r.scores.dtype == torch.float32
        np.testing.assert_array_equal(r.pos.cpu().numpy(), ref["pos"])
        np.testing.assert_array_equal(r.ids.cpu().numpy(), ref["pos"].astype(np.int64))
        np.testing.assert_array_equal(r.scores.cpu().numpy().view(np.int32), ref["score"].view(np.int32))


def test_top_k_with_labels_and_ids(all_cases):
    from ggad_amd.metrics import precision_recall_at, top_k
    _, s, y, k = all_cases["saturated_small"]
    ref = TK.reference(s, y, k)
    ids = np.random.default_rng(1).permutation(len(s)).astype(np.int64) + 10 ** 10
    r = top_k(torch.from_numpy(s).to(DEV), k, torch.from_numpy(y).to(DEV), torch.from_numpy(ids).to(DEV))
    np.testing.assert_array_equal(r.ids.cpu().numpy(), ids[ref["pos"]])
    np.testing.assert_array_equal(r.cum_pos.cpu().numpy(), ref["cum_pos"])
    assert (r.m, r.n_pos, r.tied_left_out) == (ref["m"], ref["n_pos"], ref["tied_left_out"])
    assert precision_recall_at(r, k) == (int(ref["cum_pos"][-1]) / k, int(ref["cum_pos"][-1]) / ref["n_pos"])


# ------------------------------------------------------------------ 4: determinism
def test_equal_inputs_give_equal_bytes(all_cases):
    _, s, y, k = all_cases["large"]
    a = _native(s, y, k)
    b = _native(s, y, k)
    with torch.cuda.stream(torch.cuda.Stream(device=DEV)):
        c = _native(s, y, k, fill=0x5A5A5A5A)
    for other in (b, c):
        for x, z in zip(a, other):
            assert x.tobytes() == z.tobytes()


# ------------------------------------------------------------------ the 3,000-node graph of tests/test_eval_cache_gpu.py
@pytest.fixture(scope="module")
def small_graph():
    rowptr, col = synth.make_graph(N_NODES, 30000, 3, kind="powerlaw", max_degree=200)
    cases = np.random.default_rng(5).choice(N_NODES, 1000, replace=False).astype(np.int64)
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


# ------------------------------------------------------------------ 5: capture
def test_scores_and_topk_replay_as_one_graph(small_graph):
    from ggad_amd.eval_cache import ResidentSweep
    L = _lib()
    _, _, cases, lab = small_graph
    model = _model(small_graph, 17, 64)
    eng = model.enc.engine
    sweep = ResidentSweep(model, cases, lab, 150)
    k = 120
    lib = L.load()
    n_ws = int(lib.ggad_topk_workspace_elems(sweep.n, k))

    def buffers():
        return (torch.full((k,), -7, dtype=torch.int32, device=DEV), torch.full((k,), -7.0, dtype=torch.float32, device=DEV),
                torch.full((k,), -7, dtype=torch.int32, device=DEV), torch.full((4,), -7, dtype=torch.int64, device=DEV),
                torch.full((n_ws,), -1, dtype=torch.int32, device=DEV))

    def run(probs, b):
        L.call("ggad_topk_f32", L.ptr(probs), L.ptr(sweep.labels), sweep.n, k, L.ptr(b[0]), L.ptr(b[1]), L.ptr(b[2]), L.ptr(b[3]), L.ptr(b[4]))

    def eager():
        b = buffers()
        run(sweep.scores(), b)
        return [x.cpu().numpy().tobytes() for x in b[:4]]

    first = eager()                                                # (also: every kernel has run once before the capture)
    held = buffers()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                  # one chain: params sync -> score -> the six top-k launches
        run(sweep.scores(), held)
    graph.replay()
    assert [x.cpu().numpy().tobytes() for x in held[:4]] == first
    assert held[3].tolist()[:2] == [k, 0]
    seen = [first]
    for seed in (3, 4):
        _perturb(eng, seed)
        graph.replay()
        got = [x.cpu().numpy().tobytes() for x in held[:4]]
        assert got == eager()
        assert got not in seen                                     # the replay saw the new weights
        seen.append(got)


# ------------------------------------------------------------------ 6: the resident sweep
def test_resident_sweep_top_k(small_graph, monkeypatch):
    from ggad_amd.eval_cache import ResidentSweep
    from ggad_amd.minibatch import BatchChunk
    _, _, cases, lab = small_graph
    model = _model(small_graph, 17, 64)
    _perturb(model.enc.engine, 2)
    sweep = ResidentSweep(model, cases, lab, 150)
    bare = ResidentSweep(model, cases, None, 150)
    calls = []
    real = BatchChunk.build
    monkeypatch.setattr(BatchChunk, "build", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    s = sweep.scores().cpu().numpy()
    k = 400
    ref = TK.reference(s, lab, k)
    dup = int(np.flatnonzero(ref["pos"] == 10)[0]) if 10 in ref["pos"] else None
    r = sweep.top_k(k)
    r2 = sweep.top_k(k)
    u = bare.top_k(k)
    assert calls == []                                             # no plan between the calls
    np.testing.assert_array_equal(r.ids.cpu().numpy(), cases[ref["pos"]])
    np.testing.assert_array_equal(r.pos.cpu().numpy(), ref["pos"])
    np.testing.assert_array_equal(r.cum_pos.cpu().numpy(), np.cumsum(lab[ref["pos"]]))
    np.testing.assert_array_equal(r.scores.cpu().numpy().view(np.int32), ref["score"].view(np.int32))
    assert (r.m, r.n_pos, r.tied_left_out) == (k, int(lab.sum()), ref["tied_left_out"])
    assert torch.equal(r.pos, r2.pos) and torch.equal(r.scores, r2.scores) and torch.equal(r.cum_pos, r2.cum_pos)
    # positions 10 and 500 hold the same id in different slices: both are elements of the list in their own right
    both = np.isin(np.array([10, 500]), ref["pos"])
    if both.all():
        assert (r.ids == int(cases[10])).sum().item() == 2
    assert dup is None or int(r.ids[dup]) == int(cases[10])
    assert u.cum_pos is None and u.n_pos == 0 and torch.equal(u.ids, r.ids) and torch.equal(u.scores, r.scores)
    with pytest.raises(ValueError, match="without labels"):
        bare.report(0.5)


# ------------------------------------------------------------------ 7, 8: the handler
LINE = re.compile(r"^Top-(\d+): precision@K (\d\.\d{4})\trecall@K (\d\.\d{4})\thits (\d+) of (\d+)\ttied left out (\d+)$", re.M)


def _config(tmp, tag, eval_cache, top_k, data):
    cfg = dict(data_name="synthetic", data_dir="", data=data, seed=72, model="GCN", multi_relation="GNN", emb_size=64, thres=0.4, lr=0.005,
               weight_decay=0.007, batch_size=60, num_epochs=3, valid_epochs=2, num_batches=6, n_pseudo=20,
               save_dir=str(tmp / tag) + "/", test_ratio=0.67, device=0, eval_cache=eval_cache)
    if top_k:
        cfg.update(top_k=top_k, top_k_out=str(tmp / (tag + ".npz")))
    return cfg


@pytest.fixture(scope="module")
def handler_runs(tmp_path_factory):
    from ggad_amd.model_handler import ModelHandler
    tmp = tmp_path_factory.mktemp("topk")
    rowptr, col = synth.make_graph(N_NODES, 30000, 3, kind="powerlaw", max_degree=200)
    data = ((rowptr, col), synth.make_features(N_NODES, 17, 3), synth.make_labels(N_NODES, 0.05, 3))
    runs = {}
    for cache in (False, True):
        for top_k in (0, 200):
            tag = f"run_c{int(cache)}_k{top_k}"
            cfg = _config(tmp, tag, cache, top_k, data)
            random.seed(72)
            np.random.seed(72)
            torch.manual_seed(72)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                h = ModelHandler(cfg)
                res = h.train()
            runs[(cache, top_k)] = dict(h=h, cfg=cfg, res=res, out=buf.getvalue(), losses=np.stack(h.epoch_losses),
                                        end={k: v.cpu().numpy() for k, v in h.end_state.items()}, hist=h.valid_history,
                                        ckpt=glob.glob(str(tmp / tag / "*" / "*.pkl")))
    return runs


@pytest.mark.parametrize("cache", [False, True])
def test_model_handler_with_top_k_on_and_off(handler_runs, cache):
    from ggad_amd.sage_utils import score_nodes
    off, on = handler_runs[(cache, 0)], handler_runs[(cache, 200)]
    np.testing.assert_array_equal(off["losses"].view(np.int64), on["losses"].view(np.int64))
    assert off["end"].keys() == on["end"].keys()
    for k in off["end"]:
        np.testing.assert_array_equal(off["end"][k].view(np.int32), on["end"][k].view(np.int32))
    assert off["hist"] == on["hist"] and off["res"] == on["res"]
    assert off["h"].ranked is None and LINE.search(off["out"]) is None
    strip = lambda o: [ln for ln in o.splitlines() if not ln.startswith(("Top-", "Model path", "Epoch:", "total_time"))]   # noqa: E731
    assert strip(off["out"]) == strip(on["out"])                   # (Epoch / total_time lines carry wall-clock times, the path a date)
    # the ranking: the reference ranking of score_nodes on the restored weights
    h = on["h"]
    idx_test, y_test = np.asarray(h.dataset["idx_test"], dtype=np.int64), np.asarray(h.dataset["y_test"])
    s = score_nodes(h.model, idx_test, 60, device=True)
    assert torch.equal(s, h.test_scores)
    ref = TK.reference(s.cpu().numpy(), y_test, 200)
    r = h.ranked
    np.testing.assert_array_equal(r.pos.cpu().numpy(), ref["pos"])
    np.testing.assert_array_equal(r.ids.cpu().numpy(), idx_test[ref["pos"]])
    np.testing.assert_array_equal(r.scores.cpu().numpy().view(np.int32), ref["score"].view(np.int32))
    np.testing.assert_array_equal(r.cum_pos.cpu().numpy(), ref["cum_pos"])
    assert (r.m, r.n_pos, r.tied_left_out) == (200, ref["n_pos"], ref["tied_left_out"])
    # the printed line, after the sweep's report
    lines = on["out"].splitlines()
    m = LINE.search(on["out"])
    assert m and len(LINE.findall(on["out"])) == 1 and lines[-1].startswith("Top-200:") and lines[-2].startswith("   GNN TP:")
    hits = int(ref["cum_pos"][-1])
    assert (int(m[1]), int(m[4]), int(m[5]), int(m[6])) == (200, hits, ref["n_pos"], ref["tied_left_out"])
    assert m[2] == f"{hits / 200:.4f}" and m[3] == f"{hits / ref['n_pos']:.4f}"
    # the file
    z = np.load(on["cfg"]["top_k_out"])
    assert sorted(z.files) == ["cum_positives", "label", "n_pos", "node", "score", "tied_left_out"]
    assert (z["node"].dtype, z["score"].dtype, z["label"].dtype, z["cum_positives"].dtype) == (np.int64, np.float32, np.uint8, np.int32)
    np.testing.assert_array_equal(z["node"], idx_test[ref["pos"]])
    np.testing.assert_array_equal(z["score"].view(np.int32), ref["score"].view(np.int32))
    np.testing.assert_array_equal(z["label"], y_test[ref["pos"]])
    np.testing.assert_array_equal(z["cum_positives"], ref["cum_pos"])
    assert (int(z["n_pos"]), int(z["tied_left_out"])) == (ref["n_pos"], ref["tied_left_out"])


def test_top_k_ranks_the_same_list_with_eval_cache_on_and_off(handler_runs):
    a, b = handler_runs[(False, 200)]["h"], handler_runs[(True, 200)]["h"]
    assert torch.equal(a.test_scores, b.test_scores) and torch.equal(a.ranked.ids, b.ranked.ids)
    assert open(handler_runs[(False, 200)]["cfg"]["top_k_out"], "rb").read() == open(handler_runs[(True, 200)]["cfg"]["top_k_out"], "rb").read()


@pytest.mark.parametrize("cache", [False, True])
def test_score_from_the_saved_checkpoint(handler_runs, cache, tmp_path, capsys):
    from ggad_amd.model_handler import ModelHandler
    from ggad_amd.sage_utils import score_nodes
    run = handler_runs[(cache, 200)]
    assert len(run["ckpt"]) == 1
    trained = run["h"]
    random.seed(5)
    np.random.seed(6)
    torch.manual_seed(7)                                           # other global seeds: the split follows from the config's seed alone
    cfg = dict(run["cfg"], top_k_out=str(tmp_path / "again.npz"), save_dir=str(tmp_path / "unused") + "/")
    h = ModelHandler(cfg)
    capsys.readouterr()
    scores, ranked = h.score(run["ckpt"][0])
    out = capsys.readouterr().out
    assert getattr(h, "trainer", None) is None                     # no training, no sampler thread
    assert torch.equal(scores, trained.test_scores) and scores.is_cuda and scores.dtype == torch.float32
    assert h.metrics == run["res"] and len(h.metrics) == 5
    assert ranked is h.ranked
    for name in ("pos", "ids", "scores", "cum_pos"):
        assert torch.equal(getattr(ranked, name), getattr(trained.ranked, name)), name
    assert (ranked.m, ranked.n_pos, ranked.tied_left_out) == (trained.ranked.m, trained.ranked.n_pos, trained.ranked.tied_left_out)
    tail = run["out"].splitlines()[-4:]
    assert out.splitlines()[-4:] == tail and tail[0].startswith("   GNN F1-binary-1") and tail[3].startswith("Top-200:")
    assert open(cfg["top_k_out"], "rb").read() == open(run["cfg"]["top_k_out"], "rb").read()
    # explicit ids, no labels: an id list to rank
    ids = np.asarray(trained.dataset["idx_test"], dtype=np.int64)[::3][:500]
    h2 = ModelHandler(dict(cfg, top_k=0, top_k_out=""))
    capsys.readouterr()
    scores2, ranked2 = h2.score(run["ckpt"][0], ids=ids, k=50)
    out2 = capsys.readouterr().out
    assert h2.metrics is None and "GNN F1" not in out2 and "Top-50: no labels" in out2
    assert torch.equal(scores2, score_nodes(h2.model, ids, 60, device=True))
    ref = TK.reference(scores2.cpu().numpy(), None, 50)
    assert ranked2.cum_pos is None and ranked2.n_pos == 0 and ranked2.tied_left_out == ref["tied_left_out"]
    np.testing.assert_array_equal(ranked2.ids.cpu().numpy(), ids[ref["pos"]])
    # k = None and the config's top_k 0: nothing is ranked
    assert h2.score(run["ckpt"][0], ids=ids)[1] is None
