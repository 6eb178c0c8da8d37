"""`ggad_explain_f32` (csrc/explain.hip) and its routes against the float64 reference of tests/explain_ref.py:
  1. per shape (D, F), batch size and m: exact integers (closed sizes, every c_j of the workspace dump, the listed counts, the
     padding), the exact selection (a numpy lexsort of the kernel's own dumped float32 t_j, bit for bit), every float within the
     helper's bound, completeness on the device's own numbers, agreement with `score_nodes` and `ResidentSweep.scores()`, the meta
     words, determinism (twice, and on a workspace of 0xFF bytes), K = 1 and a position given twice;
  2. `ResidentSweep.explain` equals the free function bit for bit and builds no plan;
  3. `ModelHandler`: the closing sweep of `train()` and `score()` with `explain: 5`; off by default."""
import contextlib
import functools
import glob
import io
import random
import re

import numpy as np
import pytest
import torch

from ggad_amd import synth
import explain_ref as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTPUTS = ("logit", "feature", "closed_size", "nbr_id", "nbr_contrib", "nbr_colcount", "rest")


@functools.lru_cache(maxsize=None)
def _graph():
    from ggad_amd.graph import DeviceGraph
    return DeviceGraph(*X.graph(), DEV)


@functools.lru_cache(maxsize=None)
def _model(d, f):
    from ggad_amd.graphsage import GCN, FeatureTable, GCNAggregator, GCNEncoder
    features = FeatureTable(torch.from_numpy(X.feat(f).copy()))
    enc = GCNEncoder(features, f, d, _graph(), GCNAggregator(features, cuda=True), gcn=True, cuda=True)
    return GCN(2, enc)


def _load(model, d, f, variant):
    model.enc.engine.load_params(*(torch.from_numpy(x) for x in X.params(d, f, variant)))


def _bits(e, with_dump=True):
    torch.cuda.synchronize()
    out = [getattr(e, name).cpu().numpy().tobytes() for name in OUTPUTS]
    if with_dump:
        for k in range(int(e.pos.numel())):
            t, c = e.neighbours(k)
            out += [t.cpu().numpy().tobytes(), c.cpu().numpy().tobytes()]
    return out


def _check(e, ref, pos_list, m, what):
    """Every check of group 1 on one `Explanation`; returns the worst error / bound."""
    cap = X.caps()[0]
    got = {name: getattr(e, name).cpu().numpy() for name in OUTPUTS}
    assert got["nbr_id"].dtype == np.int64 and got["nbr_colcount"].dtype == np.int32 and got["closed_size"].dtype == np.int32
    assert e.rows == len(pos_list) and e.rows_workspace == sum(ref[p]["r"] > cap for p in pos_list), what
    worst = 0.0
    for k, p in enumerate(pos_list):
        v, w = ref[p], (what, "position", p)
        r = v["r"]
        # exact integers
        assert int(got["closed_size"][k]) == r, w
        t32, c32 = (x.cpu().numpy() for x in e.neighbours(k))
        assert t32.dtype == np.float32 and c32.dtype == np.int32 and len(t32) == len(c32) == r, w
        np.testing.assert_array_equal(c32, v["c"], err_msg=str(w))
        lm = min(m, r)
        ids, con, cc = got["nbr_id"][k], got["nbr_contrib"][k], got["nbr_colcount"][k]
        assert (ids[lm:] == -1).all() and (con[lm:].view(np.int32) == 0).all() and (cc[lm:] == 0).all(), w       # -1 / +0.0 / 0
        # the selection, exact: the kernel's own float32 contributions, descending, ties by ascending id
        sel = np.lexsort((np.arange(r), -t32))[:lm]
        np.testing.assert_array_equal(ids[:lm], v["nbr"][sel], err_msg=str(w))
        np.testing.assert_array_equal(con[:lm].view(np.int32), t32[sel].view(np.int32), err_msg=str(w))
        np.testing.assert_array_equal(cc[:lm], v["c"][sel], err_msg=str(w))
        assert len(set(ids[:lm].tolist())) == lm and np.isin(ids[:lm], v["nbr"]).all(), w
        # values against float64
        rest_sel = np.setdiff1d(np.arange(r), sel)
        b_rest = X.gam(v["rest_terms"]) * v["s_t"][rest_sel].sum()
        checks = [("t_j", t32, v["t"], v["b_t"]), ("feature", got["feature"][k], v["feature"], v["b_feature"]),
                  ("logit", got["logit"][k], v["z"], v["b_z"]), ("rest", got["rest"][k], v["t"][rest_sel].sum(), b_rest),
                  # completeness on the device's own numbers (summed here in float64)
                  ("logit = listed + rest", got["logit"][k], con[:lm].astype(np.float64).sum() + float(got["rest"][k]),
                   v["b_z"] + v["b_t"][sel].sum() + b_rest),
                  ("logit = sum of features", got["logit"][k], got["feature"][k].astype(np.float64).sum(), v["b_z"] + v["b_feature"].sum())]
        for name, a, b, bound in checks:
            a, b, bound = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(bound, dtype=np.float64)
            assert np.isfinite(a).all(), (w, name)
            err = np.abs(a - b)
            assert (err <= bound).all(), (w, name, float(err.max()), float((err / np.maximum(bound, 1e-300)).max()))
            nz = bound > 0
            if nz.any():
                worst = max(worst, float((err[nz] / bound[nz]).max()))
        if not v["mask"].any():                                      # the z = 0 row: every contribution is 0 and the ids ascend
            assert got["logit"][k] == 0.0 and not t32.any() and (np.diff(ids[:lm]) > 0).all(), w
    return worst


def _check_scores(e, ref, pos_list, probs, what):
    """sigmoid(logit) against the product path's probability at the same position: the two z's are within their bounds of the
    float64 z, the sigmoid is 1/4-Lipschitz and adds 4 roundings on a value of at most 1."""
    p = probs.cpu().numpy().astype(np.float64)
    logit = e.logit.cpu().numpy()
    worst = 0.0
    for k, pos in enumerate(pos_list):
        v = ref[pos]
        bound = 0.25 * (v["b_z"] + v["b_score_z"]) + 4 * X.U
        err = abs(float(X.sigmoid(logit[k])) - p[pos])
        assert err <= bound, (what, "position", pos, err, err / bound)
        worst = max(worst, err / bound)
    return worst


@pytest.mark.parametrize("d,f", X.shapes())
def test_explain_against_float64(d, f):
    from ggad_amd.eval_cache import ResidentSweep
    from ggad_amd.explain import explain
    from ggad_amd.sage_utils import score_nodes
    from ggad_amd import _lib
    lib = _lib.load()
    m_max = X.caps()[1]
    model = _model(d, f)
    ids = X.cases()
    ids_dev = torch.from_numpy(ids).to(DEV)
    worst = {"values": 0.0, "score_nodes": 0.0, "resident": 0.0}
    for bs in X.BATCH_SIZES:
        pos_list = X.positions_twice(bs)
        pos_dev = torch.tensor(pos_list, dtype=torch.int32, device=DEV)
        for variant in X.VARIANTS:
            _load(model, d, f, variant)
            ref = X.reference(d, f, bs, variant)
            what = f"D={d} F={f} bs={bs} {variant}"
            for m in ((1, 5, m_max) if variant == "signed" else (5,)):
                e = explain(model, ids_dev, bs, pos_dev, m)
                worst["values"] = max(worst["values"], _check(e, ref, pos_list, m, f"{what} m={m}"))
                if m != 5:
                    continue
                # the product score at the same positions, both routes
                worst["score_nodes"] = max(worst["score_nodes"], _check_scores(e, ref, pos_list, score_nodes(model, ids, bs, device=True), what))
                sweep = ResidentSweep(model, ids, None, bs)
                worst["resident"] = max(worst["resident"], _check_scores(e, ref, pos_list, sweep.scores(), what))
                del sweep
                # determinism: again, and on a workspace of 0xFF bytes (positions as a host list: the same call)
                first = _bits(e)
                assert _bits(explain(model, ids_dev, bs, list(pos_list), m)) == first, what
                need = int(lib.ggad_explain_workspace_elems(e.stride, len(pos_list), m))
                dirty = torch.full((need,), -1, dtype=torch.int32, device=DEV)
                e2 = explain(model, ids_dev, bs, pos_dev, m, workspace=dirty)
                assert e2.workspace is dirty and _bits(e2) == first, what
        # K = 1: hub B alone (the workspace branch), hub A alone (the LDS of exactly the cap) and the isolated node alone (of one entry)
        _load(model, d, f, "signed")
        ref = X.reference(d, f, bs, "signed")
        for p in (160, 20, 25):
            e = explain(model, ids_dev, bs, torch.tensor([p], dtype=torch.int32, device=DEV), m_max)
            _check(e, ref, (p,), m_max, f"D={d} F={f} bs={bs} K=1")
            assert e.rows_workspace == (1 if p == 160 else 0)
    print(f"\nexplain D={d} F={f}: worst error / bound: values {worst['values']:.3f}, sigmoid(logit) vs score_nodes {worst['score_nodes']:.3f}, "
          f"vs ResidentSweep.scores {worst['resident']:.3f}")


def test_explain_refuses_what_it_cannot_explain():
    from ggad_amd.explain import explain
    model = _model(64, 17)
    _load(model, 64, 17, "signed")
    ids_dev = torch.from_numpy(X.cases()).to(DEV)
    n = len(X.cases())
    for bad in ([n], [-1], [0, n + 5]):
        with pytest.raises(ValueError, match="outside the scored list"):
            explain(model, ids_dev, 150, torch.tensor(bad, dtype=torch.int32, device=DEV), 5)
    with pytest.raises(ValueError, match="on a GPU"):
        explain(model, ids_dev, 150, torch.tensor([0], dtype=torch.int32), 5)
    with pytest.raises(ValueError, match="ggad_explain_max_nbrs"):
        explain(model, ids_dev, 150, torch.tensor([0], dtype=torch.int32, device=DEV), X.caps()[1] + 1)
    e = explain(model, ids_dev, 150, torch.zeros(0, dtype=torch.int32, device=DEV), 5)          # K = 0: nothing to do
    assert e.rows == 0 and e.logit.numel() == 0 and e.completeness() == 0.0


def test_resident_sweep_explain_equals_the_free_function(monkeypatch):
    from ggad_amd.eval_cache import ResidentSweep
    from ggad_amd.explain import explain
    from ggad_amd.minibatch import BatchChunk
    model = _model(64, 17)
    _load(model, 64, 17, "signed")
    ids = X.cases()
    sweep = ResidentSweep(model, ids, None, 150)
    calls = []
    real = BatchChunk.build
    monkeypatch.setattr(BatchChunk, "build", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    ranked = sweep.top_k(40)
    a = sweep.explain(ranked, 5)
    b = explain(model, torch.from_numpy(ids).to(DEV), 150, ranked.pos, 5)
    c = sweep.explain(ranked.pos, 5)
    assert calls == []                                               # no plan between the calls
    assert _bits(a) == _bits(b) == _bits(c)
    assert torch.equal(a.pos, ranked.pos) and a.rows == 40
    # the explained logit is the ranked score's
    ref_p = ranked.scores.cpu().numpy().astype(np.float64)
    assert np.abs(X.sigmoid(a.logit.cpu().numpy()) - ref_p).max() < 1e-5


# ------------------------------------------------------------------ 3: the handler
LINE = re.compile(r"^\[explain\] rows explained (\d+)\tneighbours listed (\d+)\tmax \|z - sum_j t_j\| (\S+)\trows on the workspace branch (\d+)$",
                  re.M)
N_NODES = 3000


def _config(tmp, tag, data, **kw):
    cfg = dict(data_name="synthetic", data_dir="", data=data, seed=72, model="GCN", multi_relation="GNN", emb_size=64, thres=0.4, lr=0.005,
               weight_decay=0.007, batch_size=60, num_epochs=3, valid_epochs=2, num_batches=6, n_pseudo=20,
               save_dir=str(tmp / tag) + "/", test_ratio=0.67, device=0)
    cfg.update(kw)
    return cfg


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    from ggad_amd.model_handler import ModelHandler
    tmp = tmp_path_factory.mktemp("explain")
    rowptr, col = synth.make_graph(N_NODES, 30000, 3, kind="powerlaw", max_degree=200)
    data = ((rowptr, col), synth.make_features(N_NODES, 17, 3), synth.make_labels(N_NODES, 0.05, 3))
    cfg = _config(tmp, "run", data, top_k=20, explain=5, explain_out=str(tmp / "train.npz"))
    random.seed(72)
    np.random.seed(72)
    torch.manual_seed(72)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        h = ModelHandler(cfg)
        res = h.train()
    return dict(h=h, cfg=cfg, res=res, out=buf.getvalue(), tmp=tmp, ckpt=glob.glob(str(tmp / "run" / "*" / "*.pkl")))


def test_the_closing_sweep_of_train_explains_the_ranked_list(trained):
    h, out = trained["h"], trained["out"]
    assert len(LINE.findall(out)) == 1 and out.count("[explain]") == 1
    m = LINE.search(out)
    e = h.explained
    assert (int(m[1]), int(m[2]), int(m[4])) == (20, 5, 0) and float(m[3]) < 1e-5
    assert e.rows == 20 and torch.equal(e.pos, h.ranked.pos)
    assert np.abs(X.sigmoid(e.logit.cpu().numpy()) - h.ranked.scores.cpu().numpy()).max() < 1e-5
    z = np.load(trained["cfg"]["explain_out"])
    np.testing.assert_array_equal(z["node"], h.ranked.ids.cpu().numpy())
    np.testing.assert_array_equal(z["nbr_id"], e.nbr_id.cpu().numpy())


@pytest.mark.parametrize("cache", [False, True])
def test_score_with_explain_on_and_off(trained, cache, tmp_path, capsys):
    from ggad_amd.model_handler import ModelHandler
    assert len(trained["ckpt"]) == 1
    ckpt = trained["ckpt"][0]
    path = tmp_path / "e.npz"
    cfg = dict(trained["cfg"], explain_out=str(path), save_dir=str(tmp_path / "unused") + "/", eval_cache=cache)
    h = ModelHandler(cfg)
    capsys.readouterr()
    _, ranked = h.score(ckpt, k=20)
    out = capsys.readouterr().out
    assert len(LINE.findall(out)) == 1 and out.count("[explain]") == 1 and out.splitlines()[-1].startswith("[explain]")
    assert h.explained is not None and h.explained.rows == 20 and h.explained.m == 5
    assert _bits(h.explained, with_dump=False) == _bits(trained["h"].explained, with_dump=False)      # the restored weights: the same bits
    z = np.load(str(path))
    np.testing.assert_array_equal(z["node"], ranked.ids.cpu().numpy())
    np.testing.assert_array_equal(z["score"].view(np.int32), ranked.scores.cpu().numpy().view(np.int32))
    assert open(str(path), "rb").read() == open(trained["cfg"]["explain_out"], "rb").read()
    # off by default: the same call without the keys prints no [explain] line and writes no file
    off = {k: v for k, v in cfg.items() if k not in ("explain", "explain_out")}
    path.unlink()
    h2 = ModelHandler(off)
    capsys.readouterr()
    _, ranked2 = h2.score(ckpt, k=20)
    out2 = capsys.readouterr().out
    assert "[explain]" not in out2 and h2.explained is None and not path.exists()
    assert torch.equal(ranked2.ids, ranked.ids) and torch.equal(ranked2.scores, ranked.scores)
    assert [ln for ln in out.splitlines() if not ln.startswith("[explain]")][-4:] == out2.splitlines()[-4:]      # report and Top-20 line
