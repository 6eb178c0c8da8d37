"""GPU tests of the full-graph DOMINANT path (csrc/dominant.hip through `ggad_amd.model_dominant`): the fused autoencoder against
float64 at every tile and workgroup branch, against the wide path, and bit for bit against itself; the model against the fixtures
captured from the imported reference (tests/golden/make_golden_dominant.py); AUROC / AP on a planted schedule; the emb cache; one
epoch at each published size against tests/dominant_fp64.py; and the script's captured epoch against its eager one."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import dominant_fp64 as R
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H = 300
TILE = 16


def _bound(h=H):
    from ggad_amd.model_dominant import fused_supported
    f = 1
    while fused_supported(f + 1, h):
        f += 1
    return f


def _graph(n):
    """I plus about 4 random entries per row (drawn with replacement: sp.random's sampling without replacement costs O(n^2) host
    time and memory at these sizes)."""
    rng = np.random.default_rng(1)
    r, c = rng.integers(0, n, 4 * n), rng.integers(0, n, 4 * n)
    a = sp.eye(n, format="csr") + sp.csr_matrix((rng.random(4 * n), (r, c)), shape=(n, n))
    from ggad_amd.fullgraph import FullGraphAdj
    return FullGraphAdj(a, a, DEV)


def _params(F, h, seed):
    g = torch.Generator().manual_seed(seed)
    w1 = (torch.rand(h, F, generator=g) - 0.5) * (2 / np.sqrt(F))
    b1 = (torch.rand(h, generator=g) - 0.5) * 0.2
    w2 = (torch.rand(F, h, generator=g) - 0.5) * (2 / np.sqrt(h))
    b2 = (torch.rand(F, generator=g) - 0.5) * 0.2
    return [t.to(DEV).requires_grad_(True) for t in (w1, b1, w2, b2)]


def _run(fn, ps, x, rs):
    for p in ps:
        p.grad = None
    loss, score = fn(*ps, x, rs)
    loss.backward()
    return loss.item(), score.detach().cpu().numpy(), [p.grad.detach().cpu().numpy().copy() for p in ps]


def _fused(w1, b1, w2, b2, x, rs):
    from ggad_amd.model_dominant import FusedAeFn
    return FusedAeFn.apply(w1, b1, w2, b2, x, rs)


def _wide(w1, b1, w2, b2, x, rs):
    from ggad_amd.model_dominant import wide_loss
    return wide_loss(x, w1, b1, w2, b2, rs)


def _check64(F, ps, x, tr, te, got, rtol=2e-4):
    P = {k: p.detach().cpu().double().requires_grad_(True) for k, p in
         zip(["dense_attr_1.weight", "dense_attr_1.bias", "dense_attr_2.weight", "dense_attr_2.bias"], ps)}
    loss, score, grads = R.ae_grads(P, x.cpu().double(), tr, te)
    lg, sg, gg = got
    assert abs(lg - loss.item()) <= 2e-5 * abs(loss.item()), (F, lg, loss.item())
    np.testing.assert_allclose(sg, score.numpy(), rtol=2e-5, atol=1e-6)
    for (k, ref), gr in zip(grads.items(), gg):
        ref = ref.numpy()
        np.testing.assert_allclose(gr, ref, rtol=rtol, atol=2e-5 * np.abs(ref).max(), err_msg=f"F={F} {k}")


def _lists(n, m, t, rng, overlap=False):
    perm = rng.permutation(n)
    tr = perm[:m]
    te = perm[m:m + t] if not overlap else rng.permutation(n)[:t]
    return tr, te


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("F", [10, 25, 64, 93, "bound"])
def test_fused_vs_float64_and_wide_at_every_tile_branch(F):
    from ggad_amd.model_dominant import ae_rows, fused_supported
    F = _bound() if F == "bound" else F
    assert fused_supported(F, H)
    n = 16 * 16 * 300 + 50                                   # enough rows for > 256 tiles: many tiles per workgroup
    fa = _graph(n)
    rng = np.random.default_rng(F)
    x = torch.from_numpy(rng.random((n, F), dtype=np.float32)).to(DEV)
    ps = _params(F, H, F)
    cases = [(1, 0), (TILE - 1, 1), (TILE, TILE - 1), (TILE + 1, TILE + 1), (16 * 16 * 200 + 7, 16 * 16 * 60 + 3)]
    for k, (m, t) in enumerate(cases):
        tr, te = _lists(n, m, t, rng, overlap=(k == 3))
        rs = ae_rows(fa, tr, te)
        got = _run(_fused, ps, x, rs)
        _check64(F, ps, x, tr, te, got)
        wide = _run(_wide, ps, x, rs)
        assert abs(got[0] - wide[0]) <= 2e-5 * abs(wide[0])
        np.testing.assert_allclose(got[1], wide[1], rtol=2e-5, atol=1e-6)
        for a, b in zip(got[2], wide[2]):
            np.testing.assert_allclose(a, b, rtol=2e-4, atol=2e-5 * np.abs(b).max())


def test_fused_is_bitwise_repeatable():
    from ggad_amd.model_dominant import ae_rows
    n, F = 60000, 93
    fa = _graph(n)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.random((n, F), dtype=np.float32)).to(DEV)
    ps = _params(F, H, 1)
    tr, te = _lists(n, 9000, 36000, rng)
    rs = ae_rows(fa, tr, te)
    a, b = _run(_fused, ps, x, rs), _run(_fused, ps, x, rs)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert all(np.array_equal(u, v) for u, v in zip(a[2], b[2]))


def test_wide_path_above_the_bound():
    from ggad_amd.model_dominant import ae_rows, fused_supported
    F = _bound() + 1
    assert not fused_supported(F, H)
    n = 3000
    fa = _graph(n)
    rng = np.random.default_rng(9)
    x = torch.from_numpy(rng.random((n, F), dtype=np.float32)).to(DEV)
    ps = _params(F, H, 2)
    tr, te = _lists(n, 500, 1800, rng)
    rs = ae_rows(fa, tr, te)
    _check64(F, ps, x, tr, te, _run(_wide, ps, x, rs))
    with pytest.raises(ValueError, match="does not hold"):
        _fused(*ps, x, rs)


def test_row_list_refusals():
    from ggad_amd.model_dominant import ae_rows
    fa = _graph(100)
    with pytest.raises(ValueError, match="twice"):
        ae_rows(fa, [1, 2, 1], [3])
    with pytest.raises(ValueError, match="at least one"):
        ae_rows(fa, [], [3])
    assert ae_rows(fa, [1, 2], [2, 1])["t"] == 2                # the two lists may overlap


# ------------------------------------------------------------------------------------------------ the model against the fixtures
def _case(g, tag):
    return {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + ".")}


def _setup(c):
    from ggad_amd import synth
    from ggad_amd.fullgraph import FullGraphAdj
    from ggad_amd.model_dominant import Model
    from ggad_amd.utils import normalize_adj
    n = int(c["n"])
    adj = synth.csr_to_scipy(c["rowptr"], c["col"], n)
    full = FullGraphAdj(normalize_adj(adj) + sp.eye(n), adj + sp.eye(n), DEV)
    torch.manual_seed(int(c["seed"]))
    model = Model(int(c["f"]), int(c["n_h"]), "prelu", 1, "avg").to(DEV)
    x = torch.from_numpy(c["features"]).float().to(DEV)[None]
    return full, model, x


def _cmp_trained(model, c, prefix, rtol, atol):
    for k, v in model.state_dict().items():
        ref = c.get(prefix + k)
        if ref is None:
            ref = c["init." + k]                                  # never trained: bit-equal to the initial state
            assert np.array_equal(v.cpu().numpy(), ref), (prefix, k)
            continue
        np.testing.assert_allclose(v.cpu().numpy(), ref, rtol=rtol, atol=atol * np.abs(ref).max(), err_msg=prefix + k)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_model_matches_fixture(tag):
    from ggad_amd.fullgraph import FlatAdam
    from ggad_amd.model_dominant import fused_supported
    c = _case(load_golden("fullgraph_dominant.npz"), tag)
    assert fused_supported(int(c["f"]), int(c["n_h"])) == (tag == "a")
    lr = float(c["lr"])
    idx_train, idx_test = list(c["idx_train"]), c["idx_test"]
    full, model, x = _setup(c)
    opt = FlatAdam(model.parameters(), lr=lr)
    loss, score = model(x, full, idx_train, idx_test)
    loss.backward()
    np.testing.assert_allclose(model.emb.cpu().numpy(), c["emb"], rtol=1e-4, atol=1e-5 * np.abs(c["emb"]).max())
    assert abs(loss.item() - float(c["loss0"])) <= 2e-5 * abs(float(c["loss0"]))
    np.testing.assert_allclose(score.cpu().numpy(), c["score0"], rtol=1e-4, atol=1e-5)
    for k, p in model.named_parameters():
        ref = c.get("grad." + k)
        if ref is None:
            assert p.grad is None, k
            continue
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=1e-3, atol=1e-5 * np.abs(ref).max(), err_msg=k)
    assert sum(p.grad is not None for p in model.parameters()) == 4
    opt.step()
    _cmp_trained(model, c, "step1.", 1e-4, 1e-5)
    full, model, x = _setup(c)
    opt = FlatAdam(model.parameters(), lr=lr)
    losses = []
    for epoch in range(5):
        model.train()
        opt.zero_grad()
        loss, score = model(x, full, idx_train, idx_test)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        np.testing.assert_allclose(score.cpu().numpy(), c["traj_score"][epoch], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(losses, c["traj_loss"], rtol=2e-5)
    _cmp_trained(model, c, "final.", 1e-3, 1e-4)
    assert model.emb_computations == 1


def test_planted_auroc_ap_at_every_print_epoch():
    from ggad_amd.fullgraph import FlatAdam
    from ggad_amd.metrics import average_precision, roc_auc
    c = load_golden("fullgraph_dominant_planted.npz")
    full, model, x = _setup(c)
    opt = FlatAdam(model.parameters(), lr=float(c["lr"]))
    idx_train, idx_test = list(c["idx_train"]), c["idx_test"]
    yt = torch.as_tensor(c["ano"][idx_test].astype(np.int64), device=DEV)
    aucs, aps = [], []
    for epoch in range(int(c["num_epoch"])):
        model.train()
        opt.zero_grad()
        loss, score = model(x, full, idx_train, idx_test)
        loss.backward()
        opt.step()
        if epoch % 5 == 0:
            aucs.append(roc_auc(score.view(-1), yt))
            aps.append(average_precision(score.view(-1), yt))
    assert np.all(np.abs(np.array(aucs) - c["auc"]) <= 1e-4), (aucs, c["auc"])
    assert np.all(np.abs(np.array(aps) - c["ap"]) <= 1e-4), (aps, c["ap"])


def test_emb_cache_follows_the_gcn_parameters():
    c = _case(load_golden("fullgraph_dominant.npz"), "a")
    full, model, x = _setup(c)
    idx_train, idx_test = list(c["idx_train"]), c["idx_test"]
    model(x, full, idx_train, idx_test)
    e0 = model.emb.clone()
    model(x, full, idx_train, idx_test)
    assert model.emb_computations == 1 and torch.equal(model.emb, e0)
    with torch.no_grad():
        model.dense_stru.weight.mul_(1.5)
    model(x, full, idx_train, idx_test)
    assert model.emb_computations == 2 and not torch.equal(model.emb, e0)
    model(x, full, idx_train, idx_test)
    assert model.emb_computations == 2


# ------------------------------------------------------------------------------------------------ published sizes
@pytest.mark.parametrize("dataset", ["reddit", "Amazon", "photo", "t_finance", "elliptic"])
def test_one_epoch_at_published_size_vs_float64(dataset):
    from ggad_amd import synth
    from ggad_amd.fullgraph import FullGraphAdj
    from ggad_amd.model_dominant import Model
    from ggad_amd.utils import normalize_adj, preprocess_features
    from run import SIZES
    n, ne, f, rate = SIZES[dataset]
    rowptr, col = synth.make_graph(n, min(ne, 400000), 0, kind="powerlaw", max_degree=max(64, n // 8), exact=True)
    adj = synth.csr_to_scipy(rowptr, col, n)
    feats = np.asarray(preprocess_features(sp.lil_matrix(synth.make_features(n, f, 0))), dtype=np.float32)
    rng = np.random.default_rng(1)
    perm = rng.permutation(n)
    tr, te = perm[:int(0.15 * n)], perm[int(0.4 * n):]
    full = FullGraphAdj(normalize_adj(adj) + sp.eye(n), adj + sp.eye(n), DEV)
    torch.manual_seed(0)
    model = Model(f, 300, "prelu", 1, "avg").to(DEV)
    P = R.params64({k: v.cpu().numpy() for k, v in model.state_dict().items()})
    x = torch.from_numpy(feats).to(DEV)
    loss, score = model(x, full, tr, te)
    loss.backward()
    ref_loss, ref_score, grads = R.ae_grads(P, torch.from_numpy(feats).double(), tr, te)
    assert abs(loss.item() - ref_loss.item()) <= 1e-4 * abs(ref_loss.item())
    np.testing.assert_allclose(score.cpu().numpy(), ref_score.numpy(), rtol=1e-4, atol=1e-6)
    pd = dict(model.named_parameters())
    for k, ref in grads.items():
        ref = ref.numpy()
        np.testing.assert_allclose(pd[k].grad.cpu().numpy(), ref, rtol=5e-3, atol=2e-4 * np.abs(ref).max(), err_msg=f"{dataset} {k}")
    assert model.emb.shape == (n, f) and torch.isfinite(model.emb).all()


# ------------------------------------------------------------------------------------------------ the script
def _script_lines(extra):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "dominant.py"), "--dataset", "reddit", "--synthetic",
           "--num_epoch", "12", "--quiet"] + extra
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    keep = [ln for ln in r.stdout.splitlines() if not ln.startswith(("training epoch captured", "median epoch"))]
    return keep, r.stdout


def test_script_captured_equals_eager():
    graph, raw_g = _script_lines([])
    eager, _ = _script_lines(["--no_graph"])
    assert "training epoch captured as a hipGraph" in raw_g
    assert graph == eager
    assert sum(ln.startswith("Epoch:") and "train_loss=" in ln for ln in graph) == 6
    assert sum(ln.startswith("Testing reddit AUC:") for ln in graph) == 3
