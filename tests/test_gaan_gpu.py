"""GPU tests of the full-graph GAAN path (csrc/gaan.hip through `ggad_amd.model_gaan`): the edge loss against float64 at every branch
of its kernels, the model against the fixtures captured from the imported reference (tests/golden/make_golden_gaan.py), AUROC / AP on
a planted schedule, one step at each published size against the float64 restatement (tests/gaan_fp64.py), and the script's captured
epoch against its eager one."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gaan_fp64 as R
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C = 64


def _lib():
    from ggad_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------ the edge loss against float64
def _pattern(kind):
    """(A_hat-like CSR with stored zeros / negatives, row list): rows of degree 1, 63, 64, 65, thousands; an empty row, a row holding
    only its diagonal, hub columns; asymmetric; the row list a proper subset in shuffled order."""
    rng = np.random.default_rng(7)
    n = 9000
    rows, cols = [], []
    degs = {0: 1, 1: 63, 2: 64, 3: 65, 4: 2999, 5: 5000, 6: 8200}
    for i in range(n):
        if i == 7:                                             # empty row (isolated, no diagonal stored)
            continue
        if i == 8:                                             # diagonal only
            rows.append(i)
            cols.append(i)
            continue
        k = degs.get(i, int(rng.integers(1, 40)))
        c = rng.choice(n, k, replace=False)
        rows += [i] * k
        cols += list(c)
    hub = rng.choice(np.arange(11, n), 4000, replace=False)    # column 9 in 4000 rows, column 10 in 70: big column sides
    rows += list(hub) + list(hub[:70])
    cols += [9] * 4000 + [10] * 70
    a = sp.csr_matrix((rng.uniform(0.05, 1.0, len(rows)), (rows, cols)), shape=(n, n))
    a.sum_duplicates()
    a.sort_indices()
    z = rng.random(a.nnz)
    z[: a.indptr[9]] = 1.0                                     # (rows 0..8 keep their degrees)
    a.data[z < 0.03] = 0.0                                     # stored zeros
    a.data[(z >= 0.03) & (z < 0.05)] *= -1.0                   # stored negatives
    a.data[a.indptr[8]] = 1.0
    idx = rng.permutation(n)
    if kind == "subset":                                       # the special rows 0..10 first, then 60 % of the others, shuffled
        rest = idx[idx > 10]
        idx = np.concatenate([np.arange(11), rest[: int(0.6 * n)]])
    return a, idx


def _emb(n, rng, scale, saturate=False):
    emb = (rng.standard_normal((n, C)) * scale).astype(np.float32)
    if saturate:
        # four classes of rows along one direction: dots 36 and 256 (> 20: a = 1), -96 (< -90: a = 0) and -39.7 (a below 1e-12:
        # the floor of the BCE backward)
        v = np.ones(C, dtype=np.float32) / np.sqrt(C)
        k = np.arange(n) % 9
        emb[k == 0], emb[k == 1], emb[k == 2], emb[k == 3] = 6 * v, -16 * v, 6.3 * v, -6.3 * v
    return emb


@pytest.mark.parametrize("kind", ["all", "subset", "saturated"])
def test_edge_loss_vs_float64_at_every_branch(kind):
    from ggad_amd.fullgraph import FullGraphAdj
    from ggad_amd.model_gaan import EdgeLossFn, edge_list, edge_structs
    a, idx = _pattern("subset" if kind == "subset" else "all")
    n = a.shape[0]
    fa = FullGraphAdj(a, a, DEV)
    es = edge_structs(fa, idx)
    lim = int(_lib().load().ggad_gaan_bwd_small_count())
    assert es["n_big"] > 0 and es["n_small"] > 0 and es["n_small"] + es["n_big"] == n
    erow, ecol, cnt = edge_list(a, idx)
    assert es["m"] == len(erow) and (a.data <= 0).sum() > 0
    counts = np.bincount(np.concatenate([erow, ecol]), minlength=n)
    assert (counts <= lim).any() and (counts > lim).any() and counts.max() > 4000
    rowdeg = np.zeros(n, dtype=np.int64)
    rowdeg[idx] = cnt
    assert rowdeg[:9].tolist() == [1, 63, 64, 65, 2999, 5000, 8200, 0, 1]
    rng = np.random.default_rng(11)
    emb = _emb(n, rng, 0.25, saturate=(kind == "saturated"))
    z = _emb(n, rng, 0.6, saturate=(kind == "saturated"))
    g = 1.7
    loss, lf, lr, dE = R.edge_loss_ref(emb, z, erow, ecol, g=g)
    if kind == "saturated":
        d = np.einsum("ij,ij->i", emb[erow].astype(np.float64), emb[ecol])
        assert (d > 20).any() and (d < -90).any() and ((d < -30) & (d > -80)).any() and (d > 200).any()
    outs = []
    for _ in range(2):
        e = torch.from_numpy(emb).to(DEV).requires_grad_(True)
        zz = torch.from_numpy(z).to(DEV)
        l, parts = EdgeLossFn.apply(e, zz, es)
        (g * l).backward()
        outs.append((l.item(), parts.cpu().numpy(), e.grad.cpu().numpy()))
    (l0, p0, d0), (l1, p1, d1) = outs
    assert l0 == l1 and np.array_equal(p0, p1) and np.array_equal(d0, d1)          # bit for bit
    assert abs(l0 - loss) <= 2e-5 * abs(loss)
    assert abs(p0[0] - lf) <= 2e-5 * abs(lf) and abs(p0[1] - lr) <= 2e-5 * abs(lr)
    np.testing.assert_allclose(d0, dE, rtol=1e-4, atol=1e-5 * np.abs(dE).max())
    untouched = counts == 0
    assert np.all(d0[untouched] == 0)


def test_edge_loss_refusals():
    from ggad_amd.fullgraph import FullGraphAdj
    from ggad_amd.model_gaan import EdgeLossFn, edge_structs
    n = 50
    a = sp.csr_matrix(sp.eye(n) + sp.random(n, n, 0.1, random_state=1))
    fa = FullGraphAdj(a, a, DEV)
    with pytest.raises(ValueError, match="twice"):
        edge_structs(fa, [1, 2, 3, 2])
    es = edge_structs(fa, np.arange(n))
    with pytest.raises(ValueError, match="channels"):
        EdgeLossFn.apply(torch.randn(n, 32, device=DEV), torch.randn(n, 32, device=DEV), es)
    assert int(_lib().load().ggad_gaan_edge_channels()) == C


# ------------------------------------------------------------------------------------------------ the model against the fixtures
def _case(g, tag):
    return {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + ".")}


def _setup(c):
    from ggad_amd import synth
    from ggad_amd.fullgraph import FullGraphAdj
    from ggad_amd.model_gaan import Model
    from ggad_amd.utils import normalize_adj
    n = int(c["n"])
    adj = synth.csr_to_scipy(c["rowptr"], c["col"], n)
    full = FullGraphAdj(normalize_adj(adj) + sp.eye(n), adj + sp.eye(n), DEV)
    torch.manual_seed(int(c["seed"]))
    model = Model(int(c["f"]), int(c["n_h"]), "prelu", 1, "avg").to(DEV)
    x = torch.from_numpy(c["features"]).float().to(DEV)[None]
    return full, model, x


def _cmp_state(model, c, prefix, rtol, atol, what, bias_steps=0, lr_atol=0.0):
    """state_dict against the fixture; the biases in front of a batch norm (and the running means that carry them) move by Adam
    steps on a round-off gradient: held to 2 lr per step (see test_aegis_gpu.py)."""
    lr = float(c["lr"])
    for k, v in model.state_dict().items():
        ref = c.get(prefix + k)
        if ref is None:
            continue
        got = v.cpu().numpy()
        if k.endswith(("lins.0.bias", "running_mean")) and bias_steps:
            assert np.abs(got - ref).max() <= 2 * lr * bias_steps, (what, k)
            continue
        if got.dtype.kind == "i":
            assert np.array_equal(got, ref), (what, k)
        else:
            np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol * (np.abs(ref).max() + 1e-3) + lr_atol * lr, err_msg=f"{what} {k}")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_model_matches_fixture(tag):
    from ggad_amd.fullgraph import FlatAdam
    g = load_golden("fullgraph_gaan.npz")
    c = _case(g, tag)
    lr = float(c["lr"])
    idx_train, idx_test = list(c["idx_train"]), c["idx_test"]
    # (1) one epoch from the initial state
    full, model, x = _setup(c)
    _cmp_state(model, c, "init.", 0, 0, "init")
    opt = FlatAdam(model.parameters(), lr=lr)
    opt_gen = FlatAdam(model.generator.parameters(), lr=lr)
    loss, loss_g, score, parts, x_, z = model.train_forward(x, full, idx_train, idx_test)
    torch.autograd.backward([loss, loss_g])
    for k, v in (("x_", x_), ("emb", model.emb), ("z_", z)):
        np.testing.assert_allclose(v.detach().cpu().numpy(), c[k], rtol=1e-4, atol=2e-5 * np.abs(c[k]).max(), err_msg=k)
    from ggad_amd.model_gaan import edge_structs
    assert edge_structs(full, idx_train)["m"] == int(c["m"])
    for name, got in (("loss0", loss.item()), ("loss_f0", parts[0].item()), ("loss_r0", parts[1].item()), ("loss_g0", loss_g.item())):
        assert abs(got - float(c[name])) < 2e-5 * abs(float(c[name])), (name, got, float(c[name]))
    np.testing.assert_allclose(score.cpu().numpy(), c["score0"], rtol=1e-4, atol=1e-5)
    for k, p in model.named_parameters():
        ref = c.get("grad." + k)
        if ref is None:
            assert p.grad is None, k
            continue
        got = p.grad.cpu().numpy().reshape(ref.shape)
        if k.endswith("lins.0.bias"):                       # in front of batch norm: zero up to round-off on both sides
            wscale = np.abs(c["grad." + k.replace(".bias", ".weight")]).max()
            assert np.abs(got).max() < 1e-3 * wscale, k
            continue
        np.testing.assert_allclose(got, ref, rtol=2e-3, atol=1e-4 * (np.abs(ref).max() + 1e-6), err_msg="grad " + k)
    opt.step()
    opt_gen.step()
    _cmp_state(model, c, "step1.", 1e-4, 1e-5, "step1", bias_steps=2)           # (the generator is stepped twice)
    # (2) the script's loop, 5 epochs: losses, scores, BN buffers every epoch, the weights at the end
    full, model, x = _setup(c)
    opt = FlatAdam(model.parameters(), lr=lr)
    opt_gen = FlatAdam(model.generator.parameters(), lr=lr)
    losses, losses_g = [], []
    for epoch in range(5):
        model.train()
        opt.zero_grad()
        opt_gen.zero_grad()
        loss, loss_g, score = model(x, full, idx_train, idx_test)
        torch.autograd.backward([loss, loss_g])
        opt.step()
        opt_gen.step()
        losses.append(loss.item())
        losses_g.append(loss_g.item())
        np.testing.assert_allclose(score.cpu().numpy(), c["traj_score"][epoch], rtol=2e-4, atol=2e-5)
        sd = model.state_dict()
        for k in [k for k in c if k.startswith("traj_buf.")]:
            name = k[len("traj_buf."):]
            ref = c[k][epoch]
            got = sd[name].cpu().numpy()
            if got.dtype.kind == "i":
                assert np.array_equal(got, ref), (epoch, name)
            elif name.endswith("running_mean"):              # carries the round-off-driven lins.0.bias (see _cmp_state)
                assert np.abs(got - ref).max() <= 4 * lr * (epoch + 1) + 1e-4 * np.abs(ref).max(), (epoch, name)
            else:
                np.testing.assert_allclose(got, ref, rtol=1e-3, atol=1e-5 * np.abs(ref).max(), err_msg=f"{epoch} {name}")
    np.testing.assert_allclose(losses, c["traj_loss"], rtol=2e-4)
    np.testing.assert_allclose(losses_g, c["traj_loss_g"], rtol=2e-4)
    assert int(model.discriminator.norms[0].module.num_batches_tracked) == 10
    _cmp_state(model, c, "final.", 1e-3, 1e-4, "final", bias_steps=10, lr_atol=0.25)


def test_eval_mode_raises():
    c = _case(load_golden("fullgraph_gaan.npz"), "a")
    full, model, x = _setup(c)
    model.eval()
    with pytest.raises(ValueError, match="training mode"):
        model(x, full, list(c["idx_train"]), c["idx_test"])


def test_planted_auroc_ap_at_every_print_epoch():
    from ggad_amd.fullgraph import FlatAdam
    from ggad_amd.metrics import average_precision, roc_auc
    c = load_golden("fullgraph_gaan_planted.npz")
    full, model, x = _setup(c)
    lr = float(c["lr"])
    all_idx, idx_test = list(c["all_idx"]), c["idx_test"]
    opt = FlatAdam(model.parameters(), lr=lr)
    opt_gen = FlatAdam(model.generator.parameters(), lr=lr)
    yt = torch.as_tensor(c["ano"][idx_test].astype(np.int64), device=DEV)
    aucs, aps = [], []
    for epoch in range(int(c["num_epoch"])):
        model.train()
        opt.zero_grad()
        opt_gen.zero_grad()
        loss, loss_g, score = model(x, full, all_idx, idx_test)
        torch.autograd.backward([loss, loss_g])
        opt.step()
        opt_gen.step()
        if epoch % 5 == 0:
            aucs.append(roc_auc(score.view(-1), yt))
            aps.append(average_precision(score.view(-1), yt))
            model.eval()
    # 1e-4, or 3 x the reference's own movement under a 1e-7 relative change of its initial weights where that is larger
    tol_auc = max(1e-4, 3 * float(np.max(c["self_sens_auc"])))
    tol_ap = max(1e-4, 3 * float(np.max(c["self_sens_ap"])))
    assert np.all(np.abs(np.array(aucs) - c["auc"]) <= tol_auc), (aucs, c["auc"])
    assert np.all(np.abs(np.array(aps) - c["ap"]) <= tol_ap), (aps, c["ap"])


# ------------------------------------------------------------------------------------------------ published sizes
@pytest.mark.parametrize("dataset", ["reddit", "Amazon", "photo", "t_finance", "elliptic"])
def test_one_step_at_published_size_vs_float64(dataset):
    """Both losses, the test scores, every gradient and the weights after both Adam steps at the published size (synthetic graph),
    against the sparse float64 restatement."""
    from ggad_amd import synth
    from ggad_amd.fullgraph import FlatAdam, FullGraphAdj
    from ggad_amd.model_gaan import Model, edge_structs
    from ggad_amd.utils import normalize_adj, preprocess_features
    from run import SIZES
    n, ne, f, rate = SIZES[dataset]
    rowptr, col = synth.make_graph(n, ne, 0, kind="powerlaw", max_degree=max(64, n // 8), exact=True)
    adj = synth.csr_to_scipy(rowptr, col, n)
    feats = np.asarray(preprocess_features(sp.lil_matrix(synth.make_features(n, f, 0))), dtype=np.float32)
    rng = np.random.default_rng(1)
    all_idx = rng.permutation(n)
    idx_test = all_idx[int(0.4 * n):]
    full = FullGraphAdj(normalize_adj(adj) + sp.eye(n), adj + sp.eye(n), DEV)
    torch.manual_seed(0)
    model = Model(f, 300, "prelu", 1, "avg").to(DEV)
    P = R.params64({k: v.cpu().numpy() for k, v in model.state_dict().items()})
    noise = torch.randn(n, 16)
    model.noise_override = noise.to(DEV)
    opt = FlatAdam(model.parameters(), lr=1e-3)
    opt_gen = FlatAdam(model.generator.parameters(), lr=1e-3)
    x = torch.from_numpy(feats).to(DEV)
    loss, loss_g, score, parts, _, _ = model.train_forward(x, full, all_idx, idx_test)
    torch.autograd.backward([loss, loss_g])
    es = edge_structs(full, all_idx)
    erow, ecol = es["erow"].cpu().numpy(), es["ecol"].cpu().numpy()
    out = R.forward(P, torch.from_numpy(feats).double(), noise.double(), erow, ecol, all_idx, idx_test)
    for name, got in (("loss", loss.item()), ("loss_f", parts[0].item()), ("loss_r", parts[1].item()), ("loss_g", loss_g.item())):
        assert abs(got - out[name].item()) < 1e-4 * abs(out[name].item()), (dataset, name, got, out[name].item())
    np.testing.assert_allclose(score.cpu().numpy(), out["score"].detach().numpy(), rtol=1e-4, atol=1e-5)
    names = [k for k, p in model.named_parameters() if p.grad is not None]
    grads = torch.autograd.grad(out["loss"] + out["loss_g"], [P[k] for k in names])
    pd = dict(model.named_parameters())
    for k, gr in zip(names, grads):
        ref = gr.numpy()
        got = pd[k].grad.cpu().numpy().reshape(ref.shape)
        if k.endswith("lins.0.bias"):
            wscale = np.abs(pd[k.replace(".bias", ".weight")].grad.cpu().numpy()).max()
            assert np.abs(got).max() < 5e-3 * wscale and np.abs(ref).max() < 1e-9 * wscale, k      # (N rows of round-off)
            continue
        np.testing.assert_allclose(got, ref, rtol=5e-3, atol=2e-4 * (np.abs(ref).max() + 1e-9), err_msg=f"{dataset} grad {k}")
    # the weights after optimiser + optimiser_gen: float64 Adam (two instances) from the gradients just checked
    before = {k: v.detach().cpu().double() for k, v in pd.items()}
    ours = {k: pd[k].grad.detach().cpu().double() for k in names}
    opt.step()
    opt_gen.step()
    P2 = {k: before[k].clone().requires_grad_(True) for k in names}
    for k, p in P2.items():
        p.grad = ours[k].clone()
    torch.optim.Adam(list(P2.values()), lr=1e-3).step()
    torch.optim.Adam([P2[k] for k in names if k.startswith("generator.")], lr=1e-3).step()
    for k in names:
        got = pd[k].detach().cpu().numpy()
        ref = P2[k].detach().numpy().reshape(got.shape)
        step = np.abs(ref - before[k].numpy().reshape(got.shape)).max()
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6 * np.abs(ref).max() + 1e-3 * step + 1e-8, err_msg=f"{dataset} weight {k}")
    run = R.running_after(P, out["stats"])
    for k, v in run.items():
        np.testing.assert_allclose(model.state_dict()[k].cpu().numpy(), v.numpy(), rtol=1e-4, atol=1e-6, err_msg=k)


# ------------------------------------------------------------------------------------------------ the script
def _script_lines(extra):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "gaan.py"), "--dataset", "Amazon", "--synthetic",
           "--num_epoch", "22", "--quiet"] + extra
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    keep = [ln for ln in r.stdout.splitlines() if not ln.startswith(("training epoch captured", "median epoch"))]
    return keep, r.stdout


def test_script_captured_equals_eager():
    graph, raw_g = _script_lines([])
    eager, _ = _script_lines(["--no_graph"])
    assert "training epoch captured as a hipGraph" in raw_g
    assert graph == eager
    assert sum(ln.startswith("Epoch:") and "train_loss=" in ln for ln in graph) == 5
    assert sum(ln.startswith("Testing Amazon AUC:") for ln in graph) == 5
