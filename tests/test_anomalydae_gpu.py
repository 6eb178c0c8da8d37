"""GPU tests of the full-graph AnomalyDAE path (csrc/anomalydae.hip through `ggad_amd.gat` / `ggad_amd.model_anomalydae`): the GAT
layer and the fused reconstruction loss against float64 dense formulations, the model against the fixtures captured from the
imported reference, and the script's captured epoch against its eager one."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from ggad_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _full(a_norm, raw=None):
    import scipy.sparse as sp
    from ggad_amd.fullgraph import FullGraphAdj
    a = sp.csr_matrix(a_norm)
    return FullGraphAdj(a, a if raw is None else raw, DEV)


def _rand_adj(n, seed, density=0.05, symmetric=False):
    """Weighted adjacency (A_hat-like, positive entries) with raw self loops on every third node, an isolated node (n - 1) and a
    node (n - 2) whose only entry is its self loop."""
    rng = np.random.default_rng(seed)
    a = (rng.random((n, n)) < density) * (0.05 + rng.random((n, n)))
    if symmetric:
        a = np.triu(a, 1)
        a = a + a.T
    a[np.arange(0, n, 3), np.arange(0, n, 3)] = 0.9
    a[n - 1, :] = 0
    a[:, n - 1] = 0
    a[n - 2, :] = 0
    a[:, n - 2] = 0
    a[n - 2, n - 2] = 1.1
    return a


def _dense_gat64(h, w, a_s, a_d, b, adj):
    y = h @ w.T
    als, ald = y @ a_s.reshape(-1), y @ a_d.reshape(-1)
    n = y.shape[0]
    eye = torch.eye(n, dtype=torch.bool)
    mask = ((adj > 0) & ~eye) | eye                               # mask[r, i]: edge source r -> target i
    e = torch.nn.functional.leaky_relu(als[:, None] + ald[None, :], 0.2).masked_fill(~mask, -math.inf)
    return torch.softmax(e, dim=0).T @ y + b


@pytest.mark.parametrize("f", [10, 25, 64, 93, 745])
@pytest.mark.parametrize("symmetric", [False, True])
def test_gat_forward_backward_vs_float64(f, symmetric):
    from ggad_amd.gat import GATConv
    n, hd = 203, 40
    a = _rand_adj(n, f + symmetric, symmetric=symmetric)
    fa = _full(a)
    torch.manual_seed(f)
    conv = GATConv(hd, f)
    conv.bias.data.normal_()
    conv.to(DEV)
    rng = np.random.default_rng(f)
    h = torch.from_numpy(rng.standard_normal((n, hd)).astype(np.float32))
    g = torch.from_numpy(rng.standard_normal((n, f)).astype(np.float32))
    hd_ = h.to(DEV).requires_grad_(True)
    z = conv(hd_, fa)
    z.backward(g.to(DEV))
    h64 = h.double().requires_grad_(True)
    ps = [p.detach().cpu().double().requires_grad_(True) for p in (conv.lin_src.weight, conv.att_src, conv.att_dst, conv.bias)]
    ref = _dense_gat64(h64, *ps, torch.from_numpy(a))
    ref.backward(g.double())
    np.testing.assert_allclose(z.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=2e-5)
    got = [hd_.grad, conv.lin_src.weight.grad, conv.att_src.grad, conv.att_dst.grad, conv.bias.grad]
    for name, a_, b_ in zip(["h", "W", "att_src", "att_dst", "bias"], got, [h64.grad] + [p.grad for p in ps]):
        b_ = b_.numpy()
        np.testing.assert_allclose(a_.cpu().numpy(), b_, rtol=2e-4, atol=2e-5 * (np.abs(b_).max() + 1), err_msg=name)


@pytest.mark.parametrize("n_rows", [1, 15, 17, 70])
@pytest.mark.parametrize("n,f,scale", [(203, 10, 0.4), (301, 93, 0.15), (130, 745, 0.05), (97, 25, 3.0)])
def test_recon_loss_forward_backward_vs_float64(n_rows, n, f, scale):
    """loss / score / d loss / dz / d loss / dx_hat against float64 autograd on the materialised matrix; |R| about a 16-row tile,
    N and F off the tile multiples, a row with only its self loop (n - 2) and an isolated one (n - 1) among the rows, and
    saturated sigmoids (scale 3: |z_i . z_j| well above 30)."""
    from ggad_amd.model_anomalydae import recon_loss, recon_score
    rng = np.random.default_rng(n + f + n_rows)
    a = _rand_adj(n, n_rows)
    fa = _full(a)
    rows = np.concatenate([[n - 2, n - 1], rng.permutation(n - 2)])[:n_rows].astype(np.int64)
    z = rng.standard_normal((n, f)).astype(np.float32) * scale
    x = rng.random((n, f)).astype(np.float32)
    xh = rng.standard_normal((n, f)).astype(np.float32)
    zd = torch.from_numpy(z).to(DEV).requires_grad_(True)
    xhd = torch.from_numpy(xh).to(DEV).requires_grad_(True)
    loss, score = recon_loss(zd, xhd, torch.from_numpy(x).to(DEV), fa, rows)
    (2.5 * loss).backward()
    z64 = torch.from_numpy(z).double().requires_grad_(True)
    xh64 = torch.from_numpy(xh).double().requires_grad_(True)
    A = torch.from_numpy(a)
    r = torch.from_numpy(rows)
    s_ = torch.sigmoid(z64 @ z64.T)
    attr = torch.sqrt(torch.sum((torch.from_numpy(x).double()[r] - xh64[r]) ** 2, 1))
    stru = torch.sqrt(torch.sum((A[r] - s_[r]) ** 2, 1))
    sc = 0.5 * attr + 0.5 * stru
    ref = sc.mean()
    (2.5 * ref).backward()
    assert abs(loss.item() - ref.item()) < 2e-6 * (1 + abs(ref.item()))
    np.testing.assert_allclose(score.cpu().numpy(), sc.detach().numpy(), rtol=2e-6, atol=2e-5)
    np.testing.assert_allclose(recon_score(zd.detach(), xhd.detach(), torch.from_numpy(x).to(DEV), fa, rows).cpu().numpy(),
                               score.cpu().numpy(), rtol=0, atol=0)
    gz = z64.grad.numpy()
    np.testing.assert_allclose(zd.grad.cpu().numpy(), gz, rtol=2e-4, atol=1e-5 * (np.abs(gz).max() + 1e-3))
    np.testing.assert_allclose(xhd.grad.cpu().numpy(), xh64.grad.numpy(), rtol=1e-5, atol=1e-8)


def test_recon_loss_refuses_duplicate_rows():
    from ggad_amd.model_anomalydae import recon_loss
    fa = _full(_rand_adj(50, 0))
    z = torch.zeros(50, 8, device=DEV)
    with pytest.raises(ValueError, match="twice"):
        recon_loss(z, z, z, fa, [3, 4, 3])


def _golden_adj(g, c):
    import scipy.sparse as sp
    from ggad_amd import utils as U
    from ggad_amd.fullgraph import FullGraphAdj
    n = int(g[f"{c}.n"])
    a = synth.csr_to_scipy(g[f"{c}.rowptr"], g[f"{c}.col"], n)
    return FullGraphAdj(U.normalize_adj(a) + sp.eye(n), a + sp.eye(n), DEV)


@pytest.mark.parametrize("case", ["a", "b"])
def test_model_against_reference_fixture(case):
    from ggad_amd.fullgraph import FlatAdam
    from ggad_amd.model_anomalydae import Model, recon_score
    g = load_golden("fullgraph_anomalydae.npz")
    c = case
    fa = _golden_adj(g, c)
    f, h = int(g[f"{c}.f"]), int(g[f"{c}.n_h"])
    torch.manual_seed(int(g[f"{c}.seed"]))
    model = Model(f, h, "prelu", 1, "avg")
    sd = {k[len(f"{c}.init."):]: v for k, v in g.items() if k.startswith(f"{c}.init.")}
    assert sorted(sd) == sorted(model.state_dict())
    for k, v in model.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), sd[k], err_msg=k)
    model.to(DEV)
    opt = FlatAdam(model.parameters(), lr=float(g[f"{c}.lr"]), weight_decay=0.0)
    feats = torch.from_numpy(g[f"{c}.features"])[None].to(DEV)
    nrm, tst = g[f"{c}.normal_idx"], g[f"{c}.idx_test"]
    for step in range(len(g[f"{c}.losses"])):
        model.train()
        opt.zero_grad()
        loss, score = model(feats, fa, nrm, tst)
        loss.backward()
        assert abs(loss.item() - g[f"{c}.losses"][step]) < 1e-5, step
        np.testing.assert_allclose(score.cpu().numpy(), g[f"{c}.scores"][step], atol=1e-5 * (1 + step))
        if step == 0:
            xhat, z = model.model_enc(feats[0], fa)
            np.testing.assert_allclose(z.detach().cpu().numpy(), g[f"{c}.z"], atol=3e-6)
            np.testing.assert_allclose(xhat.detach().cpu().numpy(), g[f"{c}.xhat"], atol=3e-6)
            np.testing.assert_allclose(score.cpu().numpy(), g[f"{c}.score_test0"], atol=1e-5)
            sc_tr = recon_score(z.detach(), xhat.detach(), feats[0], fa, nrm).cpu().numpy()
            np.testing.assert_allclose(sc_tr, 0.5 * g[f"{c}.attr"] + 0.5 * g[f"{c}.stru"], atol=1e-5)
            for k, p in model.named_parameters():
                if f"{c}.grad.{k}" in g:
                    np.testing.assert_allclose(p.grad.cpu().numpy(), g[f"{c}.grad.{k}"], atol=4e-6, rtol=2e-4, err_msg=k)
                else:
                    assert p.grad is None, k
        opt.step()
    for k, v in model.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), g[f"{c}.final.{k}"], atol=3e-5, err_msg=k)


def test_planted_schedule_auroc_ap():
    """The restated anomalyDAE.py loop on planted anomalies: AUROC / AP of the training-forward test scores at every evaluation."""
    from sklearn.metrics import average_precision_score, roc_auc_score
    from ggad_amd.fullgraph import FlatAdam
    from ggad_amd.model_anomalydae import Model
    g = load_golden("fullgraph_anomalydae_planted.npz")
    c = "p"
    fa = _golden_adj({f"{c}.{k}": v for k, v in g.items()}, c)
    torch.manual_seed(int(g["seed"]))
    model = Model(int(g["f"]), int(g["n_h"]), "prelu", 1, "avg").to(DEV)
    opt = FlatAdam(model.parameters(), lr=float(g["lr"]), weight_decay=0.0)
    feats = torch.from_numpy(g["features"])[None].to(DEV)
    yt = g["ano"][g["idx_test"]]
    aucs, aps = [], []
    for epoch in range(int(g["num_epoch"])):
        opt.zero_grad()
        loss, score = model(feats, fa, g["normal_idx"], g["idx_test"])
        loss.backward()
        opt.step()
        if epoch % 5 == 0:
            sc = score.cpu().numpy()
            aucs.append(roc_auc_score(yt, sc))
            aps.append(average_precision_score(yt, sc, average="macro", pos_label=1))
    assert np.abs(np.array(aucs) - g["auc"]).max() <= 1e-4, (aucs, g["auc"])
    assert np.abs(np.array(aps) - g["ap"]).max() <= 1e-4, (aps, g["ap"])


def test_script_captured_epoch_equals_eager():
    outs = []
    for extra in ([], ["--no_graph"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "anomalyDAE.py"), "--dataset", "reddit", "--synthetic", "--num_epoch", "12",
                            "--quiet"] + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        keep = [l for l in r.stdout.splitlines() if l.startswith("Epoch:") or l.startswith("Testing")]
        assert len(keep) == 6 + 3 * 2
        outs.append(keep)
        if not extra:
            assert "captured" in r.stdout
    assert outs[0] == outs[1]
