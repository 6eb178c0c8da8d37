"""GPU tests of the full-graph AEGIS path (csrc/aegis.hip through `ggad_amd.model_aegis`): the fused batch-norm heads and the losses
against float64, the model against the fixtures captured from the imported reference (tests/golden/make_golden_aegis.py), one step
at each published size against the float64 restatement (tests/aegis_fp64.py), and the script's captured epoch against its eager
one."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import aegis_fp64 as R
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _lib():
    from ggad_amd import _lib as L
    return L


def _bn_ref(h, g, b, act, w2=None, b2=None):
    mean = h.mean(0)
    var = h.var(0, unbiased=False)
    u = (h - mean) / torch.sqrt(var + 1e-5) * g + b
    y = torch.relu(u) if act == 0 else torch.sigmoid(u)
    if w2 is None:
        return y
    return torch.sigmoid(y @ w2 + b2)


RPG = 256         # rows per statistics workgroup below the 256-group saturation (ggad_aegis_bn_rows_per_group, checked below)


def _boundaries():
    rpg = RPG
    ms = {2, 3, 7535, 46564, 93128}
    for k in (1, 2, 37, 255, 256, 257):                 # group counts 1, 2, ..., the saturation at 256 groups
        for d in (-1, 0, 1):
            ms.add(k * rpg + d)
    return sorted(m for m in ms if m >= 2)


@pytest.mark.parametrize("m", _boundaries())
def test_bn_forward_backward_vs_float64(m):
    """Both activations, one and two row blocks, with and without the head; running statistics after two calls; every launch twice,
    bit for bit."""
    from ggad_amd.model_aegis import ACT_RELU, ACT_SIGMOID, BnActFn, BnHeadFn, bn_forward
    assert int(_lib().load().ggad_aegis_bn_rows_per_group()) == RPG
    rng = np.random.default_rng(m)
    C = 64
    h = torch.from_numpy((rng.standard_normal((m, C)) * rng.uniform(0.1, 3, C) + rng.uniform(-2, 2, C)).astype(np.float32))
    g = torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32))
    b = torch.from_numpy(rng.uniform(-0.5, 0.5, C).astype(np.float32))
    w2 = torch.from_numpy((rng.standard_normal(C) * 0.3).astype(np.float32))
    b2 = torch.from_numpy(np.array([0.1], dtype=np.float32))
    h64, g64, b64, w64 = h.double().requires_grad_(), g.double().requires_grad_(), b.double().requires_grad_(), w2.double().requires_grad_()
    b264 = b2.double().requires_grad_()
    for act in (ACT_RELU, ACT_SIGMOID):
        bn = nn.BatchNorm1d(C).to(DEV)
        bn.weight.data.copy_(g)
        bn.bias.data.copy_(b)
        hd = h.to(DEV).requires_grad_(True)
        gamma, beta = bn.weight, bn.bias
        # plain y (the generator's shape): forward, backward
        y = BnActFn.apply(hd, gamma, beta, bn, act)
        dy = torch.from_numpy(rng.standard_normal((m, C)).astype(np.float32))
        y.backward(dy.to(DEV))
        ref = _bn_ref(h64, g64, b64, act)
        gr = torch.autograd.grad(ref, [h64, g64, b64], dy.double())
        np.testing.assert_allclose(y.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=2e-5)
        for name, a_, r_ in zip(("dh", "dgamma", "dbeta"), (hd.grad, gamma.grad, beta.grad), gr):
            r_ = r_.numpy()
            np.testing.assert_allclose(a_.cpu().numpy(), r_, rtol=2e-4, atol=2e-5 * (np.abs(r_).max() + 1e-3) * max(1, m ** 0.5 / 30),
                                       err_msg=f"{name} act {act}")
        y2 = BnActFn.apply(hd.detach(), gamma, beta, bn, act)
        assert torch.equal(y.detach(), y2)
        # two calls -> running statistics, num_batches_tracked
        mean, var_u = h64.detach().mean(0), h64.detach().var(0, unbiased=True)
        rm = 0.9 * (0.9 * 0 + 0.1 * mean) + 0.1 * mean
        rv = 0.9 * (0.9 * 1 + 0.1 * var_u) + 0.1 * var_u
        np.testing.assert_allclose(bn.running_mean.cpu().numpy(), rm.numpy(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(bn.running_var.cpu().numpy(), rv.numpy(), rtol=1e-5, atol=1e-6)
        assert int(bn.num_batches_tracked) == 2
        # the head (discriminator2's shape): p, dh, dgamma, dbeta, dw2, db2
        gamma.grad = beta.grad = None
        hd2 = h.to(DEV).requires_grad_(True)
        w2d = w2.view(1, C).to(DEV).requires_grad_(True)
        b2d = b2.to(DEV).requires_grad_(True)
        p = BnHeadFn.apply(hd2, gamma, beta, w2d, b2d, bn, act)
        dp = torch.from_numpy(rng.standard_normal(m).astype(np.float32))
        p.backward(dp.to(DEV))
        pref = _bn_ref(h64, g64, b64, act, w64, b264)
        grs = torch.autograd.grad(pref, [h64, g64, b64, w64, b264], dp.double())
        np.testing.assert_allclose(p.detach().cpu().numpy(), pref.detach().numpy(), rtol=1e-5, atol=1e-6)
        for name, a_, r_ in zip(("dh", "dgamma", "dbeta", "dw2", "db2"), (hd2.grad, gamma.grad, beta.grad, w2d.grad.view(-1), b2d.grad), grs):
            r_ = r_.numpy()
            np.testing.assert_allclose(a_.cpu().numpy(), r_, rtol=2e-4, atol=2e-5 * (np.abs(r_).max() + 1e-3) * max(1, m ** 0.5 / 30),
                                       err_msg=f"head {name} act {act}")
        p2 = BnHeadFn.apply(hd2.detach(), gamma, beta, w2d.detach(), b2d.detach(), bn, act)
        assert torch.equal(p.detach(), p2)
        # two row blocks = their concatenation; the head on a row list
        if m >= 4:
            k = m // 3
            rows = torch.from_numpy(rng.permutation(m)[: max(1, m // 5)].astype(np.int64)).to(DEV)
            hdv = h.to(DEV)
            with torch.no_grad():
                p_two, mean2, inv2 = bn_forward(hdv[:k].contiguous(), hdv[k:].contiguous(), bn, act, rows=rows,
                                                head=(w2.to(DEV), b2.to(DEV)), update=False)
                p_one, mean1, inv1 = bn_forward(hdv, None, bn, act, rows=rows, head=(w2.to(DEV), b2.to(DEV)), update=False)
                y_two, _, _ = bn_forward(hdv[:k].contiguous(), hdv[k:].contiguous(), bn, act, update=False)
            np.testing.assert_allclose(mean2.cpu().numpy(), mean.numpy(), rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(p_two.cpu().numpy(), p_one.cpu().numpy(), rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(p_two.cpu().numpy(), pref.detach().numpy()[rows.cpu().numpy()], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(y_two.cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=2e-5)
            assert int(bn.num_batches_tracked) == 4          # update=False leaves the buffers alone


def test_bn_saturated_head_and_refusals():
    """A head saturated to p = 1: loss_g = 100 (the log clamp) and the gradient reaching h is 0, not NaN; M = 1 and C != 64 refused."""
    from ggad_amd.model_aegis import ACT_SIGMOID, BnHeadFn, aegis_losses, bn_forward, loss_rows
    from ggad_amd.fullgraph import FullGraphAdj
    import scipy.sparse as sp
    C, n = 64, 300
    bn = nn.BatchNorm1d(C).to(DEV)
    h = torch.randn(n, C, device=DEV).requires_grad_(True)
    w2 = torch.full((1, C), 40.0, device=DEV).requires_grad_(True)
    b2 = torch.tensor([30.0], device=DEV).requires_grad_(True)
    p = BnHeadFn.apply(h, bn.weight, bn.bias, w2, b2, bn, ACT_SIGMOID)
    assert torch.all(p == 1.0)
    fa = FullGraphAdj(sp.eye(n, format="csr"), sp.eye(n, format="csr"), DEV)
    x = torch.rand(n, 10, device=DEV)
    zd = torch.rand(n, 12, device=DEV).requires_grad_(True)
    lg, la = aegis_losses(p, zd, x, loss_rows(fa, np.arange(n)))
    torch.autograd.backward([lg, la])
    assert abs(lg.item() - 100.0) < 1e-4
    for t in (h.grad, w2.grad, b2.grad, bn.weight.grad, bn.bias.grad):
        assert torch.all(torch.isfinite(t)) and torch.all(t == 0)
    with pytest.raises(ValueError, match="more than 1 value"):
        bn_forward(torch.randn(1, C, device=DEV), None, bn, ACT_SIGMOID, head=(torch.ones(C, device=DEV), torch.zeros(1, device=DEV)))
    with pytest.raises(ValueError, match="channels"):
        bn_forward(torch.randn(50, 32, device=DEV), None, nn.BatchNorm1d(32).to(DEV), ACT_SIGMOID,
                   head=(torch.ones(32, device=DEV), torch.zeros(1, device=DEV)))


@pytest.mark.parametrize("n,f,nr", [(301, 10, 301), (293, 93, 57), (120, 745, 40)])
def test_losses_vs_float64(n, f, nr):
    from ggad_amd.fullgraph import FullGraphAdj
    from ggad_amd.model_aegis import aegis_losses, loss_rows
    import scipy.sparse as sp
    rng = np.random.default_rng(n + f)
    fp = (f + 3) // 4 * 4
    fa = FullGraphAdj(sp.eye(n, format="csr"), sp.eye(n, format="csr"), DEV)
    rows = rng.permutation(n)[:nr]
    p = rng.uniform(0.01, 0.99, n).astype(np.float32)
    p[:3] = [0.0, 1.0 - 1e-8, 0.5]
    x = rng.random((n, f)).astype(np.float32)
    zd = np.zeros((n, fp), dtype=np.float32)
    zd[:, :f] = rng.random((n, f))
    pd = torch.from_numpy(p).to(DEV).requires_grad_(True)
    zdd = torch.from_numpy(zd).to(DEV).requires_grad_(True)
    lg, la = aegis_losses(pd, zdd, torch.from_numpy(x).to(DEV), loss_rows(fa, rows))
    torch.autograd.backward([2.0 * lg, 3.0 * la])
    p64 = torch.from_numpy(p).double().requires_grad_(True)
    z64 = torch.from_numpy(zd).double().requires_grad_(True)
    lg64 = torch.nn.functional.binary_cross_entropy(p64, torch.zeros_like(p64))
    r = torch.from_numpy(rows)
    la64 = torch.mean(torch.sqrt(torch.sum((torch.from_numpy(x).double()[r] - z64[r, :f]) ** 2, 1)))
    torch.autograd.backward([2.0 * lg64, 3.0 * la64])
    assert abs(lg.item() - lg64.item()) < 1e-5 * abs(lg64.item())
    assert abs(la.item() - la64.item()) < 1e-5 * abs(la64.item())
    np.testing.assert_allclose(pd.grad.cpu().numpy(), p64.grad.numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(zdd.grad.cpu().numpy(), z64.grad.numpy(), rtol=1e-5, atol=1e-7)
    lg2, la2 = aegis_losses(pd.detach(), zdd.detach(), torch.from_numpy(x).to(DEV), loss_rows(fa, rows))
    assert lg2.item() == lg.item() and la2.item() == la.item()


# ------------------------------------------------------------------------------------------------ the model against the fixtures
def _case(g, tag):
    return {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + ".")}


def _setup(c):
    import scipy.sparse as sp
    from ggad_amd import synth
    from ggad_amd.fullgraph import FullGraphAdj
    from ggad_amd.model_aegis import Model
    from ggad_amd.utils import normalize_adj
    n = int(c["n"])
    adj = synth.csr_to_scipy(c["rowptr"], c["col"], n)
    full = FullGraphAdj(normalize_adj(adj) + sp.eye(n), adj + sp.eye(n), DEV)
    torch.manual_seed(int(c["seed"]))
    model = Model(int(c["f"]), int(c["n_h"]), "prelu", 1, "avg").to(DEV)
    x = torch.from_numpy(c["features"]).float().to(DEV)[None]
    return full, model, x


def _cmp_state(model, c, prefix, rtol, atol, what, bias_steps=0, lr_atol=0.0):
    """state_dict against the fixture.  The biases in front of a batch norm (lins.0.bias of both MLPs) have a zero gradient up to
    round-off, so Adam moves them by round-off noise scaled up to at most lr per update on either side; they do not change any
    output (batch norm subtracts them again): held to lr x 2 x bias_steps.  lr_atol: an absolute floor in units of lr (an Adam
    update of an element whose gradient is near zero is up to lr in either direction)."""
    lr = float(c["lr"])
    for k, v in model.state_dict().items():
        ref = c.get(prefix + k)
        if ref is None:
            continue
        got = v.cpu().numpy()
        if k.endswith(("lins.0.bias", "running_mean")) and bias_steps:          # (the running mean carries that bias)
            assert np.abs(got - ref).max() <= 2 * lr * bias_steps, (what, k)
            continue
        if got.dtype.kind == "i":
            assert np.array_equal(got, ref), (what, k)
        else:
            np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol * (np.abs(ref).max() + 1e-3) + lr_atol * lr, err_msg=f"{what} {k}")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_model_matches_fixture(tag):
    from ggad_amd.fullgraph import FlatAdam
    from ggad_amd.metrics import average_precision, roc_auc
    g = load_golden("fullgraph_aegis.npz")
    c = _case(g, tag)
    lr = float(c["lr"])
    all_idx, normal_idx, idx_test = list(c["all_idx"]), list(c["normal_idx"]), c["idx_test"]
    # (1) one main epoch from the initial state
    full, model, x = _setup(c)
    _cmp_state(model, c, "init.", 0, 0, "init")
    opt = FlatAdam(model.parameters(), lr=lr)
    opt_gen = FlatAdam(model.generator.parameters(), lr=lr)
    loss_ae, loss_g, score, z, z_gen, z_dec = model.train_forward(x, full, all_idx, idx_test)
    torch.autograd.backward([loss_g, loss_ae])
    for k, v in (("z", z), ("z_gen", z_gen), ("z_dec", z_dec)):
        np.testing.assert_allclose(v.detach().cpu().numpy(), c[k], rtol=1e-4, atol=2e-5, err_msg=k)
    assert abs(loss_ae.item() - float(c["loss_ae0"])) < 2e-5 * abs(float(c["loss_ae0"]))
    assert abs(loss_g.item() - float(c["loss_g0"])) < 2e-5 * abs(float(c["loss_g0"]))
    np.testing.assert_allclose(score.cpu().numpy(), c["score0"], rtol=1e-4, atol=1e-5)
    for k, p in model.named_parameters():
        ref = c.get("grad." + k)
        if ref is None:
            assert p.grad is None, k
            continue
        got = p.grad.cpu().numpy().reshape(ref.shape)
        scale = np.abs(ref).max()
        if k.endswith("lins.0.bias"):                       # in front of batch norm: zero up to round-off on both sides
            wscale = np.abs(c["grad." + k.replace(".bias", ".weight")]).max()
            assert np.abs(got).max() < 1e-4 * wscale, k
            continue
        np.testing.assert_allclose(got, ref, rtol=2e-3, atol=1e-4 * (scale + 1e-6), err_msg="grad " + k)
    opt.step()
    opt_gen.step()
    _cmp_state(model, c, "step1.", 1e-4, 1e-5, "step1", bias_steps=1)
    from ggad_amd.model_aegis import Model
    a1 = Model.affinity(z, full).cpu().numpy()
    a2 = Model.affinity(z_gen, full).cpu().numpy()
    np.testing.assert_allclose(a1, c["affinity1_0"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(a2, c["affinity2_0"], rtol=1e-4, atol=1e-5)
    # (2) the script's schedule: 10 pre-training epochs (accumulated gradients), 5 main epochs
    full, model, x = _setup(c)
    opt_ae = FlatAdam(model.parameters(), lr=1e-3)
    opt = FlatAdam(model.parameters(), lr=lr)
    opt_gen = FlatAdam(model.generator.parameters(), lr=lr)
    pre = []
    for _ in range(10):
        loss_ae, _, _, _, _, _ = model.train_forward(x, full, normal_idx, idx_test)
        loss_ae.backward()
        opt_ae.step()
        pre.append(loss_ae.item())
    np.testing.assert_allclose(pre, c["pre_losses"], rtol=1e-4)
    for k, p in model.named_parameters():
        ref = c.get("pre_grad." + k)
        if ref is None:
            assert p.grad is None, k
        else:
            np.testing.assert_allclose(p.grad.cpu().numpy().reshape(ref.shape), ref, rtol=2e-3, atol=1e-4 * np.abs(ref).max(), err_msg=k)
    yt = torch.as_tensor(c["ano"][idx_test].astype(np.int64), device=DEV)
    l_ae, l_g = [], []
    for epoch in range(5):
        model.train()
        opt.zero_grad()
        opt_gen.zero_grad()
        loss_ae, loss_g, score, _, _, _ = model.train_forward(x, full, all_idx, idx_test)
        torch.autograd.backward([loss_g, loss_ae])
        opt.step()
        opt_gen.step()
        l_ae.append(loss_ae.item())
        l_g.append(loss_g.item())
        np.testing.assert_allclose(score.cpu().numpy()[:, 0], c["main_scores"][epoch], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(l_ae, c["main_loss_ae"], rtol=2e-4)
    np.testing.assert_allclose(l_g, c["main_loss_g"], rtol=2e-4)
    _cmp_state(model, c, "final.", 1e-3, 1e-4, "final", bias_steps=15, lr_atol=0.25)
    from sklearn.metrics import roc_auc_score
    sc = score.view(-1)
    assert abs(roc_auc(sc, yt) - roc_auc_score(c["ano"][idx_test], c["main_scores"][-1])) < 1e-3
    _ = average_precision


def test_planted_auroc_ap_at_every_print_epoch():
    from ggad_amd.fullgraph import FlatAdam
    from ggad_amd.metrics import average_precision, roc_auc
    c = load_golden("fullgraph_aegis_planted.npz")
    full, model, x = _setup(c)
    lr = float(c["lr"])
    all_idx, normal_idx, idx_test = list(c["all_idx"]), list(c["normal_idx"]), c["idx_test"]
    opt_ae = FlatAdam(model.parameters(), lr=1e-3)
    opt = FlatAdam(model.parameters(), lr=lr)
    opt_gen = FlatAdam(model.generator.parameters(), lr=lr)
    for _ in range(int(c["recon_epochs"])):
        loss_ae, _, _, _, _, _ = model.train_forward(x, full, normal_idx, idx_test)
        loss_ae.backward()
        opt_ae.step()
    yt = torch.as_tensor(c["ano"][idx_test].astype(np.int64), device=DEV)
    aucs, aps = [], []
    for epoch in range(int(c["num_epoch"])):
        model.train()
        opt.zero_grad()
        opt_gen.zero_grad()
        loss_ae, loss_g, score, _, _, _ = model.train_forward(x, full, all_idx, idx_test)
        torch.autograd.backward([loss_g, loss_ae])
        opt.step()
        opt_gen.step()
        if epoch % 5 == 0:
            aucs.append(roc_auc(score.view(-1), yt))
            aps.append(average_precision(score.view(-1), yt))
            model.eval()
    # the reference's own numbers move by self_sens_* under a 1e-7 relative change of its initial weights (make_golden_aegis.py);
    # per evaluation that sensitivity is itself noisy, so the bound is 5 x its largest value over the schedule, at least 2e-4
    tol_auc = max(2e-4, 5 * float(np.max(c["self_sens_auc"])))
    tol_ap = max(2e-4, 5 * float(np.max(c["self_sens_ap"])))
    assert np.all(np.abs(np.array(aucs) - c["auc"]) <= tol_auc), (aucs, c["auc"])
    assert np.all(np.abs(np.array(aps) - c["ap"]) <= tol_ap), (aps, c["ap"])


# ------------------------------------------------------------------------------------------------ published sizes
@pytest.mark.parametrize("dataset", ["reddit", "Amazon", "photo", "t_finance", "elliptic"])
def test_one_step_at_published_size_vs_float64(dataset):
    """Loss values, test scores, every gradient and the weights after both Adam steps at the published size (synthetic graph),
    against the sparse float64 restatement.  Photo's F = 745 runs the padded dec2."""
    import scipy.sparse as sp
    from ggad_amd import synth
    from ggad_amd.fullgraph import FlatAdam, FullGraphAdj
    from ggad_amd.model_aegis import Model
    from ggad_amd.utils import normalize_adj, preprocess_features
    from run import SIZES
    n, ne, f, rate = SIZES[dataset]
    rowptr, col = synth.make_graph(n, ne, 0, kind="powerlaw", max_degree=max(64, n // 8), exact=True)
    adj = synth.csr_to_scipy(rowptr, col, n)
    feats = synth.make_features(n, f, 0)
    feats = np.asarray(preprocess_features(sp.lil_matrix(feats)), dtype=np.float32)
    ano = synth.make_labels(n, rate, 0)
    rng = np.random.default_rng(1)
    all_idx = rng.permutation(n)
    idx_test = all_idx[int(0.4 * n):]
    full = FullGraphAdj(normalize_adj(adj) + sp.eye(n), adj + sp.eye(n), DEV)
    n_h = 300 if dataset != "t_finance" else 64       # (T-Finance: 21 M entries; keeps the float64 host side short)
    torch.manual_seed(0)
    model = Model(f, n_h, "prelu", 1, "avg").to(DEV)
    P = R.params64({k: v.cpu().numpy() for k, v in model.state_dict().items()})
    noise = torch.randn(n, 16)
    model.noise_override = noise.to(DEV)
    opt = FlatAdam(model.parameters(), lr=1e-3)
    opt_gen = FlatAdam(model.generator.parameters(), lr=1e-3)
    x = torch.from_numpy(feats).to(DEV)
    loss_ae, loss_g, score, z, z_gen, z_dec = model.train_forward(x, full, all_idx, idx_test)
    torch.autograd.backward([loss_g, loss_ae])
    A, _ = R.a_hat(rowptr, col, n)
    out = R.forward(P, torch.from_numpy(feats).double(), A, noise.double(), all_idx, idx_test)
    assert abs(loss_ae.item() - out["loss_ae"].item()) < 1e-4 * abs(out["loss_ae"].item())
    assert abs(loss_g.item() - out["loss_g"].item()) < 1e-4 * abs(out["loss_g"].item())
    np.testing.assert_allclose(score.cpu().numpy()[:, 0], out["score"].detach().numpy(), rtol=1e-4, atol=1e-5)
    names = [k for k, p in model.named_parameters() if p.grad is not None]
    grads = torch.autograd.grad(out["loss_g"] + out["loss_ae"], [P[k] for k in names])
    pd = dict(model.named_parameters())
    for k, gr in zip(names, grads):
        ref = gr.numpy()
        got = pd[k].grad.cpu().numpy().reshape(ref.shape)
        if k.endswith("lins.0.bias"):
            wscale = np.abs(pd[k.replace(".bias", ".weight")].grad.cpu().numpy()).max()
            assert np.abs(got).max() < 1e-3 * wscale and np.abs(ref).max() < 1e-9 * wscale, k
            continue
        np.testing.assert_allclose(got, ref, rtol=5e-3, atol=2e-4 * (np.abs(ref).max() + 1e-9), err_msg=f"{dataset} grad {k}")
    # the weights after optimiser + optimiser_gen: float64 Adam (two instances) from the gradients just checked -- the float64 ones
    # would not do: an element whose gradient is near Adam's eps moves by up to lr on a round-off change of it
    before = {k: v.detach().cpu().double() for k, v in pd.items()}
    ours = {k: pd[k].grad.detach().cpu().double() for k in names}
    opt.step()
    opt_gen.step()
    P2 = {k: before[k].clone().requires_grad_(True) for k in names}
    for k, p in P2.items():
        p.grad = ours[k].clone()
    o1 = torch.optim.Adam(list(P2.values()), lr=1e-3)
    gen = [P2[k] for k in names if k.startswith("generator.")]
    o2 = torch.optim.Adam(gen, lr=1e-3)
    o1.step()
    o2.step()
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
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "aegis.py"), "--dataset", "reddit", "--synthetic",
           "--num_epoch", "22", "--quiet"] + extra
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    keep = [ln for ln in r.stdout.splitlines() if not ln.startswith(("training epoch captured", "median epoch"))]
    return keep, r.stdout


def test_script_captured_equals_eager(tmp_path):
    graph, raw_g = _script_lines(["--affinity_dir", str(tmp_path / "g")])
    eager, _ = _script_lines(["--no_graph", "--affinity_dir", str(tmp_path / "e")])
    assert "training epoch captured as a hipGraph" in raw_g
    assert graph == eager
    assert sum(ln.startswith("Epoch:") and "ae_loss=" in ln for ln in graph) == 10
    assert sum(ln.startswith("Testing reddit AUC:") for ln in graph) == 5
    for ep in (0, 20):                                  # epoch 20 of the captured run comes from a replay
        a = np.load(tmp_path / "g" / f"aegis_reddit_affinity_{ep}.npz")
        b = np.load(tmp_path / "e" / f"aegis_reddit_affinity_{ep}.npz")
        for k in ("normal", "generated", "anomalous"):
            assert np.array_equal(a[k], b[k])
        assert len(a["generated"]) == 500 and len(a["anomalous"]) == 50
