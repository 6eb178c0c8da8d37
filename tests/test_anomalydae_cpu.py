"""The one restated layer of the AnomalyDAE fixtures, pinned twice: the generator's torch_geometric 2.1 `GATConv` stub against a
dense float64 masked-softmax formulation (forward and gradients), and the fixtures' shapes and keys."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from ggad_amd import synth


def _gen():
    spec = importlib.util.spec_from_file_location("make_golden_anomalydae", os.path.join(GOLDEN, "make_golden_anomalydae.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _graph(n, seed):
    """Asymmetric weighted adjacency with raw self loops, an isolated node and a node whose only entry is its self loop."""
    rng = np.random.default_rng(seed)
    a = (rng.random((n, n)) < 0.08) * rng.random((n, n))
    a[np.arange(0, n, 3), np.arange(0, n, 3)] = 0.7            # raw self loops: removed, then one loop added
    a[n - 1, :] = 0
    a[:, n - 1] = 0                                             # isolated
    a[n - 2, :] = 0
    a[:, n - 2] = 0
    a[n - 2, n - 2] = 1.3                                       # only its self loop
    return torch.from_numpy(a)


@pytest.mark.parametrize("f", [10, 25, 93])
def test_gat_stub_equals_dense_float64(f):
    G = _gen()
    n, h_dim = 57, 12
    adj = _graph(n, f)
    torch.manual_seed(f)
    conv = G.PygGATConv(h_dim, f).double()
    h = torch.randn(n, h_dim, dtype=torch.float64, requires_grad=True)
    ei = torch.nonzero(adj > 0).T                               # (source r, target i) in row-major order, as neighList_to_edgeList
    conv.bias.data.normal_()
    out = conv(h, ei)
    gout = torch.randn_like(out)
    grads = torch.autograd.grad(out, [h, conv.lin_src.weight, conv.att_src, conv.att_dst, conv.bias], gout)
    h2 = h.detach().clone().requires_grad_(True)
    params = [p.detach().clone().requires_grad_(True) for p in (conv.lin_src.weight, conv.att_src, conv.att_dst, conv.bias)]
    ref = G.dense_gat(h2, *params, adj)
    grads_ref = torch.autograd.grad(ref, [h2] + params, gout)
    np.testing.assert_allclose(out.detach().numpy(), ref.detach().numpy(), rtol=1e-12, atol=1e-12)
    for a, b in zip(grads, grads_ref):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-10, atol=1e-12)


def test_gat_stub_parameter_draws():
    """Three draws of lin_src's weight, then att_src, att_dst; bias zero; lin_dst is lin_src (both keys in the state_dict)."""
    G = _gen()
    torch.manual_seed(7)
    conv = G.PygGATConv(20, 9)
    torch.manual_seed(7)
    w = torch.empty(9, 20)
    for _ in range(3):
        w.uniform_(-np.sqrt(6 / 29), np.sqrt(6 / 29))
    a_s = torch.empty(1, 1, 9).uniform_(-np.sqrt(6 / 10), np.sqrt(6 / 10))
    a_d = torch.empty(1, 1, 9).uniform_(-np.sqrt(6 / 10), np.sqrt(6 / 10))
    sd = conv.state_dict()
    assert sorted(sd) == ["att_dst", "att_src", "bias", "lin_dst.weight", "lin_src.weight"]
    assert torch.equal(sd["lin_src.weight"], w) and torch.equal(sd["lin_dst.weight"], w)
    assert torch.equal(sd["att_src"], a_s) and torch.equal(sd["att_dst"], a_d)
    assert torch.equal(sd["bias"], torch.zeros(9))


def test_gatconv_module_matches_stub_state():
    """ggad_amd.gat.GATConv draws the same parameters under the same seed (no device needed to construct it) and refuses
    non-default arguments."""
    from ggad_amd.gat import GATConv
    G = _gen()
    torch.manual_seed(3)
    a = G.PygGATConv(30, 11).state_dict()
    torch.manual_seed(3)
    b = GATConv(30, 11).state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for kw in (dict(heads=2), dict(dropout=0.1), dict(add_self_loops=False), dict(negative_slope=0.1), dict(bias=False)):
        with pytest.raises(ValueError):
            GATConv(30, 11, **kw)


def test_fixture_keys_and_shapes():
    g = load_golden("fullgraph_anomalydae.npz")
    params = ["dense_stru.weight", "dense_stru.bias", "gat_layer.att_src", "gat_layer.att_dst", "gat_layer.bias",
              "gat_layer.lin_src.weight", "gat_layer.lin_dst.weight", "dense_attr_1.weight", "dense_attr_1.bias",
              "dense_attr_2.weight", "dense_attr_2.bias", "disc.f_k.weight", "disc.f_k.bias"]
    for c in g["cases"]:
        n, f, h = int(g[f"{c}.n"]), int(g[f"{c}.f"]), int(g[f"{c}.n_h"])
        assert synth.csr_to_scipy(g[f"{c}.rowptr"], g[f"{c}.col"], n).shape == (n, n)
        assert g[f"{c}.features"].shape == (n, f)
        assert g[f"{c}.z"].shape == (n, f) and g[f"{c}.xhat"].shape == (n, f)
        nr, nt = len(g[f"{c}.normal_idx"]), len(g[f"{c}.idx_test"])
        assert len(np.unique(g[f"{c}.normal_idx"])) == nr and len(np.unique(g[f"{c}.idx_test"])) == nt
        assert g[f"{c}.attr"].shape == (nr,) and g[f"{c}.stru"].shape == (nr,)
        assert g[f"{c}.score_test0"].shape == (nt,)
        assert g[f"{c}.scores"].shape == (len(g[f"{c}.losses"]), nt)
        for k in params:
            assert f"{c}.init.{k}" in g and f"{c}.final.{k}" in g, k
        assert g[f"{c}.init.gat_layer.lin_src.weight"].shape == (f, h)
        assert g[f"{c}.init.gat_layer.att_src"].shape == (1, 1, f)
        assert f"{c}.grad.disc.f_k.weight" not in g                    # the discriminator gets no gradient
        assert np.isclose(float(g[f"{c}.loss0"]), g[f"{c}.losses"][0])
        assert np.isclose(float(g[f"{c}.loss0"]), np.mean(0.5 * g[f"{c}.attr"] + 0.5 * g[f"{c}.stru"]), rtol=1e-6)
    p = load_golden("fullgraph_anomalydae_planted.npz")
    assert len(p["auc"]) == len(p["ap"]) == len(p["eval_epochs"]) == (int(p["num_epoch"]) + 4) // 5
    assert p["features"].shape == (int(p["n"]), int(p["f"]))
