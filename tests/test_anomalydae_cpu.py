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


# ---- the sparse float64 AnomalyDAE oracle (oracle/ggad_oracle.py: adae_gat / adae_recon / adae_forward)
def _csr_with_zeros(a, seed, n_zero=6):
    """CSR of the dense `a` plus `n_zero` explicitly stored zeros at positions where `a` has none (columns sorted)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    n = a.shape[0]
    r, c = np.nonzero(a)
    free = np.flatnonzero((a == 0).reshape(-1))
    free = free[(free // n < n - 2) & (free % n < n - 2)]                 # keep the isolated / self-loop-only nodes as they are
    z = rng.choice(free, n_zero, replace=False)
    m = sp.csr_matrix((np.concatenate([a[r, c], np.zeros(n_zero)]), (np.concatenate([r, z // n]), np.concatenate([c, z % n]))),
                      shape=(n, n))
    m.sort_indices()
    assert m.nnz == len(r) + n_zero and (m.data == 0).sum() == n_zero
    return m


@pytest.mark.parametrize("f", [1, 10, 70])
@pytest.mark.parametrize("symmetric", [False, True])
def test_oracle_gat_equals_dense_float64(f, symmetric):
    """adae_gat (edge list, sparse attention matrix) equals the dense masked softmax, values and every gradient, on a graph with
    raw self loops, an isolated node, a self-loop-only node and stored zeros (not edges)."""
    from oracle import ggad_oracle as O
    G = _gen()
    n, hd = 41, 13
    a = _graph(n, 100 + f).numpy()
    if symmetric:
        a = np.triu(a, 1) + np.triu(a, 1).T + np.diag(np.diag(a))
    m = _csr_with_zeros(a, f)
    rng = np.random.default_rng(f)
    h = torch.from_numpy(rng.standard_normal((n, hd))).requires_grad_(True)
    ps = [torch.from_numpy(rng.standard_normal(s)).requires_grad_(True) for s in ((f, hd), (1, 1, f), (1, 1, f), (f,))]
    out = O.adae_gat(h, *ps, m.indptr, m.indices, m.data)
    gout = torch.from_numpy(rng.standard_normal((n, f)))
    grads = torch.autograd.grad(out, [h] + ps, gout)
    h2 = h.detach().clone().requires_grad_(True)
    ps2 = [p.detach().clone().requires_grad_(True) for p in ps]
    ref = G.dense_gat(h2, *ps2, torch.from_numpy(m.toarray()))
    grads_ref = torch.autograd.grad(ref, [h2] + ps2, gout)
    np.testing.assert_allclose(out.detach().numpy(), ref.detach().numpy(), rtol=1e-12, atol=1e-12)
    for name, a_, b_ in zip(["h", "W", "att_src", "att_dst", "bias"], grads, grads_ref):
        np.testing.assert_allclose(a_.numpy(), b_.numpy(), rtol=1e-10, atol=1e-12, err_msg=name)


@pytest.mark.parametrize("chunk_rows", [1, 4, 1000])
def test_oracle_recon_equals_dense_float64(chunk_rows):
    """adae_recon (row chunks of sigmoid(z z^T) under checkpointing) equals the materialised N x N formulation of
    double_recon_loss: loss, score, attr, stru, d/dz, d/dx_hat; unsorted rows with an isolated row, a self-loop-only row and a
    row holding a stored zero; one and several chunks."""
    from oracle import ggad_oracle as O
    n, f = 37, 9
    m = _csr_with_zeros(_graph(n, 5).numpy(), 2)
    zero_row = int(np.repeat(np.arange(n), np.diff(m.indptr))[m.data == 0][0])
    rng = np.random.default_rng(chunk_rows)
    rows = np.unique(np.concatenate([[n - 1, n - 2, zero_row], rng.choice(n, 12, replace=False)]))
    rows = rng.permutation(rows)
    z = torch.from_numpy(rng.standard_normal((n, f)) * 0.6).requires_grad_(True)
    xh = torch.from_numpy(rng.standard_normal((n, f))).requires_grad_(True)
    x = torch.from_numpy(rng.random((n, f)))
    loss, score, attr, stru = O.adae_recon(z, xh, x, (m.indptr, m.indices, m.data), rows, chunk_elems=chunk_rows * n)
    (1.7 * loss).backward()
    z2 = z.detach().clone().requires_grad_(True)
    xh2 = xh.detach().clone().requires_grad_(True)
    A = torch.from_numpy(m.toarray())
    r = torch.from_numpy(rows)
    attr2 = torch.sqrt(torch.sum((x[r] - xh2[r]) ** 2, 1))
    stru2 = torch.sqrt(torch.sum((A[r] - torch.sigmoid(z2 @ z2.T)[r]) ** 2, 1))
    score2 = 0.5 * attr2 + 0.5 * stru2
    (1.7 * score2.mean()).backward()
    for name, a_, b_ in [("loss", loss, score2.mean()), ("score", score, score2), ("attr", attr, attr2), ("stru", stru, stru2),
                         ("dz", z.grad, z2.grad), ("dxhat", xh.grad, xh2.grad)]:
        np.testing.assert_allclose(a_.detach().numpy(), b_.detach().numpy(), rtol=1e-12, atol=1e-14, err_msg=name)


def _fixture_inputs(g, c):
    import scipy.sparse as sp
    from ggad_amd import utils as U
    n = int(g[f"{c}.n"])
    a = synth.csr_to_scipy(g[f"{c}.rowptr"], g[f"{c}.col"], n)
    ah = sp.csr_matrix(U.normalize_adj(a) + sp.eye(n))
    ah.sort_indices()
    return (ah.indptr, ah.indices, ah.data.astype(np.float32)), torch.from_numpy(g[f"{c}.features"]).double()


@pytest.mark.parametrize("case", ["a", "b"])
def test_oracle_reproduces_reference_fixture(case):
    """adae_forward + adae_recon in float64 reproduce what the imported reference computed (fp32) on the fixture's first step:
    z, x_hat, attr / stru, loss, the test scores and every parameter gradient, within test_model_against_reference_fixture's
    tolerances for the HIP path."""
    from oracle import ggad_oracle as O
    g = load_golden("fullgraph_anomalydae.npz")
    c = case
    A, x = _fixture_inputs(g, c)
    P = {k: torch.from_numpy(g[f"{c}.init.{k}"]).double().requires_grad_(True) for k in O.ADAE_PARAM_ORDER}
    xhat, z = O.adae_forward(P, x, A)
    loss, _, attr, stru = O.adae_recon(z, xhat, x, A, g[f"{c}.normal_idx"])
    loss.backward()
    with torch.no_grad():
        score_test = O.adae_recon(z, xhat, x, A, g[f"{c}.idx_test"])[1]
    np.testing.assert_allclose(z.detach().numpy(), g[f"{c}.z"], atol=3e-6)
    np.testing.assert_allclose(xhat.detach().numpy(), g[f"{c}.xhat"], atol=3e-6)
    np.testing.assert_allclose(attr.detach().numpy(), g[f"{c}.attr"], atol=1e-5)
    np.testing.assert_allclose(stru.detach().numpy(), g[f"{c}.stru"], atol=1e-5)
    assert abs(loss.item() - float(g[f"{c}.loss0"])) < 1e-5
    np.testing.assert_allclose(score_test.numpy(), g[f"{c}.score_test0"], atol=1e-5)
    grads = sorted(k[len(f"{c}.grad."):] for k in g if k.startswith(f"{c}.grad."))
    assert grads == sorted(O.ADAE_PARAM_ORDER)
    for k in O.ADAE_PARAM_ORDER:
        np.testing.assert_allclose(P[k].grad.numpy(), g[f"{c}.grad.{k}"], atol=4e-6, rtol=2e-4, err_msg=k)


def _cached_ptrs(fa, rows):
    """data_ptr() of every tensor of the cached structures of the row list `rows` (None: not cached), read from the cache without
    a lookup (a lookup would rebuild an evicted list)."""
    arr = np.asarray(rows, dtype=np.int64)
    for k, s in fa.__dict__.get("_adae", {}).items():
        if isinstance(k, tuple) and k[0] == "rows" and np.array_equal(s["host"], arr):
            return {n: t.data_ptr() for n, t in s.items() if isinstance(t, torch.Tensor)}
    return None


def test_row_list_looked_up_during_capture_is_never_evicted(monkeypatch):
    """A captured graph holds raw pointers to the structures of its row list: a lookup during a stream capture pins the list, and
    scoring 20 other lists afterwards (more than the 16 the cache keeps) leaves its tensors in place.  The capture is simulated
    (`_capturing` patched; the structures live on the host here): the GPU side is test_anomalydae_branches_gpu.py."""
    import scipy.sparse as sp
    from ggad_amd import model_anomalydae as M
    from ggad_amd.fullgraph import FullGraphAdj
    n = 60
    a = sp.csr_matrix(_graph(n, 1).numpy() + np.eye(n))
    fa = FullGraphAdj(a, a, "cpu")
    rows = np.arange(3, 40, 2)
    M.row_structs(fa, rows)                                         # built eagerly first, as before the script's capture
    with monkeypatch.context() as mp:
        mp.setattr(M, "_capturing", lambda dev: True)
        captured = M.row_structs(fa, rows)
    ptrs = {k: t.data_ptr() for k, t in captured.items() if isinstance(t, torch.Tensor)}
    del captured
    for k in range(20):
        M.row_structs(fa, np.arange(k, k + 10))
    assert _cached_ptrs(fa, rows) == ptrs
    assert _cached_ptrs(fa, np.arange(0, 10)) is None               # unpinned lists are still evicted
