"""The float64 restatement of the fused TAM head (tests/tam_head_fp64.py) against (a) torch's CPU autograd in float64 on the
reference's dense formulation (`tam.py:113-146`, restated below) and (b) the vectors captured from the imported reference
(`tests/golden/fullgraph_tam.npz`).  No GPU."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import tam_head_fp64 as H

HERE = os.path.dirname(os.path.abspath(__file__))


def dense_max_message(feature, adj_matrix, normal_label_idx, guarded=False):
    """`max_message` of the reference, line by line (also returns the un-normalised message = `inference` with the NaN rows zeroed).
    `guarded`: the normalisation as x * (1 / |x|, inf -> 0), what the project's row-normalise kernels compute.  The forward values are
    the same (the reference zeroes the NaN products of a zero row two lines later); the gradients differ only when a row has zero
    norm, where the reference's 0 / 0 turns the WHOLE gradient into NaN (NaN x 0 in the backward of the product) -- see below."""
    if guarded:
        feature = feature * _masked_inv(feature)
    else:
        feature = feature / torch.norm(feature, dim=-1, keepdim=True)
    sim_matrix = torch.mm(feature, feature.T)
    sim_matrix = torch.squeeze(sim_matrix) * adj_matrix
    sim_matrix[torch.isinf(sim_matrix)] = 0
    sim_matrix[torch.isnan(sim_matrix)] = 0
    row_sum = torch.sum(adj_matrix, 0)
    r_inv = torch.pow(row_sum, -1).flatten()
    r_inv[torch.isinf(r_inv)] = 0.
    raw = torch.sum(sim_matrix, 1) * r_inv
    message = (raw - torch.min(raw)) / (torch.max(raw) - torch.min(raw))
    return -torch.sum(message[normal_label_idx]), message, raw


def _masked_inv(x):
    """1 / |x_i| with its own gradient, 0 (and gradient 0) for the rows of zero norm."""
    nz = (x.detach() != 0).any(-1, keepdim=True)
    safe = torch.where(nz, x, torch.ones_like(x))
    return torch.where(nz, 1.0 / torch.norm(safe, dim=-1, keepdim=True), torch.zeros_like(x[:, :1]))


def _sym(n, density, rng, values=False, diag=1.0):
    m = sp.random(n, n, density=density, random_state=np.random.RandomState(int(rng.integers(1 << 30))), format="csr")
    m.data[:] = 1.0
    m = ((m + m.T) > 0).astype(np.float64)
    if values:
        w = sp.triu(m, 1).tocsr()
        w.data[:] = rng.uniform(0.5, 2.0, w.nnz)
        m = w + w.T
    m = (m.tolil())
    m.setdiag(diag)
    m = m.tocsr()
    m.sort_indices()
    return m


def _case(name):
    rng = np.random.default_rng(11)
    n, h = 40, 7
    if name == "plain":
        R = _sym(n, 0.15, rng)
        e = rng.standard_normal((n, h))
        idx = rng.permutation(n)[:12]
    elif name == "values_repeats":
        R = _sym(n, 0.15, rng, values=True, diag=2.0)
        e = rng.standard_normal((n, h))
        idx = np.concatenate([rng.permutation(n)[:12], [3, 3, 5]])
    elif name == "zero_rows":
        R = _sym(n, 0.15, rng)
        e = rng.standard_normal((n, h))
        e[[4, 17]] = 0.0
        idx = np.concatenate([rng.permutation(n)[:10], [4]])
    elif name == "ties":
        # non-negative embeddings: 0 <= a <= 1.  Three zero rows (a = 0 exactly) and three self-loop-only rows holding a power-of-two
        # multiple of a basis vector (a = 1 exactly); every other row has a neighbour at an angle, so it stays inside (0, 1)
        R = _sym(n, 0.15, rng).tolil()
        ones = [1, 20, 33]
        for i in ones:
            R[i, :] = 0
            R[:, i] = 0
            R[i, i] = 1.0
        R = R.tocsr()
        R.eliminate_zeros()
        R.sort_indices()
        e = rng.uniform(0.2, 1.0, (n, h))
        zeros = [0, 9, 39]
        e[zeros] = 0.0
        for k, i in enumerate(ones):
            e[i] = 0.0
            e[i, k] = 2.0 ** (k - 1)
        idx = np.concatenate([rng.permutation(n)[:10], [0, 0, 20, 9, 33, 33]])        # repeats, incl. arg-min and arg-max nodes
    else:
        raise KeyError(name)
    return R, e, np.asarray(idx, dtype=np.int64)


@pytest.mark.parametrize("name", ["plain", "values_repeats", "zero_rows", "ties"])
def test_helper_matches_dense_autograd(name):
    R, e, idx = _case(name)
    n = R.shape[0]
    colsum = np.asarray(R.sum(0)).reshape(-1)
    with np.errstate(divide="ignore"):
        r_inv = 1.0 / colsum
    r_inv[np.isinf(r_inv)] = 0.0
    out = H.tam_head_fp64(R.indptr, R.indices, R.data, r_inv, e, idx, g=1.0)

    et = torch.tensor(e, dtype=torch.float64, requires_grad=True)
    loss, m, raw = dense_max_message(et, torch.tensor(R.toarray(), dtype=torch.float64), torch.as_tensor(idx))
    g_raw, = torch.autograd.grad(loss, raw, retain_graph=True)
    loss.backward()
    np.testing.assert_allclose(out["a"], raw.detach().numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(out["m"], m.detach().numpy(), rtol=0, atol=1e-13)
    assert abs(out["loss"] - loss.item()) < 1e-12 * max(1.0, abs(loss.item()))
    assert abs(out["lo"] - raw.min().item()) < 1e-14 and abs(out["hi"] - raw.max().item()) < 1e-14
    np.testing.assert_allclose(out["da"], g_raw.numpy(), rtol=1e-12, atol=1e-12)        # the closed form, ties shared evenly
    if name == "ties":
        assert out["n_lo"] == 3 and out["n_hi"] == 3 and out["lo"] == 0.0 and out["hi"] == 1.0
        inside = np.ones(n, bool)
        inside[[0, 9, 39, 1, 20, 33]] = False
        assert out["a"][inside].min() > 0.05 and out["a"][inside].max() < 0.999
    zero = np.sqrt((e * e).sum(1)) == 0
    ge = et.grad.numpy()
    if zero.any():
        # the reference's literal expression: forward as above, but every element of its gradient is NaN.  The gradient reference is
        # the guarded normalisation, whose zero rows get 0 -- what `k_rownorm_bwd` of the composed path gives
        assert np.isnan(ge).all()
        eg = torch.tensor(e, dtype=torch.float64, requires_grad=True)
        loss_g, m_g, raw_g = dense_max_message(eg, torch.tensor(R.toarray(), dtype=torch.float64), torch.as_tensor(idx), guarded=True)
        assert (raw_g - raw).abs().max().item() < 1e-14 and abs(loss_g.item() - loss.item()) < 1e-12       # x / |x| vs x * (1 / |x|)
        loss_g.backward()
        ge = eg.grad.numpy()
        assert np.all(out["d_emb"][zero] == 0.0) and np.all(ge[zero] == 0.0)
    scale = max(1.0, np.abs(ge).max())
    np.testing.assert_allclose(out["d_emb"], ge, rtol=0, atol=1e-11 * scale)


def test_helper_scales_with_upstream_gradient():
    R, e, idx = _case("values_repeats")
    colsum = np.asarray(R.sum(0)).reshape(-1)
    a = H.tam_head_fp64(R.indptr, R.indices, R.data, 1.0 / colsum, e, idx, g=1.0)
    b = H.tam_head_fp64(R.indptr, R.indices, R.data, 1.0 / colsum, e, idx, g=-2.5)
    np.testing.assert_allclose(b["d_emb"], -2.5 * a["d_emb"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("cut", [0, 1])
def test_helper_matches_golden(cut):
    g = np.load(os.path.join(HERE, "golden", "fullgraph_tam.npz"))
    n = int(g["n"])
    A = sp.csr_matrix((np.ones(len(g["col"]), np.float64), g["col"], g["rowptr"]), shape=(n, n))
    R = (A + sp.eye(n)).tocsr()
    R.sort_indices()
    assert abs(R - R.T).nnz == 0
    r_inv = 1.0 / np.asarray(R.sum(0)).reshape(-1)
    out = H.tam_head_fp64(R.indptr, R.indices, R.data, r_inv, g[f"cut{cut}.emb"], g["normal_idx"])
    # the golden vectors are float32 results of the reference: the tolerances of tests/test_tam_gpu.py
    np.testing.assert_allclose(out["a"], g[f"cut{cut}.message"], atol=3e-6)
    np.testing.assert_allclose(out["m"], g[f"cut{cut}.message_norm"], atol=5e-6)
    assert abs(out["loss"] - g[f"cut{cut}.losses"][0]) < 2e-4
