"""The restatement the device tests of the mini-batch AEGIS step are measured against (`tests/aegis_mb_fp64.py`) is the model: at
float32 it equals the oracle's `aegis_forward` / `aegis_loss` under torch autograd on a small CSR graph, and its running buffers are
`nn.BatchNorm1d`'s after the two calls of one forward."""
import numpy as np
import torch

import aegis_mb_fp64 as R
from ggad_amd import synth
from oracle import ggad_oracle as O


def _setup():
    n, f, b = 400, 17, 37
    rowptr, col = synth.make_graph(n, 3000, 9, kind="powerlaw", max_degree=60)
    feat = O.normalize_rows(synth.make_features(n, f, 9)).astype(np.float32)
    noise = np.random.default_rng(9).standard_normal((n, f)).astype(np.float32)
    nodes = np.random.default_rng(10).choice(n, size=b, replace=False)
    params = R.make_params(f, 12)
    x_feat = O.aggregate_batch(rowptr, col, feat, nodes, False).to_feats
    x_noise = O.aggregate_batch(rowptr, col, noise, nodes, False).to_feats
    return rowptr, col, feat, noise, nodes, params, x_feat, x_noise


def test_float32_restatement_equals_the_oracle_under_autograd():
    """Bounds: those of `test_aegis_minibatch_model_against_the_oracle_restatement` (tests/test_baselines_gpu.py:193-212)."""
    rowptr, col, feat, noise, nodes, params, x_feat, x_noise = _setup()
    P = {k: torch.from_numpy(p.copy()).requires_grad_() for k, p in zip(R.PARAMS, params)}
    la, lg, _ = O.aegis_forward(P, rowptr, col, feat, noise, nodes)
    r1, r2 = O.aegis_loss(P, rowptr, col, feat, noise, nodes)
    (r1 + r2).backward()
    got = R.evaluate(x_feat, x_noise, params, torch.float32)
    np.testing.assert_allclose(got["p"], la.detach().numpy(), atol=3e-6, rtol=0)
    np.testing.assert_allclose(got["p_gen"], lg.detach().numpy(), atol=3e-6, rtol=0)
    np.testing.assert_allclose([got["loss_dis"][0], got["loss_g"][0]], [r1.item(), r2.item()], atol=5e-6, rtol=0)
    for k in R.PARAMS:
        np.testing.assert_allclose(got["grad." + k], P[k].grad.numpy(), atol=5e-6, rtol=2e-4, err_msg=k)
    assert float(np.abs(got["grad.enc.weight"]).max()) > 1e-4          # a live gradient, not zeros against zeros


def test_running_buffers_equal_batchnorm1d_after_the_two_calls():
    _, _, _, _, nodes, params, x_feat, x_noise = _setup()
    b = len(nodes)
    w, w0, b0, gamma, beta = (torch.from_numpy(p) for p in params[:5])
    bn = torch.nn.BatchNorm1d(64)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        h = torch.relu(torch.cat([torch.from_numpy(x_feat), torch.from_numpy(x_noise)], 0).mm(w.t())).mm(w0.t()) + b0
        bn(h)
        bn(h[b:])
        first = (bn.running_mean.clone().numpy(), bn.running_var.clone().numpy())
        bn(h)
        bn(h[b:])
    assert bn.training and int(bn.num_batches_tracked) == 4
    got = R.evaluate(x_feat, x_noise, params, torch.float32)
    np.testing.assert_allclose(got["running_mean"], first[0], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(got["running_var"], first[1], rtol=1e-6, atol=0)
    again = R.evaluate(x_feat, x_noise, params, torch.float32, running=first)
    np.testing.assert_allclose(again["running_mean"], bn.running_mean.numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(again["running_var"], bn.running_var.numpy(), rtol=1e-6, atol=0)
