"""The float64 mode of the mini-batch oracle (`aggregate_batch` / `encoder_forward` / `batch_loss` with dtype=np.float64, and
`adam_f64`): the high-precision reference the HIP kernels are compared with in tests/test_resident_step_gpu.py.

It must reproduce the reference's captured vectors (tests/golden/minibatch_*.npz, float32 captures) within the tolerances the
float32 oracle meets in tests/test_oracle_golden.py: the float64 result is the truth, the captures carry fp32 round-off.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import ggad_oracle as O

TOL = 2e-6


def _leaves(g, prefix, dtype):
    return O.MiniParams.leaves(g[prefix + ".weight"], g[prefix + ".enc.weight"], g[prefix + ".enc.fc.weight"], dtype)


@pytest.mark.parametrize("name", ["minibatch_small.npz", "minibatch_dense.npz"])
def test_float64_oracle_reproduces_the_reference_vectors(name):
    g = load_golden(name)
    p = _leaves(g, "init", torch.float64)
    n = len(p.tensors())
    m = [np.zeros(t.shape) for t in p.tensors()]
    v = [np.zeros(t.shape) for t in p.tensors()]
    for step, (nodes, lab) in enumerate(zip(g["batches"], g["labels"])):
        agg = O.aggregate_batch(g["rowptr"], g["col"], g["feat"], nodes, True, dtype=np.float64)
        assert agg.to_feats.dtype == np.float64 and agg.to_feats_neigh.dtype == np.float64
        if step == 0:
            np.testing.assert_allclose(agg.to_feats, g["agg_to_feats"], atol=TOL, rtol=0)
            perm = np.searchsorted(agg.unique, g["agg_unique"])
            np.testing.assert_allclose(agg.to_feats_neigh[perm], g["agg_to_feats_neigh"], atol=TOL, rtol=0)
            with torch.no_grad():
                ca, nbar, af, afn = O.encoder_forward(p, agg, lab, True, dtype=np.float64)
            for t in (ca, nbar, af, afn):
                assert t.dtype == torch.float64
            np.testing.assert_allclose(ca.numpy(), g["enc_combined_all"], atol=TOL, rtol=0)
            np.testing.assert_allclose(nbar.numpy(), g["enc_to_feats_neigh"], atol=TOL, rtol=0)
            np.testing.assert_allclose(af.numpy(), g["enc_anomaly_feat"], atol=TOL, rtol=0)
            np.testing.assert_allclose(afn.numpy(), g["enc_anomaly_feat_new"], atol=TOL, rtol=0)
        for t in p.tensors():
            t.grad = None
        terms = O.batch_loss(p, agg, lab, dtype=torch.float64)
        assert all(x.dtype == torch.float64 for x in terms)
        terms[0].backward()
        np.testing.assert_allclose([x.item() for x in terms], g["losses"][step], atol=5e-6, rtol=0)
        grads = [t.grad.numpy() for t in p.tensors()]
        if step == 0:
            for key, gr in zip(("grad.weight", "grad.enc.weight", "grad.enc.fc.weight"), grads):
                np.testing.assert_allclose(gr, g[key], atol=TOL, rtol=1e-5, err_msg=key)
        with torch.no_grad():
            for k in range(n):
                pk, m[k], v[k] = O.adam_f64(p.tensors()[k].numpy(), m[k], v[k], grads[k], step + 1)
                p.tensors()[k].copy_(torch.from_numpy(pk))
        if step == 0:
            np.testing.assert_allclose(p.weight.detach().numpy(), g["step1.weight"], atol=TOL, rtol=0)
            np.testing.assert_allclose(p.enc_weight.detach().numpy(), g["step1.enc.weight"], atol=TOL, rtol=0)
            np.testing.assert_allclose(p.enc_fc_weight.detach().numpy(), g["step1.enc.fc.weight"], atol=TOL, rtol=0)
    np.testing.assert_allclose(p.weight.detach().numpy(), g["final.weight"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(p.enc_weight.detach().numpy(), g["final.enc.weight"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(p.enc_fc_weight.detach().numpy(), g["final.enc.fc.weight"], atol=2e-5, rtol=0)


@pytest.mark.parametrize("name", ["minibatch_small.npz", "minibatch_dense.npz"])
def test_float32_default_is_unchanged_and_float64_is_closer_to_itself(name):
    """dtype=np.float32 (the default) is the same computation as before the dtype argument existed: bit-identical aggregates
    and losses; the float64 result differs from it by fp32 round-off only."""
    g = load_golden(name)
    nodes, lab = g["batches"][0], g["labels"][0]
    a32 = O.aggregate_batch(g["rowptr"], g["col"], g["feat"], nodes, True)
    b32 = O.aggregate_batch(g["rowptr"], g["col"], g["feat"], nodes, True, dtype=np.float32)
    assert a32.to_feats.dtype == np.float32
    assert np.array_equal(a32.to_feats, b32.to_feats) and np.array_equal(a32.to_feats_neigh, b32.to_feats_neigh)
    l32 = [x.item() for x in O.batch_loss(_leaves(g, "init", torch.float32), a32, lab)]
    l32b = [x.item() for x in O.batch_loss(_leaves(g, "init", torch.float32), a32, lab, dtype=torch.float32)]
    assert l32 == l32b
    a64 = O.aggregate_batch(g["rowptr"], g["col"], g["feat"], nodes, True, dtype=np.float64)
    l64 = [x.item() for x in O.batch_loss(_leaves(g, "init", torch.float64), a64, lab, dtype=np.float64)]
    np.testing.assert_allclose(l64, l32, atol=2e-6, rtol=0)
    assert np.abs(a64.to_feats - a32.to_feats).max() > 0          # really a different precision


@pytest.mark.parametrize("step", [1, 2, 10000])
def test_adam_f64_is_torch_adam_in_float64(step):
    """`adam_f64` against torch.optim.Adam itself on float64 tensors (lr 1e-3, weight decay 0.007, betas (0.9, 0.999), eps
    1e-8), from fresh state (step 1) and from preloaded moments at later step numbers: equal to float64 round-off."""
    rng = np.random.default_rng(step)
    p0 = rng.standard_normal((7, 5))
    g = rng.standard_normal((7, 5)) * 1e-3
    m0 = np.zeros_like(p0) if step == 1 else rng.standard_normal((7, 5)) * 1e-3
    v0 = np.zeros_like(p0) if step == 1 else rng.random((7, 5)) * 1e-5
    t = torch.tensor(p0, requires_grad=True)
    opt = torch.optim.Adam([t], lr=1e-3, weight_decay=0.007)
    if step > 1:
        opt.state[t] = dict(step=torch.tensor(float(step - 1), dtype=torch.float32), exp_avg=torch.tensor(m0),
                            exp_avg_sq=torch.tensor(v0))
    t.grad = torch.tensor(g)
    opt.step()
    p1, m1, v1 = O.adam_f64(p0, m0, v0, g, step)
    np.testing.assert_allclose(p1, t.detach().numpy(), atol=1e-15, rtol=1e-13)
    np.testing.assert_allclose(m1, opt.state[t]["exp_avg"].numpy(), atol=1e-18, rtol=1e-13)
    np.testing.assert_allclose(v1, opt.state[t]["exp_avg_sq"].numpy(), atol=1e-20, rtol=1e-13)
