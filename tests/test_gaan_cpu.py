"""Full-graph GAAN without a GPU: the drop-in Model's initial state equals the imported reference's (fixture) bit for bit, the host
edge-set builder yields the reference's neighList_to_edgeList_train set, and the float64 restatement the GPU tests compare against
(tests/gaan_fp64.py) reproduces the fixture's forward values, scores and gradients."""
import numpy as np
import pytest
import torch

import gaan_fp64 as R
from conftest import load_golden


# biases in front of a training-mode batch norm: their gradient is exactly zero in exact arithmetic
ZERO_GRAD = ("generator.lins.0.bias", "discriminator.lins.0.bias")


@pytest.fixture(scope="module")
def g():
    return load_golden("fullgraph_gaan.npz")


def _case(g, tag):
    return {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + ".")}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_initial_state_dict_is_bit_equal_to_the_reference(g, tag):
    from ggad_amd.model_gaan import Model
    c = _case(g, tag)
    torch.manual_seed(int(c["seed"]))
    model = Model(int(c["f"]), int(c["n_h"]), "prelu", 1, "avg")
    sd = model.state_dict()
    ref = {k[5:]: v for k, v in c.items() if k.startswith("init.")}
    assert list(sd) == list(ref)
    for k, v in sd.items():
        assert v.dtype == torch.from_numpy(ref[k]).dtype, k
        assert np.array_equal(v.numpy(), ref[k]), k
    # the constructors consumed the same stream: the next draw is the first forward's noise
    assert np.array_equal(torch.randn(int(c["n"]), 16).numpy(), c["noise0"])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_edge_set_builder_equals_reference_edge_list(g, tag):
    """Same pairs, same order, same count as the reference's neighList_to_edgeList_train on the dense A_hat; graph 'b' (asymmetric,
    a proper row subset) has stored entries of A_hat that are not positive, and they are left out."""
    from ggad_amd.model_gaan import edge_list
    c = _case(g, tag)
    n = int(c["n"])
    import scipy.sparse as sp
    A = R.a_hat(c["rowptr"], c["col"], n)
    ref = c["edges"]
    # stored entries that are not positive, at places the dense A_hat holds 0 (a zero, or a negative value: not > 0 either way)
    rng = np.random.default_rng(5)
    free = np.flatnonzero(np.asarray(A.todense()).reshape(-1) == 0)
    put = rng.choice(free, 300, replace=False)
    coo = A.tocoo()
    extra = np.where(np.arange(300) % 2 == 0, 0.0, -0.25)
    A2 = sp.csr_matrix((np.concatenate([coo.data, extra]), (np.concatenate([coo.row, put // n]), np.concatenate([coo.col, put % n]))),
                       shape=(n, n))
    assert A2.nnz == A.nnz + 300 and (A2.data <= 0).sum() == 300
    for mat in (A, A2):
        erow, ecol, cnt = edge_list(mat, c["idx_train"])
        assert len(erow) == int(c["m"]) == len(ref)
        assert np.array_equal(erow, ref[:, 0]) and np.array_equal(ecol, ref[:, 1])
        assert cnt.sum() == len(ref) and np.all(cnt >= 1)                 # every row keeps its diagonal at least
    if tag == "b":
        assert len(c["idx_train"]) < n
        assert abs(A - A.T).nnz > 0
        assert A[n - 1].nnz == 1 and A[n - 2].nnz == 1                    # isolated; self loop only


@pytest.mark.parametrize("tag", ["a", "b"])
def test_float64_restatement_reproduces_the_fixture(g, tag):
    from ggad_amd.model_gaan import edge_list
    c = _case(g, tag)
    n = int(c["n"])
    P = R.params64({k[5:]: v for k, v in c.items() if k.startswith("init.")})
    erow, ecol, _ = edge_list(R.a_hat(c["rowptr"], c["col"], n), c["idx_train"])
    x = torch.from_numpy(c["features"]).double()
    out = R.forward(P, x, torch.from_numpy(c["noise0"]).double(), erow, ecol, c["idx_train"], c["idx_test"])
    for k, ref in (("x_", c["x_"]), ("emb", c["emb"]), ("z", c["z_"])):
        np.testing.assert_allclose(out[k].detach().numpy(), ref, rtol=2e-5, atol=2e-5 * np.abs(ref).max(), err_msg=k)
    for k in ("loss", "loss_f", "loss_r", "loss_g"):
        ref = float(c[k + "0"])
        assert abs(out[k].item() - ref) <= 1e-5 * abs(ref), (k, out[k].item(), ref)
    np.testing.assert_allclose(out["score"].detach().numpy(), c["score0"], rtol=1e-5, atol=1e-6)
    names = [k for k in P if P[k].requires_grad]
    grads = torch.autograd.grad(out["loss"] + out["loss_g"], [P[k] for k in names], allow_unused=True)
    seen = 0
    for k, gr in zip(names, grads):
        ref = c.get("grad." + k)
        if ref is None:
            assert gr is None or not gr.abs().max() > 0, k                  # the unused disc gets no gradient
            continue
        seen += 1
        gr = gr.numpy().reshape(ref.shape)
        if k in ZERO_GRAD:
            scale = np.abs(c["grad." + k.replace(".bias", ".weight")]).max()
            assert np.abs(ref).max() < 1e-3 * scale and np.abs(gr).max() < 1e-12 * scale, k
            continue
        np.testing.assert_allclose(gr, ref, rtol=2e-4, atol=2e-5 * (np.abs(ref).max() + 1e-6), err_msg=k)
    assert seen == len([k for k in c if k.startswith("grad.")]) == 12
    run = R.running_after(P, out["stats"])
    for k, v in run.items():
        np.testing.assert_allclose(v.numpy(), c["step1." + k], rtol=1e-5, atol=1e-7, err_msg=k)
    assert int(c["step1.discriminator.norms.0.module.num_batches_tracked"]) == 2
    assert int(c["step1.generator.norms.0.module.num_batches_tracked"]) == 1


def test_edge_reference_saturation_matches_float32():
    """The float64 edge reference with float32 saturation: dots > 17 give a = 1 (BCE(a', 0) term clamped at 100), dots < -89 give
    a = 0 (BCE(a, 1) term clamped at 100); the backward coefficient of a saturated entry is exactly 0."""
    emb = np.array([[30.0, 0.0], [1.0, 0.0], [-4.0, 0.0]])
    erow, ecol = np.array([0, 0, 1]), np.array([1, 2, 1])
    a = R.sigmoid32(np.einsum("ij,ij->i", emb[erow], emb[ecol]))
    assert a[0] == 1.0 and a[1] == 0.0
    loss, lf, lr, dE = R.edge_loss_ref(emb, emb, erow, ecol, f32_sigmoid=True)
    assert lr > 100.0 / 3 - 1e-9 and lf > 100.0 / 3
    assert np.all(np.isfinite(dE))
