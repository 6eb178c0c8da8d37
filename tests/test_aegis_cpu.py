"""Full-graph AEGIS without a GPU: the drop-in Model's initial state equals the imported reference's (fixture) bit for bit, the
fixture generator's torch_geometric MLP stub is torch's own layers and draws what `graphsage_aegis.MLP` draws, and the float64
restatement the GPU tests compare against (tests/aegis_fp64.py) reproduces the fixture's forward values and gradients."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aegis_fp64 as R
from conftest import GOLDEN, load_golden


# biases in front of a training-mode batch norm: their gradient is exactly zero in exact arithmetic
ZERO_GRAD = ("generator.lins.0.bias", "discriminator2.lins.0.bias")


def _gen():
    spec = importlib.util.spec_from_file_location("make_golden_aegis", os.path.join(GOLDEN, "make_golden_aegis.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def g():
    return load_golden("fullgraph_aegis.npz")


def _case(g, tag):
    return {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + ".")}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_initial_state_dict_is_bit_equal_to_the_reference(g, tag):
    from ggad_amd.model_aegis import Model
    c = _case(g, tag)
    torch.manual_seed(int(c["seed"]))
    model = Model(int(c["f"]), int(c["n_h"]), "prelu", 1, "avg")
    sd = model.state_dict()
    ref = {k[5:]: v for k, v in c.items() if k.startswith("init.")}
    assert sorted(sd) == sorted(ref)
    for k, v in sd.items():
        assert v.dtype == torch.from_numpy(ref[k]).dtype, k
        assert np.array_equal(v.numpy(), ref[k]), k
    # the next draw of the CPU generator is the first forward's noise: the constructors consumed the same stream
    noise = torch.randn(int(c["n"]), 16)
    assert noise.shape == (int(c["n"]), 16)


def test_mlp_stub_equals_torch_layers_and_draws_like_graphsage_aegis_mlp():
    from ggad_amd.graphsage_aegis import MLP
    G = _gen()
    for act, tf in ((F.relu, torch.relu), (torch.sigmoid, torch.sigmoid)):
        torch.manual_seed(5)
        stub = G.PygMLP(16, 64, 37, 2, dropout=0.0, act=act).double()
        torch.manual_seed(5)
        ours = MLP(16, 64, 37, 2, 0.0, act)
        assert list(stub.state_dict()) == list(ours.state_dict())
        for (k, a), b in zip(stub.state_dict().items(), ours.state_dict().values()):
            assert np.array_equal(a.float().numpy() if a.is_floating_point() else a.numpy(), b.numpy()), k
        x = torch.randn(50, 16, dtype=torch.float64)
        stub.train()
        got = stub(x)
        bn = stub.norms[0].module
        h = x @ stub.lins[0].weight.T + stub.lins[0].bias
        ref = tf(F.batch_norm(h, None, None, bn.weight, bn.bias, training=True, eps=1e-5)) @ stub.lins[1].weight.T + stub.lins[1].bias
        np.testing.assert_allclose(got.detach().numpy(), ref.detach().numpy(), rtol=1e-13, atol=1e-13)
        assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("tag", ["a", "b"])
def test_float64_restatement_reproduces_the_fixture_forward_and_gradients(g, tag):
    from ggad_amd.model_aegis import Model
    c = _case(g, tag)
    n = int(c["n"])
    torch.manual_seed(int(c["seed"]))
    Model(int(c["f"]), int(c["n_h"]), "prelu", 1, "avg")
    noise = torch.randn(n, 16).double()
    P = R.params64({k[5:]: v for k, v in c.items() if k.startswith("init.")})
    A, _ = R.a_hat(c["rowptr"], c["col"], n)
    x = torch.from_numpy(c["features"]).double()
    out = R.forward(P, x, A, noise, c["all_idx"], c["idx_test"])
    for k in ("x_gen", "z", "z_gen", "z_dec"):
        np.testing.assert_allclose(out[k].detach().numpy(), c[k], rtol=2e-5, atol=2e-6, err_msg=k)
    np.testing.assert_allclose(out["score"].detach().numpy(), c["score0"][:, 0], rtol=1e-5, atol=1e-6)
    assert abs(out["loss_ae"].item() - float(c["loss_ae0"])) <= 1e-5 * abs(float(c["loss_ae0"]))
    assert abs(out["loss_g"].item() - float(c["loss_g0"])) <= 1e-5 * abs(float(c["loss_g0"]))
    names = [k for k in P if P[k].requires_grad]
    grads = torch.autograd.grad(out["loss_g"] + out["loss_ae"], [P[k] for k in names], allow_unused=True)
    seen = 0
    for k, gr in zip(names, grads):
        ref = c.get("grad." + k)
        if ref is None:
            assert gr is None or not gr.abs().max() > 0, k            # the unused disc / discriminator get no gradient
            continue
        seen += 1
        gr = gr.numpy().reshape(ref.shape)
        if k in ZERO_GRAD:                                            # a bias in front of batch norm: 0 up to round-off
            scale = np.abs(c["grad." + k.replace(".bias", ".weight")]).max()
            assert np.abs(ref).max() < 1e-5 * scale and np.abs(gr).max() < 1e-12 * scale, k
            continue
        np.testing.assert_allclose(gr, ref, rtol=2e-4, atol=2e-5 * (np.abs(ref).max() + 1e-6), err_msg=k)
    assert seen == len([k for k in c if k.startswith("grad.")]) == 24
    run = R.running_after(P, out["stats"])
    for k, v in run.items():
        np.testing.assert_allclose(v.numpy(), c["step1." + k], rtol=1e-5, atol=1e-7, err_msg=k)


def test_fixture_affinity_and_draw_arrays_follow_the_script(g):
    """The fixture's epoch-0 affinities equal the sparse float64 affinity of its own embeddings, and the three plotted arrays are the
    ones aegis.py builds from them (normal nodes, affinity2[:500], 50 lowest at the shuffled 'anomalous' indices)."""
    G = _gen()
    for tag in ("a", "b"):
        c = _case(g, tag)
        n = int(c["n"])
        _, raw = R.a_hat(c["rowptr"], c["col"], n)
        arrs = G.draw_arrays(c["affinity1_0"], c["affinity2_0"], c["all_idx"], c["ano"])
        for i, a in enumerate(arrs):
            np.testing.assert_array_equal(a, c[f"draw{i}_0"])
        assert len(arrs[2]) == min(50, int(c["ano"].sum()))
        np.testing.assert_allclose(R.affinity(c["z"], raw), c["affinity1_0"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(R.affinity(c["z_gen"], raw), c["affinity2_0"], rtol=1e-5, atol=1e-6)
