"""Full-graph DOMINANT without a GPU: the drop-in Model's initial state equals the imported reference's (fixture) bit for bit, the
host gcn_norm operator equals the fixture's float64 D^-1/2 P^T D^-1/2, the float64 restatement the GPU tests compare against
(tests/dominant_fp64.py) reproduces the fixture's first epoch, and dominant.py's defaults are the reference's."""
import numpy as np
import pytest
import torch

import dominant_fp64 as R
from conftest import load_golden


@pytest.fixture(scope="module")
def g():
    return load_golden("fullgraph_dominant.npz")


def _case(g, tag):
    return {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + ".")}


def _dense_op(c):
    n = int(c["n"])
    op = np.zeros((n, n))
    op[c["gcn_op_row"], c["gcn_op_col"]] = c["gcn_op_val"]
    return op


def _a_hat(c):
    import scipy.sparse as sp
    from ggad_amd import synth
    from ggad_amd.utils import normalize_adj
    n = int(c["n"])
    return sp.csr_matrix(normalize_adj(synth.csr_to_scipy(c["rowptr"], c["col"], n)) + sp.eye(n))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_initial_state_dict_is_bit_equal_to_the_reference(g, tag):
    from ggad_amd.model_dominant import Model
    c = _case(g, tag)
    torch.manual_seed(int(c["seed"]))
    model = Model(int(c["f"]), int(c["n_h"]), "prelu", 1, "avg")
    sd = model.state_dict()
    ref = {k[5:]: v for k, v in c.items() if k.startswith("init.")}
    assert list(sd) == list(ref)
    assert list(sd)[2:6] == ["gat_layer.convs.0.bias", "gat_layer.convs.0.lin.weight", "gat_layer.convs.1.bias",
                             "gat_layer.convs.1.lin.weight"]
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), ref[k]), k


@pytest.mark.parametrize("tag", ["a", "b"])
def test_gcn_operator_equals_dense_float64(g, tag):
    """Same pattern, values to float32 round-off; graph 'b' is asymmetric with stored zeros, an isolated node and a diagonal-only
    node, where D^-1/2 P^T D^-1/2 differs from the row-normalised A_hat."""
    from ggad_amd.model_dominant import gcn_operator
    c = _case(g, tag)
    A = _a_hat(c)
    op = gcn_operator(A)
    ref = _dense_op(c)
    got = np.asarray(op.todense(), dtype=np.float64)
    assert np.array_equal(got != 0, ref != 0)
    np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0)
    assert float(c["pyg_vs_dense"]) < 1e-12
    if tag == "b":
        n = int(c["n"])
        assert abs(A - A.T).nnz > 0
        assert not np.allclose(ref, np.asarray(A.todense()))
        assert A[n - 1].nnz == 1 and A[n - 2].nnz == 1


@pytest.mark.parametrize("tag", ["a", "b"])
def test_float64_restatement_reproduces_the_fixture(g, tag):
    c = _case(g, tag)
    P = R.params64({k[5:]: v for k, v in c.items() if k.startswith("init.")})
    x = torch.from_numpy(c["features"]).double()
    e = R.emb(P, x, _dense_op(c)).detach().numpy()
    np.testing.assert_allclose(e, c["emb"], rtol=1e-4, atol=1e-5 * np.abs(c["emb"]).max())
    loss, score, grads = R.ae_grads(P, x, c["idx_train"], c["idx_test"])
    assert abs(loss.item() - float(c["loss0"])) <= 1e-5 * abs(float(c["loss0"]))
    np.testing.assert_allclose(score.numpy(), c["score0"], rtol=1e-5, atol=1e-6)
    assert sorted(k[5:] for k in c if k.startswith("grad.")) == sorted(grads)
    for k, gr in grads.items():
        ref = c["grad." + k]
        np.testing.assert_allclose(gr.numpy(), ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max(), err_msg=k)


def test_parse_defaults_match_the_reference():
    import dominant
    table = {"Amazon": (1e-3, 800), "t_finance": (5e-4, 1500), "reddit": (1e-3, 500), "photo": (3e-3, 500), "elliptic": (3e-3, 500)}
    for ds, (lr, ep) in table.items():
        a = dominant.parse(["--dataset", ds])
        assert (a.lr, a.num_epoch) == (lr, ep), ds
    a = dominant.parse([])
    assert a.dataset == "t_finance" and a.embedding_dim == 300 and a.weight_decay == 0.0 and a.seed == 0
    assert dominant.parse(["--dataset", "x", "--lr", "0.1", "--num_epoch", "3"]).num_epoch == 3
    with pytest.raises(SystemExit):
        dominant.parse(["--dataset", "x"])
