"""The float64 restatement of the PC-GNN head (tests/pcgnn_head_fp64.py) against torch's CPU autograd on the expressions of
`ggad_amd/layers.py` (`torch.relu`, `x / norm`, `torch.where(isnan)`, `mean` over an `argwhere` selection, `clamp_min`), and the
`pcgnn_fused` config check.  No GPU."""
import numpy as np
import pytest
import torch

import pcgnn_head_fp64 as H


def _torch_head(t1s, nbs, w, w_cls, labels):
    """Forward and gradients by autograd in float64, written as `InterAgg.forward` (:127-134) and `PCALayer` (:154,161-171) are."""
    t1 = [torch.from_numpy(t).double().requires_grad_(True) for t in t1s]
    nb = [torch.from_numpy(t).double().requires_grad_(True) for t in nbs]
    w = torch.from_numpy(w).double().requires_grad_(True)
    wc = torch.from_numpy(w_cls).double().requires_grad_(True)
    y = torch.from_numpy(labels).long()
    combined = torch.relu(torch.cat(t1, dim=1).mm(w))
    neigh = torch.relu(torch.cat(nb, dim=1).mm(w))
    cn = combined / torch.norm(combined, dim=-1, keepdim=True)
    cn = torch.where(torch.isnan(cn), torch.full_like(cn, 0), cn)
    nn_ = neigh / torch.norm(neigh, dim=-1, keepdim=True)
    nn_ = torch.where(torch.isnan(nn_), torch.full_like(nn_, 0), nn_)
    affinity = (nn_ * cn).sum(1)
    scores = combined.mm(wc.t())
    loss_cls = torch.nn.CrossEntropyLoss()(scores, y)
    a0 = torch.mean(affinity[torch.argwhere(y == 0)], 0)
    a1 = torch.mean(affinity[torch.argwhere(y == 1)], 0)
    con = (1 - (a0 - a1)).clamp_min(min=0)
    total = loss_cls + 5 * con
    total.backward()
    out = {"scores": scores, "affinity": affinity, "loss": torch.cat([total.reshape(1), con.reshape(1)]), "d_w": w.grad, "d_cls": wc.grad}
    for r in range(3):
        out[f"d_t1_{r}"], out[f"d_nb_{r}"] = t1[r].grad, nb[r].grad
    return {k: v.detach().numpy() for k, v in out.items()}


@pytest.mark.parametrize("b,d", [(1, 5), (2, 1), (7, 3), (65, 33), (200, 64)])
def test_restatement_equals_torch_float64_autograd(b, d):
    """Every label case and both dead rows: forward, loss pair and the eight gradients agree to float64 rounding, NaN where torch has
    NaN (the loss pair of a one-class batch) and nowhere else."""
    for name, t1s, nbs, w, w_cls, y in H.cases(b, d, 100 * b + d):
        want = _torch_head(t1s, nbs, w, w_cls, y)
        got = H.head(t1s, nbs, w, w_cls, y, np.float64)
        one_class = len(np.unique(y)) == 1
        assert np.isnan(want["loss"]).all() == one_class, name
        if name == "dead_combined":
            assert (got["combined"][b // 3] == 0).all()
        if name == "dead_neigh":
            assert (got["neigh"][(2 * b) // 3] == 0).all()
        for k in H.KEYS:
            assert got[k].shape == want[k].shape, (name, k)
            if k != "loss":
                assert np.isfinite(want[k]).all(), (name, k)
            scale = 1.0 if np.isnan(want[k]).all() else max(1.0, float(np.nanmax(np.abs(want[k]))))
            np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-12 * scale, equal_nan=True, err_msg=f"{name} {k}")


def test_float32_restatement_is_close_to_float64():
    """The yardstick is the same code in float32: same NaN positions, errors of float32 size."""
    for name, t1s, nbs, w, w_cls, y in H.cases(65, 33, 7):
        a, b = H.head(t1s, nbs, w, w_cls, y, np.float64), H.head(t1s, nbs, w, w_cls, y, np.float32)
        for k in H.KEYS:
            assert b[k].dtype == np.float32 and np.array_equal(np.isnan(a[k]), np.isnan(b[k])), (name, k)
            scale = 1.0 if np.isnan(a[k]).all() else max(1.0, float(np.nanmax(np.abs(a[k]))))
            np.testing.assert_allclose(b[k], a[k], rtol=0, atol=2e-5 * scale, equal_nan=True, err_msg=f"{name} {k}")


def test_pcgnn_fused_without_pcgnn_device_is_a_config_error():
    """`pcgnn_fused: true` needs `pcgnn_device: true`; the handler says so before it touches data or a GPU."""
    from ggad_amd.model_handler import ModelHandler
    cfg = dict(data_name="synthetic", data_dir="", model="PCGNN", seed=72, pcgnn_fused=True)
    with pytest.raises(ValueError, match="pcgnn_fused.*pcgnn_device"):
        ModelHandler(cfg)
    with pytest.raises(ValueError, match="pcgnn_fused.*pcgnn_device"):
        ModelHandler(dict(cfg, pcgnn_device=False))
    with pytest.raises(ValueError, match="data_name"):                     # with both keys the check passes (and the loader objects)
        ModelHandler(dict(cfg, pcgnn_device=True))

