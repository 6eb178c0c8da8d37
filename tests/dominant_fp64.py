"""Float64 restatement of the full-graph DOMINANT epoch (model_domaint.py:96-210), the yardstick of tests/test_dominant_cpu.py and the
GPU tests.  Parameters are a dict name -> float64 tensor (the reference's state_dict names)."""
import numpy as np
import torch


def params64(state: dict, requires_grad=True) -> dict:
    out = {}
    for k, v in state.items():
        t = torch.as_tensor(np.asarray(v)).double()
        if requires_grad:
            t.requires_grad_(True)
        out[k] = t
    return out


def emb(P, x, op):
    """GCN(relu(dense_stru(x))) with the dense operator op = D^-1/2 P^T D^-1/2 (float64 numpy or tensor)."""
    op = torch.as_tensor(op, dtype=torch.float64)
    h = torch.relu(x @ P["dense_stru.weight"].T + P["dense_stru.bias"])
    z = torch.relu(op @ (h @ P["gat_layer.convs.0.lin.weight"].T) + P["gat_layer.convs.0.bias"])
    return op @ (z @ P["gat_layer.convs.1.lin.weight"].T) + P["gat_layer.convs.1.bias"]


def forward(P, x, idx_train, idx_test):
    """(loss, score): loss = mean_{i in idx_train} ||x_i - x_i_hat||, score_k = ||x_k - x_k_hat||, on the listed rows only."""
    tr, te = torch.as_tensor(np.asarray(idx_train, dtype=np.int64)), torch.as_tensor(np.asarray(idx_test, dtype=np.int64))

    def err(rows):
        xr = x[rows]
        h = torch.relu(xr @ P["dense_attr_1.weight"].T + P["dense_attr_1.bias"])
        xh = h @ P["dense_attr_2.weight"].T + P["dense_attr_2.bias"]
        return torch.sqrt(((xr - xh) ** 2).sum(1))

    return err(tr).mean(), err(te)


def ae_grads(P, x, idx_train, idx_test):
    """(loss, score, {name: grad}) of the four autoencoder tensors."""
    loss, score = forward(P, x, idx_train, idx_test)
    names = ["dense_attr_1.weight", "dense_attr_1.bias", "dense_attr_2.weight", "dense_attr_2.bias"]
    grads = torch.autograd.grad(loss, [P[k] for k in names])
    return loss.detach(), score.detach(), dict(zip(names, grads))
