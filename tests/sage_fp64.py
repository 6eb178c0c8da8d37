"""Restatement of one GraphSAGE step on a given sample table (reference src/graphsage.py:19-154), in torch on the CPU at a chosen
precision: the float64 yardstick of tests/test_sage_device_gpu.py, and -- evaluated in float32 -- the measure of what float32
arithmetic in another summation order costs.  The sample table is an input, so only arithmetic is compared."""
import numpy as np
import torch

KEYS = ("combined", "emb", "scores", "loss", "dscores", "grad.enc", "grad.cls")


def evaluate(feat, nodes, nbr, cnt, w_enc, w_cls, labels, dtype):
    """combined = [x_v || sum_j x_nbr[j] / cnt] (a row of length 0: 0 * (1 / 0) = NaN), emb = relu(combined W_enc^T), scores =
    emb W_cls^T; with labels the mean cross entropy, dscores = d loss / d scores and both weight gradients."""
    x = torch.from_numpy(np.asarray(feat)).to(dtype)
    we = torch.from_numpy(np.asarray(w_enc)).to(dtype).requires_grad_(True)
    wc = torch.from_numpy(np.asarray(w_cls)).to(dtype).requires_grad_(True)
    nbr_t = torch.from_numpy(np.asarray(nbr)).long()
    cnt_t = torch.from_numpy(np.asarray(cnt)).long()
    k = nbr_t.shape[1]
    mask = torch.arange(k)[None, :] < cnt_t[:, None]
    inv = 1.0 / cnt_t.to(dtype)
    rows = x[torch.where(mask, nbr_t, torch.zeros_like(nbr_t))]
    wgt = mask.to(dtype) * inv[:, None]
    neigh = (rows * wgt[:, :, None]).sum(1)
    combined = torch.cat([x[torch.from_numpy(np.asarray(nodes)).long()], neigh], dim=1)
    emb = torch.relu(combined @ we.t())
    scores = emb @ wc.t()
    out = {"combined": combined, "emb": emb, "scores": scores}
    if labels is not None:
        scores.retain_grad()
        loss = torch.nn.functional.cross_entropy(scores, torch.from_numpy(np.asarray(labels)).long())
        loss.backward()
        out.update({"loss": loss.reshape(1), "dscores": scores.grad, "grad.enc": we.grad, "grad.cls": wc.grad})
    return {k_: v.detach().to(torch.float64).numpy().copy() for k_, v in out.items()}
