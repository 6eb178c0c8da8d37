"""Float64 restatement of the full-graph GAAN forward (model_gaan.py:269-336) on the sparse edge set, the yardstick of
tests/test_gaan_cpu.py and the GPU tests.  Parameters are a dict name -> float64 tensor (the reference's state_dict names); batch norm
runs in training mode with torch's formulas (biased variance normalises, the unbiased one feeds the running statistics)."""
import numpy as np
import scipy.sparse as sp
import torch

EPS, MOM = 1e-5, 0.1


def a_hat(rowptr, col, n):
    """normalize_adj(A) + I of the reference (utils.py:47-54) as scipy CSR (float64), stored zeros kept."""
    from ggad_amd.utils import normalize_adj
    a = sp.csr_matrix((np.ones(len(col)), np.asarray(col), np.asarray(rowptr)), shape=(n, n))
    return sp.csr_matrix(normalize_adj(a) + sp.eye(n))


def params64(state: dict, requires_grad=True) -> dict:
    out = {}
    for k, v in state.items():
        t = torch.as_tensor(np.asarray(v))
        if t.is_floating_point():
            t = t.double()
            if requires_grad and "running" not in k:
                t.requires_grad_(True)
        out[k] = t
    return out


def bn_train(h, g, b):
    """Training-mode BatchNorm1d: (y, batch mean, unbiased batch variance)."""
    mean = h.mean(0)
    var = h.var(0, unbiased=False)
    y = (h - mean) / torch.sqrt(var + EPS) * g + b
    return y, mean.detach(), h.detach().var(0, unbiased=True)


def mlp(P, pfx, h):
    """Linear -> BatchNorm1d -> ReLU -> Linear; returns (out, (batch mean, unbiased batch variance))."""
    h = h @ P[f"{pfx}.lins.0.weight"].T + P[f"{pfx}.lins.0.bias"]
    y, m, v = bn_train(h, P[f"{pfx}.norms.0.module.weight"], P[f"{pfx}.norms.0.module.bias"])
    return torch.relu(y) @ P[f"{pfx}.lins.1.weight"].T + P[f"{pfx}.lins.1.bias"], (m, v)


def sigmoid32(d):
    """sigmoid of float64 dots with float32's saturation: 1 / (1 + exp(-d)) with exp and the division rounded to float32 (exp
    overflows to inf below d = -88.7, 1 + exp rounds to 1 above d = 16.6)."""
    with np.errstate(over="ignore"):
        e = np.exp(-np.asarray(d, dtype=np.float64)).astype(np.float32)
    return np.float32(1) / (np.float32(1) + e)


def edge_terms(a, t):
    """torch's BCE terms (t - 1) max(log1p(-a), -100) - t max(log(a), -100) in float64."""
    with np.errstate(divide="ignore"):
        return -(t * np.maximum(np.log(a), -100.0) + (1 - t) * np.maximum(np.log1p(-a), -100.0))


def edge_loss_ref(emb, z, erow, ecol, g=1.0, f32_sigmoid=True):
    """(loss, BCE(a', 0), BCE(a, 1), dE) in float64 over the edge list; dE = G emb + G^T emb with torch's backward coefficients.
    f32_sigmoid: a and a' rounded as float32 evaluates the sigmoid (what the reference and the kernels compute, and what decides
    the clamps: sigmoid(17) is 1.0f, so its BCE term against 0 is 100, not 17); everything else in float64."""
    emb, z = np.asarray(emb, dtype=np.float64), np.asarray(z, dtype=np.float64)
    erow, ecol = np.asarray(erow), np.asarray(ecol)
    d, dz = np.empty(len(erow)), np.empty(len(erow))
    for lo in range(0, len(erow), 1 << 20):                          # (in blocks: T-Finance has 21 M entries)
        r, c = erow[lo:lo + (1 << 20)], ecol[lo:lo + (1 << 20)]
        d[lo:lo + len(r)] = np.einsum("ij,ij->i", emb[r], emb[c])
        dz[lo:lo + len(r)] = np.einsum("ij,ij->i", z[r], z[c])
    if f32_sigmoid:
        a, af = sigmoid32(d).astype(np.float64), sigmoid32(dz).astype(np.float64)
    else:
        a, af = 1.0 / (1.0 + np.exp(-d)), 1.0 / (1.0 + np.exp(-dz))
    m = len(erow)
    lf = edge_terms(af, 0.0).mean()
    lr = edge_terms(a, 1.0).mean()
    g0 = g / 2.0 / m
    c = g0 * (a - 1.0) / np.maximum((1.0 - a) * a, 1e-12) * (1.0 - a) * a
    n = emb.shape[0]
    G = sp.csr_matrix((c, (erow, ecol)), shape=(n, n))
    dE = G @ emb + G.T @ emb
    return (lf + lr) / 2.0, lf, lr, np.asarray(dE)


class _EdgeLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb, z, erow, ecol):
        loss, lf, lr, _ = edge_loss_ref(emb.detach().numpy(), z.detach().numpy(), erow, ecol)
        ctx.save_for_backward(emb, z)
        ctx.e = (erow, ecol)
        return torch.tensor([loss, lf, lr], dtype=torch.float64)

    @staticmethod
    def backward(ctx, g):
        emb, z = ctx.saved_tensors
        dE = edge_loss_ref(emb.detach().numpy(), z.detach().numpy(), *ctx.e, g=float(g[0]))[3]
        return torch.from_numpy(dE), None, None, None


def forward(P, x, noise, erow, ecol, idx_train, idx_test):
    """dict with x_ (x_hat), emb, z, loss, loss_f (BCE(a', 0)), loss_r (BCE(a, 1)), loss_g, score and the batch statistics of the three
    batch-norm calls (gen; dis on x, then on x_).  The loss's gradient is taken only through emb, as the reference detaches a'."""
    st = {}
    x_, st["gen"] = mlp(P, "generator", noise)
    emb, st["dis_x"] = mlp(P, "discriminator", x)
    z, st["dis_z"] = mlp(P, "discriminator", x_)
    vals = _EdgeLoss.apply(emb, z.detach(), np.asarray(erow), np.asarray(ecol))
    r = torch.as_tensor(np.asarray(idx_train, dtype=np.int64))
    loss_g = torch.mean(torch.sqrt(torch.sum((x[r] - x_[r]) ** 2, 1)))
    t = torch.as_tensor(np.asarray(idx_test, dtype=np.int64))
    score = torch.sqrt(torch.sum((x[t] - x_[t]) ** 2, 1))
    return dict(x_=x_, emb=emb, z=z, loss=vals[0] * 1.0, loss_f=vals[1], loss_r=vals[2], loss_g=loss_g, score=score, stats=st)


def running_after(P, stats):
    """Running statistics after one forward: the generator's once, the discriminator's twice (x, then x_)."""
    out = {}
    for pfx, calls in (("generator", ("gen",)), ("discriminator", ("dis_x", "dis_z"))):
        rm, rv = P[f"{pfx}.norms.0.module.running_mean"].clone(), P[f"{pfx}.norms.0.module.running_var"].clone()
        for key in calls:
            m, v = stats[key]
            rm, rv = (1 - MOM) * rm + MOM * m, (1 - MOM) * rv + MOM * v
        out[f"{pfx}.norms.0.module.running_mean"] = rm
        out[f"{pfx}.norms.0.module.running_var"] = rv
    return out
