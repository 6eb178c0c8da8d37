"""Float64 restatement of the full-graph AEGIS forward (model_AEGIS.py:185-239) on a sparse A_hat, the yardstick of
tests/test_aegis_cpu.py and the GPU tests.  Parameters are a dict name -> float64 tensor (the reference's state_dict names); batch
norm runs in training mode with torch's formulas (biased variance normalises, the unbiased one feeds the running statistics)."""
import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F

EPS, MOM = 1e-5, 0.1


def a_hat(rowptr, col, n):
    """normalize_adj(A) + I of the reference (utils.py:47-54) as a float64 sparse tensor, and raw = A + I as scipy CSR."""
    a = sp.csr_matrix((np.ones(len(col)), np.asarray(col), np.asarray(rowptr)), shape=(n, n))
    rs = np.asarray(a.sum(1)).reshape(-1)
    with np.errstate(divide="ignore"):
        d = np.power(rs, -0.5)
    d[np.isinf(d)] = 0.0
    an = (sp.diags(d) @ a @ sp.diags(d)).T.tocsr() + sp.eye(n)          # (A D^-1/2)^T D^-1/2, as utils.normalize_adj writes it
    an = sp.coo_matrix(an)
    t = torch.sparse_coo_tensor(np.vstack([an.row, an.col]), an.data, (n, n), dtype=torch.float64).coalesce()
    return t, (a + sp.eye(n)).tocsr()


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


def forward(P, x, A, noise, idx_train, idx_test):
    """dict with x_gen, z, z_gen, z_dec, score (idx_test rows of the 2N-row logits), p_gen, loss_g, loss_ae and the batch statistics
    of the three batch-norm calls (gen, dis_all, dis_gen)."""
    def gcn(name, h):
        return F.prelu(torch.sparse.mm(A, h @ P[name + ".fc.weight"].T) + P[name + ".bias"], P[name + ".act.weight"])

    def lin(pfx, k, h):
        return h @ P[f"{pfx}.lins.{k}.weight"].T + P[f"{pfx}.lins.{k}.bias"]

    def norm(pfx):
        return P[f"{pfx}.norms.0.module.weight"], P[f"{pfx}.norms.0.module.bias"]

    st = {}
    y, m, v = bn_train(lin("generator", 0, noise), *norm("generator"))
    st["gen"] = (m, v)
    x_gen = lin("generator", 1, torch.relu(y))
    z_gen = gcn("gcn_enc2", gcn("gcn_enc1", x_gen))
    z = gcn("gcn_enc2", gcn("gcn_enc1", x))
    z_dec = gcn("gcn_dec2", gcn("gcn_dec1", z))
    h_all = lin("discriminator2", 0, torch.cat([z, z_gen], 0))
    y, m, v = bn_train(h_all, *norm("discriminator2"))
    st["dis_all"] = (m, v)
    logits = torch.sigmoid(lin("discriminator2", 1, torch.sigmoid(y)))
    y, m, v = bn_train(lin("discriminator2", 0, z_gen), *norm("discriminator2"))
    st["dis_gen"] = (m, v)
    p_gen = torch.sigmoid(lin("discriminator2", 1, torch.sigmoid(y)))[:, 0]
    loss_g = torch.mean(-torch.clamp(torch.log1p(-p_gen), min=-100.0))
    r = torch.as_tensor(np.asarray(idx_train, dtype=np.int64))
    loss_ae = torch.mean(torch.sqrt(torch.sum((x[r] - z_dec[r]) ** 2, 1)))
    return dict(x_gen=x_gen, z=z, z_gen=z_gen, z_dec=z_dec, score=logits[torch.as_tensor(np.asarray(idx_test, dtype=np.int64)), 0],
                p_gen=p_gen, loss_g=loss_g, loss_ae=loss_ae, stats=st)


def running_after(P, stats, k_calls=("gen", "dis_all", "dis_gen")):
    """Running statistics after one forward: generator once, discriminator2 twice (2N rows, then N)."""
    out = {}
    rm, rv = P["generator.norms.0.module.running_mean"].clone(), P["generator.norms.0.module.running_var"].clone()
    m, v = stats["gen"]
    out["generator.norms.0.module.running_mean"] = (1 - MOM) * rm + MOM * m
    out["generator.norms.0.module.running_var"] = (1 - MOM) * rv + MOM * v
    rm, rv = P["discriminator2.norms.0.module.running_mean"].clone(), P["discriminator2.norms.0.module.running_var"].clone()
    for key in ("dis_all", "dis_gen"):
        m, v = stats[key]
        rm, rv = (1 - MOM) * rm + MOM * m, (1 - MOM) * rv + MOM * v
    out["discriminator2.norms.0.module.running_mean"] = rm
    out["discriminator2.norms.0.module.running_var"] = rv
    return out


def affinity(emb, raw_csr):
    """aegis.py:126-146 for one N-row block, without the N x N matrix: r_inv_j sum_i raw_ij <e_i, e_j>."""
    e = np.asarray(emb, dtype=np.float64)
    nrm = np.linalg.norm(e, axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        inv = 1.0 / nrm
    inv[np.isinf(inv)] = 0.0
    en = e * inv
    colsum = np.asarray(raw_csr.sum(0)).reshape(-1)
    with np.errstate(divide="ignore"):
        r_inv = 1.0 / colsum
    r_inv[np.isinf(r_inv)] = 0.0
    s = raw_csr.T.tocsr() @ en
    return np.sum(en * s, 1) * r_inv
