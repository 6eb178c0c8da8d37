"""float64 restatement of the fused TAM head (`ggad_amd/csrc/tam.hip`, `ggad_amd/tam_utils.py::max_message_fused`) on CSR inputs: a
helper of `test_tam_head_cpu.py` / `test_tam_head_gpu.py`, not a test.

    inv_i = 1 / |e_i| (inf -> 0),  e_hat_i = inv_i e_i
    a_i   = r_inv_i <e_hat_i, sum_{j in R_i} v_ij e_hat_j>
    lo, hi = min a, max a;  d = hi - lo;  n_lo, n_hi = ties;  cnt_i = occurrences of i in idx;  K = len(idx)
    S = sum cnt_i a_i;  N = S - K lo;  loss = -N / d;  m_i = (a_i - lo) / d
    dloss/da_i = -cnt_i / d + [a_i = lo] (K / d - N / d^2) / n_lo + [a_i = hi] (N / d^2) / n_hi
    c_i = g r_inv_i dloss/da_i;  den_i = sum_{j in R_i} v_ij (c_i + c_j) e_hat_j      (R symmetric)
    d_e_i = inv_i (den_i - e_hat_i <e_hat_i, den_i>)
"""
import numpy as np
import scipy.sparse as sp


def tam_head_fp64(rowptr, col, val, r_inv, emb, idx, g=1.0):
    e = np.asarray(emb, dtype=np.float64)
    n = e.shape[0]
    R = sp.csr_matrix((np.asarray(val, dtype=np.float64), np.asarray(col), np.asarray(rowptr)), shape=(n, n))
    r_inv = np.asarray(r_inv, dtype=np.float64)
    nrm = np.sqrt((e * e).sum(1))
    with np.errstate(divide="ignore"):
        inv = 1.0 / nrm
    inv[np.isinf(inv)] = 0.0
    eh = e * inv[:, None]
    a = r_inv * (eh * (R @ eh)).sum(1)
    lo, hi = a.min(), a.max()
    d = hi - lo
    at_lo, at_hi = (a == lo), (a == hi)
    n_lo, n_hi = int(at_lo.sum()), int(at_hi.sum())
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    cnt = np.bincount(idx, minlength=n).astype(np.float64)
    K = float(len(idx))
    S = float((cnt * a).sum())
    N = S - K * lo
    with np.errstate(divide="ignore", invalid="ignore"):
        loss = -N / d
        m = (a - lo) / d
        da = -cnt / d + at_lo * ((K / d - N / d ** 2) / n_lo) + at_hi * ((N / d ** 2) / n_hi)
    c = g * r_inv * da
    Rc = sp.diags(c) @ R + R @ sp.diags(c)                    # v_ij (c_i + c_j)
    den = Rc @ eh
    d_emb = inv[:, None] * (den - eh * (eh * den).sum(1, keepdims=True))
    return dict(inv=inv, a=a, lo=lo, hi=hi, n_lo=n_lo, n_hi=n_hi, S=S, K=K, loss=loss, m=m, da=da, d_emb=d_emb)
