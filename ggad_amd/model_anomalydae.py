"""Full-graph AnomalyDAE comparison model -- drop-in for the reference's `model_AnomalyDAE.py` on the kernels of
csrc/anomalydae.hip.

    Model(n_in, n_h, activation, negsamp_round, readout)
        .forward(seq1, adj, idx_train, idx_test, sparse=False) -> (loss, score_test)            model_AnomalyDAE.py:115,269

Same constructor order and state_dict keys as the reference (dense_stru, gat_layer, dense_attr_1 / _2, then the unused
discriminator, which still consumes the RNG).  The linear layers run on `fullgraph.gemm` with its bias / ReLU epilogue, the GAT
layer is `ggad_amd.gat.GATConv`, and `double_recon_loss` is the fused structure loss: s_ = sigmoid(z z^T) is never formed, its
rows are reduced inside the kernels.  Documented deviation: `model_enc` returns (x_hat, z) instead of (x_hat, s_).
`adj` is a `FullGraphAdj` or the reference's dense adjacency (converted once, `model.as_full_adj`); the row lists must be
duplicate-free, as the reference's are.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import call, ptr
from .fullgraph import FullGraphAdj, _capturing, _dev_f32, _dev_i32, gemm
from .gat import GATConv, colsum
from .model import AvgReadout, Discriminator, MaxReadout, MinReadout, WSReadout, as_full_adj


class LinearBiasFn(torch.autograd.Function):
    """y = [relu](x W^T + b): nn.Linear with bias on the matrix cores (bias and ReLU in the GEMM's epilogue)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu: bool):
        y = gemm(x, weight, False, True, bias=bias, relu=relu)
        ctx.save_for_backward(x, weight, y)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        g = g.contiguous()
        if ctx.relu:
            dz = torch.empty_like(g)
            call("ggad_relu_bwd_f32", ptr(g), ptr(y), g.numel(), ptr(dz))
        else:
            dz = g
        dx = gemm(dz, weight, False, False) if ctx.needs_input_grad[0] else None
        return dx, gemm(dz, x, True, False), colsum(dz), None


def row_structs(adj: FullGraphAdj, idx) -> dict:
    """Device structures of one row list of the loss: the rows (int64), the compact CSR of A_hat[rows, :], the position of every
    node in the list and the same entries grouped by column.  Cached on `adj` by contents; a list holding a node twice raises.
    The cache keeps at most 16 lists, except that a list looked up during a stream capture is pinned and never evicted: the
    captured graph holds raw pointers to its structures, and nothing else keeps them alive."""
    arr = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
    cache = adj.__dict__.setdefault("_adae", {})
    key = ("rows", arr.size, hash(arr.tobytes()))
    s = cache.get(key)
    if s is not None and np.array_equal(s["host"], arr):
        if _capturing(adj.dev):
            s["pinned"] = True
        return s
    if arr.size == 0:
        raise ValueError("the loss needs at least one row")
    if arr.min() < 0 or arr.max() >= adj.n:
        raise ValueError("row index out of range")
    if len(np.unique(arr)) != arr.size:
        raise ValueError("a row list of the AnomalyDAE loss holds a node twice: the lists must be duplicate-free")
    sub = adj.A.host[arr, :]
    nr, n = arr.size, adj.n
    pos = np.full(n, -1, dtype=np.int32)
    pos[arr] = np.arange(nr, dtype=np.int32)
    rl = np.repeat(np.arange(nr, dtype=np.int64), np.diff(sub.indptr))
    order = np.lexsort((rl, sub.indices))                                   # by column, then by row position
    tptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(sub.indices, minlength=n), out=tptr[1:])
    dev = adj.dev
    s = dict(host=arr, n_rows=nr, rows=torch.from_numpy(arr).to(dev), rptr=_dev_i32(sub.indptr, dev), rcol=_dev_i32(sub.indices, dev),
             rval=_dev_f32(sub.data.astype(np.float32), dev), nnz=int(sub.nnz), pos=_dev_i32(pos, dev), tptr=_dev_i32(tptr, dev),
             trow=_dev_i32(rl[order], dev), tedge=_dev_i32(order, dev), pinned=_capturing(dev))
    evictable = [k for k in cache if isinstance(k, tuple) and k[0] == "rows" and not cache[k]["pinned"]]
    if len(evictable) >= 16:
        for k in evictable:
            del cache[k]
    cache[key] = s
    return s


def _stru_fwd(z, xhat, x, rs, s_edge, loss):
    n, F = z.shape
    nr = rs["n_rows"]
    dev = z.device
    ws = torch.empty(int(_lib.load().ggad_adae_stru_fwd_workspace_elems(nr, n)), dtype=torch.float32, device=dev)
    attr, stru, score = (torch.empty(nr, dtype=torch.float32, device=dev) for _ in range(3))
    call("ggad_adae_stru_fwd_f32", ptr(z), n, F, ptr(rs["rows"]), nr, ptr(rs["rptr"]), ptr(rs["rcol"]), ptr(rs["rval"]), ptr(x),
         ptr(xhat), ptr(ws), ptr(s_edge), ptr(attr), ptr(stru), ptr(score), ptr(loss))
    return attr, stru, score


class ReconLossFn(torch.autograd.Function):
    """(loss, score) of `double_recon_loss` on the rows of `rs` (model_AnomalyDAE.py:283-292): weight 0.5, squared errors."""

    @staticmethod
    def forward(ctx, z, xhat, x, rs):
        loss = torch.empty(1, dtype=torch.float32, device=z.device)
        s_edge = torch.empty(max(rs["nnz"], 1), dtype=torch.float32, device=z.device)
        attr, stru, score = _stru_fwd(z, xhat, x, rs, s_edge, loss)
        ctx.save_for_backward(z, xhat, x, attr, stru, s_edge)
        ctx.rs = rs
        ctx.mark_non_differentiable(score)
        return loss[0], score

    @staticmethod
    def backward(ctx, g, _gs):
        z, xhat, x, attr, stru, s_edge = ctx.saved_tensors
        rs = ctx.rs
        n, F = z.shape
        nr = rs["n_rows"]
        g = g.reshape(1).contiguous()
        dz = dxhat = None
        if ctx.needs_input_grad[0]:
            ws = torch.empty(int(_lib.load().ggad_adae_stru_bwd_workspace_elems(nr, n, F)), dtype=torch.float32, device=z.device)
            dz = torch.empty_like(z)
            call("ggad_adae_stru_bwd_f32", ptr(z), n, F, ptr(rs["rows"]), nr, ptr(rs["rptr"]), ptr(rs["rcol"]), ptr(rs["rval"]),
                 ptr(s_edge), ptr(rs["pos"]), ptr(rs["tptr"]), ptr(rs["trow"]), ptr(rs["tedge"]), ptr(stru), ptr(g), ptr(ws), ptr(dz))
        if ctx.needs_input_grad[1]:
            dxhat = torch.zeros_like(xhat)
            call("ggad_adae_attr_bwd_f32", ptr(x), ptr(xhat), ptr(rs["rows"]), nr, F, ptr(attr), ptr(g), ptr(dxhat))
        return dz, dxhat, None, None


def recon_loss(z, xhat, x, adj: FullGraphAdj, idx):
    """(loss, score) of the reference's double_recon_loss on the rows `idx` of (x, x_hat, A_hat, sigmoid(z z^T))."""
    if z.shape[1] > 768:
        raise ValueError("the fused AnomalyDAE loss takes at most 768 features")
    return ReconLossFn.apply(z.contiguous(), xhat.contiguous(), x.contiguous(), row_structs(adj, idx))


def recon_score(z, xhat, x, adj: FullGraphAdj, idx):
    """score over the rows `idx` (the test scoring of the reference's forward): the forward kernels with no backward."""
    with torch.no_grad():
        return _stru_fwd(z.contiguous(), xhat.contiguous(), x.contiguous(), row_structs(adj, idx), None, None)[2]


class Model(nn.Module):
    def __init__(self, n_in, n_h, activation, negsamp_round, readout):
        super().__init__()
        self.read_mode = readout
        self.dense_stru = nn.Linear(n_in, n_h)
        self.gat_layer = GATConv(n_h, n_in)
        self.dense_attr_1 = nn.Linear(n_in, n_h)
        self.dense_attr_2 = nn.Linear(n_h, n_in)
        self.act = nn.ReLU()
        self.dropout = 0.
        if readout == "max":
            self.read = MaxReadout()
        elif readout == "min":
            self.read = MinReadout()
        elif readout == "avg":
            self.read = AvgReadout()
        elif readout == "weighted_sum":
            self.read = WSReadout()
        self.disc = Discriminator(n_h, negsamp_round)

    def model_enc(self, x, adj):
        """(x_hat, z): the attribute reconstruction and the GAT embedding (the reference returns sigmoid(z z^T) as its second
        output; the loss kernels consume z instead)."""
        fa = as_full_adj(adj, self.dense_stru.weight.device)
        h = LinearBiasFn.apply(x, self.dense_stru.weight, self.dense_stru.bias, True)                  # :253-255
        z = self.gat_layer(h, fa)                                                                        # :257
        a = LinearBiasFn.apply(x, self.dense_attr_1.weight, self.dense_attr_1.bias, True)                # :261-264
        xhat = LinearBiasFn.apply(a, self.dense_attr_2.weight, self.dense_attr_2.bias, False)            # :265
        return xhat, z

    def train_forward(self, seq1, adj, idx_train):
        """(loss, z, x_hat) of one training forward: what the script scores its test rows from."""
        dev = self.dense_stru.weight.device
        fa = as_full_adj(adj, dev)
        x = seq1.reshape(-1, seq1.shape[-1]).to(dev).contiguous()
        xhat, z = self.model_enc(x, fa)
        loss, _ = recon_loss(z, xhat, x, fa, idx_train)
        return loss, z, xhat

    def forward(self, seq1, adj, idx_train, idx_test, sparse=False):
        dev = self.dense_stru.weight.device
        fa = as_full_adj(adj, dev)
        x = seq1.reshape(-1, seq1.shape[-1]).to(dev).contiguous()
        xhat, z = self.model_enc(x, fa)
        loss, _ = recon_loss(z, xhat, x, fa, idx_train)                                                  # :283-292
        score_test = recon_score(z.detach(), xhat.detach(), x, fa, idx_test)                             # :293-299
        return loss, score_test
