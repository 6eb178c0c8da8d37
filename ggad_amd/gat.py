"""GAT layer of the full-graph AnomalyDAE model on the kernels of csrc/anomalydae.hip.

    GATConv(in_channels, out_channels).forward(x, adj) -> (N, out_channels)          model_AnomalyDAE.py:123,257

A drop-in for the `torch_geometric.nn.GATConv` (version 2.1, `requirements.txt:8`) the reference builds with its defaults:
one head, concat, negative slope 0.2, no dropout, stored self loops removed and one self loop added per node, bias.  Any
other argument raises.  Parameter names, shapes and the order of RNG draws are PyG's: `lin_src` (no bias, glorot; `lin_dst`
is the same module) is drawn by its own constructor and twice more by `reset_parameters`, then `att_src`, `att_dst`
(glorot, shape (1, 1, out)), and `bias` is zero.  `adj` is a `FullGraphAdj` (or the reference's dense adjacency): edges run
from source r to target i where A_hat[r, i] > 0, as `neighList_to_edgeList` lists them.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import call, ptr
from .fullgraph import FullGraphAdj, _dev_i32, gemm


def _glorot_(t: torch.Tensor):
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    t.data.uniform_(-a, a)


class _GlorotLinear(nn.Module):
    """torch_geometric.nn.dense.Linear(in, out, bias=False, weight_initializer='glorot')."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels))
        self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        _glorot_(self.weight)


def gat_structs(adj: FullGraphAdj) -> dict:
    """A_hat (source rows), A_hat^T (target rows) and tmap[e] = index in A_hat^T of entry e of A_hat; cached on `adj`."""
    cache = adj.__dict__.setdefault("_adae", {})
    s = cache.get("gat")
    if s is None:
        import scipy.sparse as sp
        a = adj.A.host
        b = sp.csr_matrix((np.arange(a.nnz, dtype=np.int64), a.indices, a.indptr), shape=a.shape)
        bt = b.T.tocsr()
        bt.sort_indices()
        if not (np.array_equal(bt.indptr, adj.At.host.indptr) and np.array_equal(bt.indices, adj.At.host.indices)):
            raise RuntimeError("A_hat^T of the adjacency does not match the transposed entry map")
        tmap = np.empty(a.nnz, dtype=np.int32)
        tmap[bt.data] = np.arange(a.nnz, dtype=np.int32)
        s = cache["gat"] = dict(tmap=_dev_i32(tmap, adj.dev), n_slots=int(a.nnz) + adj.n)
    return s


class GatFn(torch.autograd.Function):
    """z = GAT(h W^T) on the adjacency; backward through the target-side and source-side edge passes."""

    @staticmethod
    def forward(ctx, h, weight, att_src, att_dst, bias, adj: FullGraphAdj):
        gat_structs(adj)                                                   # host-built once, before any captured epoch
        n, F = h.shape[0], weight.shape[0]
        dev = h.device
        y = gemm(h, weight, False, True)                                   # lin_src(x)
        a_s, a_d = att_src.reshape(-1).contiguous(), att_dst.reshape(-1).contiguous()
        als = torch.empty(n, dtype=torch.float32, device=dev)
        ald = torch.empty_like(als)
        call("ggad_adae_gat_alpha_f32", ptr(y), ptr(a_s), ptr(a_d), n, F, ptr(als), ptr(ald))
        z = torch.empty(n, F, dtype=torch.float32, device=dev)
        rmax, rsum = torch.empty_like(als), torch.empty_like(als)
        At = adj.At
        call("ggad_adae_gat_fwd_f32", ptr(At.rowptr), ptr(At.col), ptr(At.val), ptr(y), ptr(als), ptr(ald),
             ptr(bias) if bias is not None else 0, n, F, ptr(z), ptr(rmax), ptr(rsum))
        ctx.save_for_backward(h, weight, a_s, a_d, y, als, ald, rmax, rsum)
        ctx.adj, ctx.has_bias = adj, bias is not None
        ctx.att_shape = att_src.shape
        return z

    @staticmethod
    def backward(ctx, g):
        h, weight, a_s, a_d, y, als, ald, rmax, rsum = ctx.saved_tensors
        adj = ctx.adj
        st = gat_structs(adj)
        g = g.contiguous()
        n, F = y.shape
        dev = y.device
        dpre = torch.empty(st["n_slots"], dtype=torch.float32, device=dev)
        dals, dald = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        dy = torch.empty(n, F, dtype=torch.float32, device=dev)
        A, At = adj.A, adj.At
        call("ggad_adae_gat_bwd_f32", ptr(At.rowptr), ptr(At.col), ptr(At.val), ptr(A.rowptr), ptr(A.col), ptr(A.val), ptr(st["tmap"]),
             ptr(y), ptr(als), ptr(ald), ptr(rmax), ptr(rsum), ptr(a_s), ptr(a_d), ptr(g), n, F, ptr(dpre), ptr(dals), ptr(dald),
             ptr(dy))
        da_s, da_d = colsum(y, dals), colsum(y, dald)
        db = colsum(g) if ctx.has_bias else None
        dw = gemm(dy, h, True, False)                                      # dW = dy^T h
        dh = gemm(dy, weight, False, False) if ctx.needs_input_grad[0] else None
        return dh, dw, da_s.view(ctx.att_shape), da_d.view(ctx.att_shape), db, None


def colsum(M: torch.Tensor, w: torch.Tensor = None) -> torch.Tensor:
    """out[f] = sum_r w[r] M[r, f] (w None: 1), fixed summation order."""
    M = M.contiguous()
    F = M.shape[1]
    ws = torch.empty(int(_lib.load().ggad_adae_colsum_workspace_elems(F)), dtype=torch.float32, device=M.device)
    out = torch.empty(F, dtype=torch.float32, device=M.device)
    call("ggad_adae_colsum_f32", ptr(M), ptr(w), M.shape[0], F, ptr(out), ptr(ws))
    return out


class GATConv(nn.Module):
    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True,
                 edge_dim=None, fill_value="mean", bias=True, **kwargs):
        super().__init__()
        if (heads, concat, negative_slope, dropout, add_self_loops, edge_dim, fill_value, bias) != (1, True, 0.2, 0.0, True, None,
                                                                                                      "mean", True) or kwargs:
            raise ValueError("ggad_amd.gat.GATConv implements the torch_geometric defaults the reference uses only "
                             "(heads=1, concat, slope 0.2, no dropout, self loops added, no edge features, bias)")
        if not isinstance(in_channels, int) or in_channels <= 0:
            raise ValueError("in_channels must be a positive int (lazy or bipartite inputs are not supported)")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, 1
        self.lin_src = _GlorotLinear(in_channels, out_channels)
        self.lin_dst = self.lin_src
        self.att_src = nn.Parameter(torch.empty(1, 1, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, 1, out_channels))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        self.lin_src.reset_parameters()
        self.lin_dst.reset_parameters()
        _glorot_(self.att_src)
        _glorot_(self.att_dst)
        self.bias.data.fill_(0.0)

    def forward(self, x, adj):
        from .model import as_full_adj
        fa = as_full_adj(adj, self.bias.device)
        if x.dim() != 2 or x.shape[0] != fa.n:
            raise ValueError("GATConv expects (N, in_channels) node features on the adjacency's N nodes")
        return GatFn.apply(x.contiguous(), self.lin_src.weight, self.att_src, self.att_dst, self.bias, fa)
