"""Full-graph DOMINANT comparison model -- drop-in for the reference's `model_domaint.py` on the kernels of csrc/dominant.hip.

    Model(n_in, n_h, activation, negsamp_round, readout)
        .forward(seq1, adj, idx_train, idx_test, sparse=False) -> (loss, score_test)         model_domaint.py:193

Same constructor order, draws and state_dict keys as the reference: `dense_stru = Linear(n_in, n_h)`, `gat_layer` (torch_geometric
2.1's `GCN(n_h, n_in, num_layers=2)`: `convs.0` = GCNConv(n_h, n_in), `convs.1` = GCNConv(n_in, n_in), each a bias and a
bias-free glorot `lin` whose weight is drawn twice -- by its own constructor, then by GCNConv.reset_parameters()), `dense_attr_1`,
`dense_attr_2`, then the unused `disc` (its Bilinear still draws).  **The GCN is a restatement of PyG's**, which is absent here.

Forward (dropout p = 0 draws nothing):

- emb = GCN(relu(dense_stru(x))) over gcn_norm's operator D^-1/2 P^T D^-1/2 (P the binary pattern of the positive entries of the
  normalised adjacency, D its column sums; `gcn_operator`), kept as `self.emb`.  It never reaches the loss: it is computed without
  autograd on the GEMM and SpMM kernels (n_in padded to a multiple of 4 with zero weight rows: exact) and cached, keyed on the
  features, the adjacency and the version counters and storages of the dense_stru / gat_layer parameters.  In-place edits through
  `.data` bump no version counter and are not seen; edit under `torch.no_grad()` instead.  dense_stru and gat_layer get no gradient.
- loss = mean_{i in idx_train} ||x_i - x_i_hat||, score_k = ||x_k - x_k_hat|| (k in idx_test), x_ = dense_attr_2(relu(dense_attr_1(x))):
  the fused path (`ggad_dominant_ae_f32`, one launch: forward on the listed rows only, scores, loss and the four gradients) where
  (n_in, n_h) fits it, else the wide path (`wide_loss`: two Linear layers on all rows, `ggad_dominant_recon_f32`).

`adj` is a `FullGraphAdj` (A_hat = normalize_adj(A) + I) or the reference's dense adjacency.  The row lists are duplicate-free each
(they may overlap each other); an empty train list raises.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import call, ptr
from .fullgraph import Csr, FullGraphAdj, _capturing, gemm, spmm, ticket_block
from .model import AvgReadout, Discriminator, MaxReadout, MinReadout, WSReadout, as_full_adj
from .model_anomalydae import LinearBiasFn


# ------------------------------------------------------------------------------------------------ the GCN (PyG 2.1 restated)
def _glorot(t):
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    t.data.uniform_(-a, a)


class PygLinear(nn.Module):
    """torch_geometric.nn.dense.Linear(in, out, bias=False, weight_initializer='glorot'): the constructor draws the weight."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels))
        self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        _glorot(self.weight)


class GCNConv(nn.Module):
    """GCNConv(in, out) of PyG 2.1 with every default: `lin` (drawn by its constructor), `bias` (zeros), then reset_parameters()
    draws lin's weight again.  Parameters only: the model runs the layer on the GEMM / SpMM kernels."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.lin = PygLinear(in_channels, out_channels)
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        self.lin.reset_parameters()
        self.bias.data.zero_()


class GCN(nn.Module):
    """GCN(in_channels, hidden_channels, num_layers) of PyG 2.1 with out_channels None: num_layers GCNConv layers in -> hidden ->
    ... -> hidden, ReLU between them, none after the last, dropout 0."""

    def __init__(self, in_channels, hidden_channels, num_layers):
        super().__init__()
        self.convs = nn.ModuleList([GCNConv(in_channels if k == 0 else hidden_channels, hidden_channels) for k in range(num_layers)])


def gcn_operator(a_hat) -> "sp.csr_matrix":
    """gcn_norm on the reference's edge list, as a CSR (float32 values) of D^-1/2 P^T D^-1/2: P[i, j] = 1 where a_hat[i, j] > 0 (as
    float32: stored zeros and negatives are not edges) plus a loop on every node that lacks one (add_remaining_self_loops),
    deg[j] = sum_i P[i, j] (the target side, edge_index[1]), and out[j] = sum_i deg[i]^-1/2 deg[j]^-1/2 x[i] (source i -> target j)."""
    import scipy.sparse as sp
    a = sp.csr_matrix(a_hat).copy()
    a.sum_duplicates()
    keep = a.data.astype(np.float32) > 0
    coo = a.tocoo()
    row, col = coo.row[keep], coo.col[keep]
    n = a.shape[0]
    has_loop = np.zeros(n, dtype=bool)
    has_loop[row[row == col]] = True
    lp = np.flatnonzero(~has_loop)
    row, col = np.concatenate([row, lp]), np.concatenate([col, lp])
    deg = np.bincount(col, minlength=n).astype(np.float32)
    with np.errstate(divide="ignore"):
        dis = deg ** np.float32(-0.5)
    dis[np.isinf(dis)] = 0
    val = dis[row] * dis[col]
    return sp.csr_matrix((val.astype(np.float32), (col, row)), shape=(n, n))        # row j of M = the sources i of target j


def _gcn_csr(adj: FullGraphAdj) -> Csr:
    c = adj.__dict__.get("_dominant_gcn")
    if c is None:
        c = adj.__dict__["_dominant_gcn"] = Csr(gcn_operator(adj.A.host), adj.dev)
    return c


# ------------------------------------------------------------------------------------------------ row lists
def ae_rows(adj: FullGraphAdj, idx_train, idx_test) -> dict:
    """Device structures of one (train, test) pair, cached on `adj` by contents: rows = [train | test] (int64), pos = position of every
    node in the train list (-1 off it).  Each list must be duplicate-free; the train list must not be empty.  At most 16 pairs are
    kept, except that a pair looked up during a stream capture is pinned: the captured graph holds raw pointers to them."""
    tr = np.ascontiguousarray(np.asarray(idx_train, dtype=np.int64).reshape(-1))
    te = np.ascontiguousarray(np.asarray(idx_test, dtype=np.int64).reshape(-1))
    cache = adj.__dict__.setdefault("_dominant_rows", {})
    key = (tr.size, te.size, hash(tr.tobytes()), hash(te.tobytes()))
    s = cache.get(key)
    if s is not None and np.array_equal(s["train"], tr) and np.array_equal(s["test"], te):
        if _capturing(adj.dev):
            s["pinned"] = True
        return s
    if tr.size == 0:
        raise ValueError("the DOMINANT loss needs at least one train row")
    for arr in (tr, te):
        if arr.size and (arr.min() < 0 or arr.max() >= adj.n):
            raise ValueError("row index out of range")
        if len(np.unique(arr)) != arr.size:
            raise ValueError("a DOMINANT row list holds a node twice: each list must be duplicate-free")
    pos = np.full(adj.n, -1, dtype=np.int32)
    pos[tr] = np.arange(tr.size, dtype=np.int32)
    s = dict(train=tr, test=te, m=int(tr.size), t=int(te.size), rows=torch.from_numpy(np.concatenate([tr, te])).to(adj.dev),
             pos=torch.from_numpy(pos).to(adj.dev), pinned=_capturing(adj.dev))
    evictable = [k for k in cache if not cache[k]["pinned"]]
    if len(evictable) >= 16:
        for k in evictable:
            del cache[k]
    cache[key] = s
    return s


def _scaled(src: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    out = torch.empty_like(src)
    call("ggad_dominant_scale_f32", ptr(src), src.numel(), ptr(g), ptr(out))
    return out


# ------------------------------------------------------------------------------------------------ the fused path
def fused_supported(n_in: int, n_h: int) -> bool:
    return bool(_lib.load().ggad_dominant_ae_supported(int(n_in), int(n_h)))


def fused_ae(x, w1, b1, w2, b2, rs):
    """(loss (1,), score (t,), flat gradient at d loss = 1: [dW1 | dB1 | dW2 | dB2]) by one ggad_dominant_ae_f32 launch."""
    F_, H = x.shape[1], w1.shape[0]
    dev = x.device
    m, t = rs["m"], rs["t"]
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    score = torch.empty(t, dtype=torch.float32, device=dev)
    grads = torch.empty(2 * H * F_ + H + F_, dtype=torch.float32, device=dev)
    HF = H * F_
    ws = torch.empty(int(_lib.load().ggad_dominant_ae_workspace_elems(m, t, F_, H)), dtype=torch.float32, device=dev)
    rc = int(_lib.load().ggad_dominant_ae_f32(ptr(x), F_, ptr(rs["rows"]), m, t, ptr(w1), ptr(b1), ptr(w2), ptr(b2), H,
                                              ptr(score) if t else 0, ptr(loss), grads.data_ptr(), grads.data_ptr() + 4 * HF,
                                              grads.data_ptr() + 4 * (HF + H), grads.data_ptr() + 4 * (2 * HF + H), ptr(ws),
                                              ptr(ticket_block(dev)), _lib.current_stream()))
    if rc == _lib.GGAD_E_UNSUPPORTED:
        raise ValueError("the fused DOMINANT autoencoder does not hold n_in = {}, n_h = {}: use the wide path".format(F_, H))
    _lib.check(rc, "ggad_dominant_ae_f32")
    return loss, score, grads


class FusedAeFn(torch.autograd.Function):
    """(loss, score) of the autoencoder on the rows of `rs`; the gradients come from the same launch, scaled by d loss in backward."""

    @staticmethod
    def forward(ctx, w1, b1, w2, b2, x, rs):
        loss, score, grads = fused_ae(x, w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous(), rs)
        ctx.save_for_backward(grads)
        ctx.shapes = (w1.shape, b1.shape, w2.shape, b2.shape)
        ctx.mark_non_differentiable(score)
        return loss[0], score

    @staticmethod
    def backward(ctx, g, _gs):
        grads, = ctx.saved_tensors
        flat = _scaled(grads, g.reshape(1).contiguous())
        out, o = [], 0
        for s in ctx.shapes:
            k = int(np.prod(s))
            out.append(flat[o:o + k].view(s))
            o += k
        return out[0], out[1], out[2], out[3], None, None


# ------------------------------------------------------------------------------------------------ the wide path
class ReconFn(torch.autograd.Function):
    """(loss, score) from a computed x_ (N x F) by ggad_dominant_recon_f32, dX_ made in the same launch."""

    @staticmethod
    def forward(ctx, xh, x, rs):
        xh = xh.contiguous()
        n, F_ = x.shape
        dev = x.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        score = torch.empty(rs["t"], dtype=torch.float32, device=dev)
        dxh = torch.empty_like(xh)
        ws = torch.empty(int(_lib.load().ggad_dominant_recon_workspace_elems(n, rs["m"], rs["t"])), dtype=torch.float32, device=dev)
        call("ggad_dominant_recon_f32", ptr(x), ptr(xh), n, F_, ptr(rs["rows"]), rs["m"], rs["t"], ptr(rs["pos"]),
             ptr(score) if rs["t"] else 0, ptr(loss), ptr(dxh), ptr(ws), ptr(ticket_block(dev)))
        ctx.save_for_backward(dxh)
        ctx.mark_non_differentiable(score)
        return loss[0], score

    @staticmethod
    def backward(ctx, g, _gs):
        dxh, = ctx.saved_tensors
        return _scaled(dxh, g.reshape(1).contiguous()), None, None


def wide_loss(x, w1, b1, w2, b2, rs):
    """The same (loss, score) as `FusedAeFn` through x_ on all N rows: LinearBiasFn x 2 and ReconFn (any n_in, n_h)."""
    h = LinearBiasFn.apply(x, w1, b1, True)
    xh = LinearBiasFn.apply(h, w2, b2, False)
    return ReconFn.apply(xh, x, rs)


# ------------------------------------------------------------------------------------------------ the model
class Model(nn.Module):
    def __init__(self, n_in, n_h, activation, negsamp_round, readout):
        super().__init__()
        self.read_mode = readout
        self.dense_stru = nn.Linear(n_in, n_h)
        self.gat_layer = GCN(n_h, n_in, num_layers=2)
        self.dense_attr_1 = nn.Linear(n_in, n_h)
        self.dense_attr_2 = nn.Linear(n_h, n_in)
        self.dropout = 0.
        self.act = nn.ReLU()
        if readout == "max":
            self.read = MaxReadout()
        elif readout == "min":
            self.read = MinReadout()
        elif readout == "avg":
            self.read = AvgReadout()
        elif readout == "weighted_sum":
            self.read = WSReadout()
        self.disc = Discriminator(n_h, negsamp_round)                                       # model_domaint.py:124 (unused, draws)
        self.n_in, self.n_h = n_in, n_h
        self.emb = None
        self.force_wide = False                 # run the wide path even where the fused one holds (tests, timing)
        self._emb_cache = None
        self.emb_computations = 0               # how many times the GCN branch ran (the cache's effect, for tests)

    # ------------------------------------------------------------------------------------------------ GCN branch
    def _emb_key(self, x, fa):
        ps = [self.dense_stru.weight, self.dense_stru.bias] + [p for p in self.gat_layer.parameters()]
        return (x.data_ptr(), x._version, tuple(x.shape), id(fa)) + tuple((p.data_ptr(), p._version) for p in ps)

    def gcn_emb(self, x, fa: FullGraphAdj) -> torch.Tensor:
        """GCN(relu(dense_stru(x))) without autograd, cached (see the module docstring)."""
        key = self._emb_key(x, fa)
        c = self._emb_cache
        if c is not None and c["key"] == key:
            return c["emb"]
        fp = (self.n_in + 3) // 4 * 4
        pad = fp - self.n_in
        with torch.no_grad():
            csr = _gcn_csr(fa)
            h = gemm(x, self.dense_stru.weight, False, True, bias=self.dense_stru.bias, relu=True)
            zero = torch.zeros(1, dtype=torch.float32, device=x.device)
            c0, c1 = self.gat_layer.convs[0], self.gat_layer.convs[1]
            w0 = torch.nn.functional.pad(c0.lin.weight, (0, 0, 0, pad))                      # (fp, n_h): zero output rows
            w1 = torch.nn.functional.pad(c1.lin.weight, (0, pad, 0, pad))                    # (fp, fp)
            b0 = torch.nn.functional.pad(c0.bias, (0, pad)).contiguous()
            b1 = torch.nn.functional.pad(c1.bias, (0, pad)).contiguous()
            z = spmm(csr, gemm(h, w0, False, True), bias=b0, prelu_a=zero)                   # ReLU = PReLU with a = 0
            emb = spmm(csr, gemm(z, w1, False, True), bias=b1)
            emb = emb[:, :self.n_in] if pad else emb
        ps = [self.dense_stru.weight, self.dense_stru.bias] + [p for p in self.gat_layer.parameters()]
        self._emb_cache = dict(key=key, emb=emb, keep=(x, fa, ps))           # (keeps the keyed storages alive: no address reuse)
        self.emb_computations += 1
        return emb

    def model_enc(self, x, fa: FullGraphAdj, rs):
        """(loss, score) of the autoencoder; sets self.emb."""
        self.emb = self.gcn_emb(x, fa)
        a1, a2 = self.dense_attr_1, self.dense_attr_2
        if not self.force_wide and fused_supported(self.n_in, self.n_h):
            return FusedAeFn.apply(a1.weight, a1.bias, a2.weight, a2.bias, x, rs)
        return wide_loss(x, a1.weight, a1.bias, a2.weight, a2.bias, rs)

    def forward(self, seq1, adj, idx_train, idx_test, sparse=False):
        dev = self.dense_attr_1.weight.device
        fa = as_full_adj(adj, dev)
        x = seq1.reshape(-1, seq1.shape[-1]).to(dev).contiguous()
        rs = ae_rows(fa, idx_train, idx_test)
        loss, score = self.model_enc(x, fa, rs)
        return loss, score
