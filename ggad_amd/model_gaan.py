"""Full-graph GAAN comparison model -- drop-in for the reference's `model_gaan.py` on the kernels of csrc/gaan.hip and csrc/aegis.hip.

    Model(n_in, n_h, activation, negsamp_round, readout)
        .forward(seq1, adj, idx_train, idx_test, sparse=False) -> (loss, loss_g, score)      model_gaan.py:306

Same constructor order and state_dict keys as the reference: `disc` (the unused Discriminator: its Bilinear still draws), then
`generator = MLP(16, 64, n_in, 2)` and `discriminator = MLP(n_in, 64, 64, 2)`, both `graphsage_aegis.MLP` (the restatement of
torch_geometric 2.1's MLP: Linear -> BatchNorm1d -> ReLU -> Linear, its names and draws).

Forward, always in training mode (the reference's script calls it only between `model.train()` and `model.eval()`; this model
raises in eval mode rather than use running statistics it was never checked on):

- noise = torch.randn(N, 16) from the CPU generator on every call (model_gaan.py:311), or the device buffer `noise_override`
  (a captured epoch: the caller draws and copies);
- x_ = generator(noise); emb = discriminator(x) (kept as `self.emb`); z = discriminator(x_) without autograd (the loss detaches
  a' = sigmoid(z z^T)) -- two batch-norm calls over N rows each, the running statistics updated with x first, then with x_;
- loss = (BCE(a'_E, 0) + BCE(a_E, 1)) / 2 on the edge set E (`edge_structs`) by `ggad_gaan_edge_fwd_f32` / `_bwd_f32`: only the
  m entries of E are evaluated, never the N x N matrices;
- loss_g = mean_{i in idx_train} ||x_i - x_i_hat|| and score_k = ||x_k - x_k_hat|| for k in idx_test by `ggad_aegis_loss_fwd_f32`
  (with no BCE part).  The reference's score is 1 * attr + 0 * stru with stru the BCE of sigmoid(emb emb^T)[idx_test] against
  itself: every BCE term is clamped, so stru is finite, 0 * stru = 0 and the score is attr exactly; the T x N term is skipped.

`adj` is a `FullGraphAdj` (A_hat = normalize_adj(A) + I) or the reference's dense adjacency.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import call, ptr
from .fullgraph import FullGraphAdj, _capturing, _dev_i32, gemm, ticket_block
from .graphsage_aegis import MLP
from .model import AvgReadout, Discriminator, MaxReadout, MinReadout, WSReadout, as_full_adj
from .model_aegis import ACT_RELU, BnActFn, _LossAeFn, bn_forward, loss_rows
from .model_anomalydae import LinearBiasFn


def edge_list(a_hat, idx) -> tuple:
    """(erow, ecol) of the edge set E: for each i of idx in list order, every j with a_hat[i, j] > 0 (as float32, the reference's
    FloatTensor) in ascending order -- what `neighList_to_edgeList_train(adj, idx_train)` returns.  Stored entries that are not
    positive are not in E.  Also returns the per-row counts (len(idx),)."""
    import scipy.sparse as sp
    a = sp.csr_matrix(a_hat).copy()
    a.sum_duplicates()
    a.sort_indices()
    arr = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
    sub = a[arr, :]
    keep = sub.data.astype(np.float32) > 0
    rl = np.repeat(np.arange(arr.size, dtype=np.int64), np.diff(sub.indptr))[keep]
    return arr[rl], sub.indices[keep].astype(np.int64), np.bincount(rl, minlength=arr.size)


def edge_structs(adj: FullGraphAdj, idx) -> dict:
    """Device structures of the edge loss for one row list, cached on `adj` by contents: E in the reference's order (erow, ecol),
    the row offsets rptr, the position pos of every node in the list, the column side (tptr / trow / tedge: the entries (i, k) of
    column k, ascending entry index) and the backward's node partition (small: at most ggad_gaan_bwd_small_count() entries on the
    row and column sides together, one 16-lane group each; big: a workgroup each).  A list holding a node twice raises.  At most 16
    lists are kept, except that a list looked up during a stream capture is pinned: the captured graph holds raw pointers to them."""
    arr = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
    cache = adj.__dict__.setdefault("_gaan", {})
    key = (arr.size, hash(arr.tobytes()))
    s = cache.get(key)
    if s is not None and np.array_equal(s["host"], arr):
        if _capturing(adj.dev):
            s["pinned"] = True
        return s
    if arr.size == 0:
        raise ValueError("the GAAN edge loss needs at least one row")
    if arr.min() < 0 or arr.max() >= adj.n:
        raise ValueError("row index out of range")
    if len(np.unique(arr)) != arr.size:
        raise ValueError("a row list of the GAAN edge loss holds a node twice: the lists must be duplicate-free")
    n = adj.n
    erow, ecol, cnt = edge_list(adj.A.host, arr)
    m = int(erow.size)
    if m >= 2 ** 31 - 1:
        raise ValueError("edge set too large for int32 offsets")
    rptr = np.zeros(arr.size + 1, dtype=np.int64)
    np.cumsum(cnt, out=rptr[1:])
    pos = np.full(n, -1, dtype=np.int32)
    pos[arr] = np.arange(arr.size, dtype=np.int32)
    order = np.argsort(ecol, kind="stable")                           # by column, then entry index
    tptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ecol, minlength=n), out=tptr[1:])
    rdeg = np.zeros(n, dtype=np.int64)
    rdeg[arr] = cnt
    count = rdeg + np.diff(tptr)
    lim = int(_lib.load().ggad_gaan_bwd_small_count())
    dev = adj.dev
    s = dict(host=arr, n_rows=int(arr.size), m=m, rows=torch.from_numpy(arr).to(dev), erow=_dev_i32(erow, dev), ecol=_dev_i32(ecol, dev),
             rptr=_dev_i32(rptr, dev), pos=_dev_i32(pos, dev), tptr=_dev_i32(tptr, dev), trow=_dev_i32(erow[order], dev),
             tedge=_dev_i32(order, dev), small=_dev_i32(np.nonzero(count <= lim)[0], dev), big=_dev_i32(np.nonzero(count > lim)[0], dev),
             pinned=_capturing(dev))
    s["n_small"], s["n_big"] = int(s["small"].numel()), int(s["big"].numel())
    evictable = [k for k in cache if not cache[k]["pinned"]]
    if len(evictable) >= 16:
        for k in evictable:
            del cache[k]
    cache[key] = s
    return s


def _check_channels(rc, C, name):
    if rc == _lib.GGAD_E_UNSUPPORTED:
        raise ValueError("the GAAN edge kernels take {} channels, not {}".format(int(_lib.load().ggad_gaan_edge_channels()), C))
    _lib.check(rc, name)


def edge_loss_fwd(emb, z, es):
    """(vals, a): vals = [loss, BCE(a', 0), BCE(a, 1)] (device, 3 floats), a = sigmoid(<emb_i, emb_j>) per entry of E."""
    n, C = emb.shape
    dev = emb.device
    vals = torch.empty(3, dtype=torch.float32, device=dev)
    a = torch.empty(max(es["m"], 1), dtype=torch.float32, device=dev)
    ws = torch.empty(int(_lib.load().ggad_gaan_edge_fwd_workspace_elems(es["m"])), dtype=torch.float32, device=dev)
    rc = int(_lib.load().ggad_gaan_edge_fwd_f32(ptr(emb), ptr(z), n, C, ptr(es["erow"]), ptr(es["ecol"]), es["m"], ptr(a), ptr(ws), ptr(vals),
                                                 _lib.current_stream()))
    _check_channels(rc, C, "ggad_gaan_edge_fwd_f32")
    return vals, a


def edge_loss_bwd(emb, a, es, g):
    n, C = emb.shape
    dE = torch.empty_like(emb)
    rc = int(_lib.load().ggad_gaan_edge_bwd_f32(ptr(emb), n, C, ptr(es["pos"]), ptr(es["rptr"]), ptr(es["ecol"]), ptr(es["tptr"]),
                                                 ptr(es["trow"]), ptr(es["tedge"]), ptr(a), es["m"], ptr(g), ptr(es["small"]), es["n_small"],
                                                 ptr(es["big"]), es["n_big"], ptr(dE), _lib.current_stream()))
    _check_channels(rc, C, "ggad_gaan_edge_bwd_f32")
    return dE


class EdgeLossFn(torch.autograd.Function):
    """loss = (BCE(sigmoid(<z_i, z_j>), 0) + BCE(sigmoid(<emb_i, emb_j>), 1)) / 2 over E (means over its m entries); z gets no
    gradient (the reference detaches a').  Returns (loss, parts = [BCE(a', 0), BCE(a, 1)])."""

    @staticmethod
    def forward(ctx, emb, z, es):
        emb, z = emb.contiguous(), z.detach().contiguous()
        vals, a = edge_loss_fwd(emb, z, es)
        ctx.save_for_backward(emb, a)
        ctx.es = es
        parts = vals[1:]
        ctx.mark_non_differentiable(parts)
        return vals[0], parts

    @staticmethod
    def backward(ctx, g, _gp):
        emb, a = ctx.saved_tensors
        return edge_loss_bwd(emb, a, ctx.es, g.reshape(1).contiguous()), None, None


def edge_loss(emb, z, adj: FullGraphAdj, idx):
    """(loss, parts) of the reference's loss_func_ed on the edge set of the rows `idx`."""
    return EdgeLossFn.apply(emb, z, edge_structs(adj, idx))


def _attr(x_, x, rs, value):
    """attr[k] = ||x_r - x_r_hat||, r = rows[k] of `rs`, and value[0] = their mean (ggad_aegis_loss_fwd_f32 with no BCE part)."""
    n, F_ = x.shape
    dev = x.device
    attr = torch.empty(rs["n_rows"], dtype=torch.float32, device=dev)
    ws = torch.empty(int(_lib.load().ggad_aegis_loss_workspace_elems(0, rs["n_rows"])), dtype=torch.float32, device=dev)
    call("ggad_aegis_loss_fwd_f32", 0, 0, ptr(x), F_, ptr(x_), x_.stride(0), ptr(rs["rows"]), rs["n_rows"], ptr(attr), 0, ptr(value),
         ptr(ws), ptr(ticket_block(dev)))
    return attr


def attr_loss(x_, x, adj: FullGraphAdj, idx_train, idx_test):
    """(loss_g, score): mean_{i in idx_train} ||x_i - x_i_hat|| with its backward to x_hat, and ||x_k - x_k_hat|| for k in idx_test."""
    x_ = x_.contiguous()
    dev = x.device
    rs = loss_rows(adj, idx_train)
    value = torch.empty(1, dtype=torch.float32, device=dev)
    attr = _attr(x_.detach(), x, rs, value)
    loss_g = _LossAeFn.apply(x_, value[0], None, x, rs, attr)
    with torch.no_grad():
        score = _attr(x_.detach(), x, loss_rows(adj, idx_test), torch.empty(1, dtype=torch.float32, device=dev))
    return loss_g, score


class Model(nn.Module):
    def __init__(self, n_in, n_h, activation, negsamp_round, readout):
        super().__init__()
        self.noise_dim = 16
        self.hid_dim = 64
        self.read_mode = readout
        self.act = nn.ReLU()
        if readout == "max":
            self.read = MaxReadout()
        elif readout == "min":
            self.read = MinReadout()
        elif readout == "avg":
            self.read = AvgReadout()
        elif readout == "weighted_sum":
            self.read = WSReadout()
        self.disc = Discriminator(n_h, negsamp_round)                                       # model_gaan.py:142 (unused, draws)
        noise_dim, hid_dim, num_layers = 16, 64, 4
        generator_layers, encoder_layers = num_layers // 2, (num_layers + 1) // 2
        self.generator = MLP(noise_dim, hid_dim, n_in, generator_layers, 0.0, F.relu)
        self.discriminator = MLP(n_in, hid_dim, hid_dim, encoder_layers, 0.0, F.relu)
        self.noise_override = None
        self.device_noise = None
        self.emb = None

    def _noise(self, n, dev):
        if self.noise_override is not None:
            return self.noise_override.reshape(n, self.noise_dim)
        if self.device_noise is not None:                                                   # the same draw on the device (ggad_amd.rng)
            buf = self.__dict__.get("_dn_buf")
            if buf is None or buf.shape != (n, self.noise_dim) or buf.device != dev:
                buf = self.__dict__["_dn_buf"] = torch.empty(n, self.noise_dim, device=dev)
            return self.device_noise.randn_(buf)
        return torch.randn(n, self.noise_dim).to(dev)                                       # model_gaan.py:311: the CPU generator

    def train_forward(self, seq1, adj, idx_train, idx_test):
        """(loss, loss_g, score, parts, x_, z): the forward with the loss parts [BCE(a', 0), BCE(a, 1)], x_ and z_ beside it."""
        if not self.training:
            raise ValueError("the full-graph GAAN forward runs batch norm in training mode only (as the reference's script calls it)")
        dev = self.generator.lins[0].weight.device
        fa = as_full_adj(adj, dev)
        x = seq1.reshape(-1, seq1.shape[-1]).to(dev).contiguous()
        n = x.shape[0]
        gen, dis = self.generator, self.discriminator
        gbn, dbn = gen.norms[0].module, dis.norms[0].module
        h = LinearBiasFn.apply(self._noise(n, dev), gen.lins[0].weight, gen.lins[0].bias, False)
        x_ = LinearBiasFn.apply(BnActFn.apply(h, gbn.weight, gbn.bias, gbn, ACT_RELU), gen.lins[1].weight, gen.lins[1].bias, False)
        h = LinearBiasFn.apply(x, dis.lins[0].weight, dis.lins[0].bias, False)
        emb = LinearBiasFn.apply(BnActFn.apply(h, dbn.weight, dbn.bias, dbn, ACT_RELU), dis.lins[1].weight, dis.lins[1].bias, False)
        self.emb = emb
        with torch.no_grad():                                   # z_ = discriminator(x_): a' is detached; the BN buffers still move
            hz = gemm(x_.detach(), dis.lins[0].weight.detach(), False, True, bias=dis.lins[0].bias.detach())
            yz, _, _ = bn_forward(hz, None, dbn, ACT_RELU)
            z = gemm(yz, dis.lins[1].weight.detach(), False, True, bias=dis.lins[1].bias.detach())
        loss, parts = edge_loss(emb, z, fa, idx_train)
        loss_g, score = attr_loss(x_, x, fa, idx_train, idx_test)
        return loss, loss_g, score, parts, x_, z

    def forward(self, seq1, adj, idx_train, idx_test, sparse=False):
        loss, loss_g, score, _, _, _ = self.train_forward(seq1, adj, idx_train, idx_test)
        return loss, loss_g, score
