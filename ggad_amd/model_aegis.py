"""Full-graph AEGIS comparison model -- drop-in for the reference's `model_AEGIS.py` on the kernels of csrc/aegis.hip.

    Model(n_in, n_h, activation, negsamp_round, readout)
        .forward(seq1, adj, idx_train, idx_test, sparse=False) -> (loss_ae, loss_g, loss_ae, score, emb_all)   model_AEGIS.py:230

Same constructor order and state_dict keys as the reference (disc, the four GCN layers, generator, discriminator,
discriminator2; the two unused modules still consume the RNG).  The MLPs are `graphsage_aegis.MLP`, the restatement of
`torch_geometric.nn.MLP` (2.1): its parameter and buffer names (`generator.lins.0.weight`, `generator.norms.0.module.running_mean`,
...), its draws.  **Parity is against that restatement**, not against torch_geometric itself, which is absent here.

Forward, always in training mode (the reference's script only calls it between `model.train()` and `model.eval()`; this model
raises in eval mode rather than use running statistics it was never checked on):

- noise = torch.randn(N, 16) from the CPU generator on every call (model_AEGIS.py:226), or the device buffer `noise_override`
  (a captured epoch: the caller draws and copies);
- x_gen = generator(noise): Linear on the GEMM with its bias epilogue, batch norm over the N rows fused with ReLU
  (`ggad_aegis_bn_fwd_f32`), Linear;
- z = enc2(enc1(x)), z_gen = enc2(enc1(x_gen)), z_dec = dec2(dec1(z)) on `GcnLayerFn` (A_hat X of the constant x is cached);
  the dead z_gen_dec is skipped.  dec2 has n_in outputs and the SpMM / PReLU kernels take widths that are multiples of 4: its
  weight and bias get zero rows up to the next one and the loss reads the first n_in columns.  Exact: PReLU(0) = 0;
- logits = sigmoid(discriminator2(cat(z, z_gen))): ONE batch-norm call over the two row blocks (statistics over 2N rows, the
  concatenation is never built, the z_gen projection is shared with the next call), its head evaluated on the idx_test rows
  only -- that is all the forward returns of it (`score`; loss_dis is discarded by the reference);
- logits_gen = sigmoid(discriminator2(z_gen)): the second batch-norm call, statistics over the N generated rows, head on all;
- loss_g = BCE(logits_gen, 0) and loss_ae = mean_{i in idx_train} ||x_i - z_dec_i|| in one launch (`aegis_losses`).
Both batch-norm modules update their running statistics as torch's does (discriminator2's twice per forward).

`adj` is a `FullGraphAdj` or the reference's dense adjacency; `affinity` gives the reference's local affinity over raw_adj
without the 2N x 2N similarity matrix.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import call, ptr
from .fullgraph import FullGraphAdj, GcnLayerFn, _capturing, gemm, spmm, ticket_block
from .graphsage_aegis import MLP
from .model import GCN, AvgReadout, MaxReadout, MinReadout, WSReadout, as_full_adj
from .model import Discriminator
from .model_anomalydae import LinearBiasFn

ACT_RELU, ACT_SIGMOID = 0, 1


def _bn_parts(bn: nn.BatchNorm1d):
    nbt = bn.num_batches_tracked
    return bn.weight, bn.bias, bn.running_mean, bn.running_var, nbt, float(bn.eps), float(bn.momentum)


def _bn_ws(M: int, C: int, dev) -> torch.Tensor:
    return torch.empty(int(_lib.load().ggad_aegis_bn_workspace_elems(M, C)), dtype=torch.float32, device=dev)


def bn_forward(h1, h2, bn: nn.BatchNorm1d, act: int, rows=None, head=None, update: bool = True):
    """act(BatchNorm1d(cat(h1, h2))) in training mode (h2 may be None), on the rows `rows` (int64 device tensor of row indices of
    the concatenation; None: all).  head = (w2 (C,), b2 (1,)): returns p = sigmoid(y . w2 + b2) per row instead of y.  Updates
    `bn`'s running statistics when `update`.  Returns (out, mean, invstd)."""
    gamma, beta, rm, rv, nbt, eps, mom = _bn_parts(bn)
    dev = h1.device
    C = h1.shape[1]
    m1, m2 = h1.shape[0], (0 if h2 is None else h2.shape[0])
    M = m1 + m2
    n_out = M if rows is None else rows.numel()
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    invstd = torch.empty(C, dtype=torch.float32, device=dev)
    if head is None:
        out = torch.empty(n_out, C, dtype=torch.float32, device=dev)
        y_ptr, ldy, w2p, b2p, pp = ptr(out), C, 0, 0, 0
    else:
        out = torch.empty(n_out, dtype=torch.float32, device=dev)
        y_ptr, ldy, w2p, b2p, pp = 0, 0, ptr(head[0]), ptr(head[1]), ptr(out)
    ws = _bn_ws(M, C, dev)
    rc = int(_lib.load().ggad_aegis_bn_fwd_f32(
        ptr(h1), m1, h1.stride(0), ptr(h2) if h2 is not None else 0, m2, h2.stride(0) if h2 is not None else 0, C, ptr(gamma), ptr(beta),
        eps, mom, ptr(rm) if update else 0, ptr(rv) if update else 0, ptr(nbt) if update else 0, act, ptr(rows), n_out, y_ptr, ldy,
        w2p, b2p, pp, ptr(mean), ptr(invstd), ptr(ws), ptr(ticket_block(dev)), _lib.current_stream()))
    if rc == _lib.GGAD_E_UNSUPPORTED:
        raise ValueError("the AEGIS batch-norm kernels take {} channels, not {}".format(int(_lib.load().ggad_aegis_bn_channels()), C))
    if rc == _lib.GGAD_E_INVALID and M < 2:
        raise ValueError("Expected more than 1 value per channel when training, got {} rows".format(M))
    _lib.check(rc, "ggad_aegis_bn_fwd_f32")
    return out, mean, invstd


def _bn_backward(h, gamma, beta, mean, invstd, act, dy=None, head=None):
    """(dh, dgamma, dbeta[, dw2, db2]) of one batch-norm call; head = (w2, p, dp)."""
    M, C = h.shape
    dev = h.device
    dh = torch.empty_like(h)
    dgamma = torch.empty(C, dtype=torch.float32, device=dev)
    dbeta = torch.empty(C, dtype=torch.float32, device=dev)
    dw2 = db2 = None
    if head is not None:
        w2, p, dp = head
        dw2 = torch.empty(C, dtype=torch.float32, device=dev)
        db2 = torch.empty(1, dtype=torch.float32, device=dev)
        args = (0, 0, ptr(w2), ptr(p), ptr(dp))
    else:
        args = (ptr(dy), dy.stride(0), 0, 0, 0)
    ws = _bn_ws(M, C, dev)
    call("ggad_aegis_bn_bwd_f32", ptr(h), M, h.stride(0), C, ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), act, *args, ptr(dh),
         dh.stride(0), ptr(dgamma), ptr(dbeta), ptr(dw2), ptr(db2), ptr(ws), ptr(ticket_block(dev)))
    return dh, dgamma, dbeta, dw2, db2


class BnActFn(torch.autograd.Function):
    """y = act(BatchNorm1d(h)) in training mode over the rows of h (the generator's hidden layer: act = ReLU)."""

    @staticmethod
    def forward(ctx, h, gamma, beta, bn, act: int):
        h = h.contiguous()
        y, mean, invstd = bn_forward(h, None, bn, act)
        ctx.save_for_backward(h, gamma, beta, mean, invstd)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, g):
        h, gamma, beta, mean, invstd = ctx.saved_tensors
        dh, dgamma, dbeta, _, _ = _bn_backward(h, gamma, beta, mean, invstd, ctx.act, dy=g.contiguous())
        return dh, dgamma, dbeta, None, None


class BnHeadFn(torch.autograd.Function):
    """p = sigmoid(act(BatchNorm1d(h)) . w2 + b2) per row, training mode over the rows of h (discriminator2 on z_gen: act = sigmoid)."""

    @staticmethod
    def forward(ctx, h, gamma, beta, w2, b2, bn, act: int):
        h = h.contiguous()
        w2 = w2.reshape(-1).contiguous()
        p, mean, invstd = bn_forward(h, None, bn, act, head=(w2, b2.reshape(-1).contiguous()))
        ctx.save_for_backward(h, gamma, beta, w2, p, mean, invstd)
        ctx.act = act
        return p

    @staticmethod
    def backward(ctx, g):
        h, gamma, beta, w2, p, mean, invstd = ctx.saved_tensors
        dh, dgamma, dbeta, dw2, db2 = _bn_backward(h, gamma, beta, mean, invstd, ctx.act, head=(w2, p, g.contiguous()))
        return dh, dgamma, dbeta, dw2.view(1, -1), db2, None, None


def loss_rows(adj: FullGraphAdj, idx) -> dict:
    """Device rows (int64) and inverse map (int32, -1 off the list) of one row list (a loss list or the scored rows), cached on
    `adj` by contents; a list that holds a node twice is refused (the reference's lists are duplicate-free).  At most 16 lists are
    kept, except that a list looked up during a stream capture is pinned: the captured graph holds raw pointers to its structures."""
    arr = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
    cache = adj.__dict__.setdefault("_aegis_rows", {})
    key = (arr.size, hash(arr.tobytes()))
    s = cache.get(key)
    if s is not None and np.array_equal(s["host"], arr):
        if _capturing(adj.dev):
            s["pinned"] = True
        return s
    if arr.size == 0:
        raise ValueError("the row list is empty")
    if arr.min() < 0 or arr.max() >= adj.n:
        raise ValueError("row index out of range")
    if len(np.unique(arr)) != arr.size:
        raise ValueError("an AEGIS row list holds a node twice: the lists must be duplicate-free")
    pos = np.full(adj.n, -1, dtype=np.int32)
    pos[arr] = np.arange(arr.size, dtype=np.int32)
    s = dict(host=arr, n_rows=int(arr.size), rows=torch.from_numpy(arr).to(adj.dev), pos=torch.from_numpy(pos).to(adj.dev),
             pinned=_capturing(adj.dev))
    evictable = [k for k in cache if not cache[k]["pinned"]]
    if len(evictable) >= 16:
        for k in evictable:
            del cache[k]
    cache[key] = s
    return s


def _loss_bwd(p, zd, x, rs, attr, g_g=None, g_ae=None):
    n, F_ = x.shape
    dp = torch.empty_like(p) if g_g is not None else None
    dzd = torch.empty_like(zd) if g_ae is not None else None
    call("ggad_aegis_loss_bwd_f32", ptr(p), n, ptr(g_g), ptr(dp), ptr(x), F_, ptr(zd), zd.stride(0), ptr(rs["pos"]) if dzd is not None else 0,
         rs["n_rows"], ptr(attr) if dzd is not None else 0, ptr(g_ae), ptr(dzd))
    return dp if dzd is None else dzd


class _LossGFn(torch.autograd.Function):
    """loss_g = BCE(p, 0), its value computed by `aegis_losses`; backward: dp."""

    @staticmethod
    def forward(ctx, p, value, zd, x, rs, attr):
        ctx.save_for_backward(p, zd, x, attr)
        ctx.rs = rs
        return value

    @staticmethod
    def backward(ctx, g):
        p, zd, x, attr = ctx.saved_tensors
        return _loss_bwd(p, zd, x, ctx.rs, attr, g_g=g.reshape(1).contiguous()), None, None, None, None, None


class _LossAeFn(torch.autograd.Function):
    """loss_ae = mean_{i in rows} ||x_i - zd_i[:F]||, its value computed by `aegis_losses`; backward: d zd (every element written)."""

    @staticmethod
    def forward(ctx, zd, value, p, x, rs, attr):
        ctx.save_for_backward(p, zd, x, attr)
        ctx.rs = rs
        return value

    @staticmethod
    def backward(ctx, g):
        p, zd, x, attr = ctx.saved_tensors
        return _loss_bwd(p, zd, x, ctx.rs, attr, g_ae=g.reshape(1).contiguous()), None, None, None, None, None


def aegis_losses(p, zd, x, rs):
    """(loss_g, loss_ae) = (BCE(p, 0), mean_{i in rs rows} ||x_i - zd_i[:F]||): both values in one launch; each loss is its own autograd
    node, so backpropagating one of them (pre-training: loss_ae alone) leaves the other's subgraph -- the generator and discriminator2
    -- without gradients, as in the reference.  zd may carry zero padding columns (its gradient there is 0)."""
    n, F_ = x.shape
    dev = x.device
    vals = torch.empty(2, dtype=torch.float32, device=dev)
    attr = torch.empty(rs["n_rows"], dtype=torch.float32, device=dev)
    ws = torch.empty(int(_lib.load().ggad_aegis_loss_workspace_elems(n, rs["n_rows"])), dtype=torch.float32, device=dev)
    p, zd = p.contiguous(), zd.contiguous()
    call("ggad_aegis_loss_fwd_f32", ptr(p), n, ptr(x), F_, ptr(zd), zd.stride(0), ptr(rs["rows"]), rs["n_rows"], ptr(attr),
         vals.data_ptr(), vals.data_ptr() + 4, ptr(ws), ptr(ticket_block(dev)))
    pd, zdd = p.detach(), zd.detach()
    loss_g = _LossGFn.apply(p, vals[0], zdd, x, rs, attr)
    loss_ae = _LossAeFn.apply(zd, vals[1], pd, x, rs, attr)
    return loss_g, loss_ae


def _gcn(layer: GCN, x, fa: FullGraphAdj, pad_to: int = 0):
    """PReLU(A_hat (x W^T) + b) through GcnLayerFn; pad_to > out_ft: zero output rows of W and b up to that width (the extra
    output columns are exactly 0)."""
    w, b = layer.fc.weight, layer.bias
    if pad_to > w.shape[0]:
        w = F.pad(w, (0, 0, 0, pad_to - w.shape[0]))
        b = F.pad(b, (0, pad_to - b.shape[0]))
    return GcnLayerFn.apply(x, w, b, layer.act.weight, fa)


class Model(nn.Module):
    def __init__(self, n_in, n_h, activation, negsamp_round, readout):
        super().__init__()
        if activation != "prelu":
            raise ValueError("the full-graph AEGIS runs its GCN layers with PReLU, as the reference's script constructs them")
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
        self.disc = Discriminator(n_h, negsamp_round)                                       # model_AEGIS.py:138 (unused, draws)
        noise_dim, hid_dim, num_layers = 16, 64, 4
        generator_layers, encoder_layers = num_layers // 2, (num_layers + 1) // 2
        self.gcn_enc1 = GCN(n_in, n_h, activation)
        self.gcn_enc2 = GCN(n_h, n_h, activation)
        self.gcn_dec1 = GCN(n_h, n_h, activation)
        self.gcn_dec2 = GCN(n_h, n_in, activation)
        self.generator = MLP(noise_dim, hid_dim, n_in, generator_layers, 0.0, F.relu)
        self.discriminator = MLP(n_in, hid_dim, hid_dim, encoder_layers, 0.0, F.relu)      # (unused, draws)
        self.discriminator2 = MLP(n_h, hid_dim, 1, encoder_layers, 0.0, torch.sigmoid)
        self.n_in = n_in
        self.noise_override = None
        self.device_noise = None

    # ------------------------------------------------------------------------------------------------ pieces
    def _noise(self, n, dev):
        if self.noise_override is not None:
            return self.noise_override.reshape(n, self.noise_dim)
        if self.device_noise is not None:                                                   # the same draw on the device (ggad_amd.rng)
            buf = self.__dict__.get("_dn_buf")
            if buf is None or buf.shape != (n, self.noise_dim) or buf.device != dev:
                buf = self.__dict__["_dn_buf"] = torch.empty(n, self.noise_dim, device=dev)
            return self.device_noise.randn_(buf)
        return torch.randn(n, self.noise_dim).to(dev)                                       # model_AEGIS.py:226: the CPU generator

    def _check_mode(self):
        if not self.training:
            raise ValueError("the full-graph AEGIS forward runs batch norm in training mode only (as the reference's script calls it)")

    def train_forward(self, seq1, adj, idx_train, idx_test):
        """(loss_ae, loss_g, score, z, z_gen, z_dec): the forward without the concatenated emb_all (what the script runs)."""
        self._check_mode()
        dev = self.gcn_enc1.fc.weight.device
        fa = as_full_adj(adj, dev)
        x = seq1.reshape(-1, seq1.shape[-1]).to(dev).contiguous()
        n = x.shape[0]
        gen = self.generator
        h = LinearBiasFn.apply(self._noise(n, dev), gen.lins[0].weight, gen.lins[0].bias, False)
        y = BnActFn.apply(h, gen.norms[0].module.weight, gen.norms[0].module.bias, gen.norms[0].module, ACT_RELU)
        x_gen = LinearBiasFn.apply(y, gen.lins[1].weight, gen.lins[1].bias, False)
        z_gen = _gcn(self.gcn_enc2, _gcn(self.gcn_enc1, x_gen, fa), fa)
        z = _gcn(self.gcn_enc2, _gcn(self.gcn_enc1, x, fa), fa)
        fp = (self.n_in + 3) // 4 * 4
        zd_pad = _gcn(self.gcn_dec2, _gcn(self.gcn_dec1, z, fa), fa, pad_to=fp)
        d2 = self.discriminator2
        bn = d2.norms[0].module
        w2, b2 = d2.lins[1].weight, d2.lins[1].bias
        h_gen = LinearBiasFn.apply(z_gen, d2.lins[0].weight, d2.lins[0].bias, False)
        with torch.no_grad():                                                                # logits over cat(z, z_gen): scores only
            h_real = gemm(z.detach(), d2.lins[0].weight.detach(), False, True, bias=d2.lins[0].bias.detach())
            rows = loss_rows(fa, idx_test)["rows"]                                          # (cached: no copy inside a capture)
            score, _, _ = bn_forward(h_real, h_gen.detach(), bn, ACT_SIGMOID, rows=rows,
                                     head=(w2.detach().reshape(-1).contiguous(), b2.detach().reshape(-1).contiguous()))
        p_gen = BnHeadFn.apply(h_gen, bn.weight, bn.bias, w2, b2, bn, ACT_SIGMOID)
        loss_g, loss_ae = aegis_losses(p_gen, zd_pad, x, loss_rows(fa, idx_train))
        return loss_ae, loss_g, score.view(-1, 1), z, z_gen, zd_pad[:, :self.n_in]

    def forward(self, seq1, adj, idx_train, idx_test, sparse=False):
        loss_ae, loss_g, score, z, z_gen, _ = self.train_forward(seq1, adj, idx_train, idx_test)
        emb_all = torch.cat([z, z_gen], 0)
        return loss_ae, loss_g, loss_ae, score, emb_all

    # ------------------------------------------------------------------------------------------------ affinity (aegis.py:126-146)
    @staticmethod
    def affinity(emb: torch.Tensor, adj: FullGraphAdj) -> torch.Tensor:
        """affinity_j = (1 / colsum_j(raw)) sum_i raw_ij <e_hat_i, e_hat_j> for the N rows of emb (e_hat = emb / |emb|, 1/0 -> 0):
        r_inv_j <e_hat_j, (raw^T e_hat)_j> with the row-normalisation kernel, the SpMM over adj.Rt and the scaled row dots.  The
        reference's 2N x 2N similarity matrix contributes only its two diagonal N x N blocks: call this once for z, once for z_gen."""
        with torch.no_grad():
            e = emb.detach().contiguous()
            n, h = e.shape
            dev = e.device
            inv = torch.empty(n, dtype=torch.float32, device=dev)
            en = torch.empty_like(e)
            call("ggad_rownorm_f32", ptr(e), n, h, ptr(inv), ptr(en))
            s = spmm(adj.Rt, en)
            aff = torch.empty(n, dtype=torch.float32, device=dev)
            call("ggad_rowdot_f32", ptr(en), None, ptr(s), n, h, ptr(adj.r_inv_dev()), ptr(aff))
        return aff
