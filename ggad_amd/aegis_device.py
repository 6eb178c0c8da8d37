"""Device path of the mini-batch AEGIS comparison model: the discriminator step and the validation sweep in the kernels of
`csrc/aegis_mb.hip`.

What `GCNEncoder.discriminate` does per batch with four `LinearFn` products, `torch.cat`, `nn.BatchNorm1d`, `torch.sigmoid`,
`F.binary_cross_entropy` and the autograd chain of all of these becomes `ggad_aegis_mb_fwd_f32` (one workgroup per batch: both
projections, both batch-norm calls, both heads, both BCE means) and `ggad_aegis_mb_bwd_f32` (the seven gradients of
loss_dis + loss_g); `ggad_aegis_mb_fold_f32` advances the batch norm's running buffers as the two calls per forward do in the default
path (the reference never leaves training mode, so they move under `no_grad` too).  The aggregation stays the plan / gather kernels
of `BatchChunk`; Adam stays `FlatAdam`.

The arithmetic differs from the default path's in summation order only.  There is no fallback: shapes outside
`ggad_aegis_mb_supported` (1 <= feat_dim <= 64, emb_size 64, 2 <= B <= `ggad_aegis_mb_max_rows()`) raise before any launch."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import call

PARAM_NAMES = ("weight", "discriminator2.lins.0.weight", "discriminator2.lins.0.bias", "discriminator2.norms.0.module.weight",
               "discriminator2.norms.0.module.bias", "discriminator2.lins.1.weight", "discriminator2.lins.1.bias")
C = 64
MOMENTUM = 0.1                                                       # nn.BatchNorm1d's default, what the reference's MLP builds


class AegisDevice:
    """Held by `GCNEncoder` when it is given one (`aegis_device=True` builds it): the static gradient buffers, the scratch of the
    backward and the statistics buffers.  All buffers grow on demand and never shrink, so after the first epoch their addresses
    are fixed and the steps can be captured."""

    def __init__(self, enc=None):
        self.lib = _lib.load()
        self.max_rows = int(self.lib.ggad_aegis_mb_max_rows())
        self.enc = None
        self.grads = None
        self._rows_cap, self._stat_cap = 0, 0
        self.scratch = self.inv_std = self.stats = self.p_all = self.p_gen = self.losses = None
        self._bp = {}
        if enc is not None:
            self.bind(enc)

    def bind(self, enc):
        if self.enc is not None and self.enc is not enc:
            raise ValueError("this AegisDevice already belongs to another encoder")
        f, d = int(enc.feat_dim), int(enc.embed_dim)
        if not self.lib.ggad_aegis_mb_supported(f, d, 2):
            raise ValueError(f"the mini-batch AEGIS step kernel takes 1 <= feat_dim <= 64 and emb_size 64; got ({f}, {d})")
        self.enc, self.F = enc, f
        self.grads = None
        return self

    # ---- tensors
    def params(self):
        """The seven tensors the step reads, in kernel order; anything the C ABI cannot read raises before a launch."""
        enc = self.enc
        d2 = enc.discriminator2
        ps = [enc.weight, d2.lins[0].weight, d2.lins[0].bias, d2.norms[0].module.weight, d2.norms[0].module.bias, d2.lins[1].weight,
              d2.lins[1].bias]
        sizes = (C * self.F, C * C, C, C, C, C, 1)
        for name, p, n in zip(PARAM_NAMES, ps, sizes):
            if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous() or p.numel() != n:
                raise ValueError(f"enc.{name}: expected a contiguous float32 tensor of {n} elements on the GPU")
        return ps

    def _bn(self):
        return self.enc.discriminator2.norms[0].module

    def _check_rows(self, x_feat, x_noise):
        for what, t in (("x_feat", x_feat), ("x_noise", x_noise)):
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
                raise ValueError(f"{what}: expected a float32 (B, {self.F}) tensor")
            if t.shape[1] != self.F:
                raise ValueError(f"{what}: expected {self.F} columns, got {t.shape[1]}")
            if not t.is_cuda or t.device != self.enc.weight.device:
                raise ValueError(f"{what}: expected a tensor on {self.enc.weight.device}")
            if not t.is_contiguous():
                raise ValueError(f"{what}: expected a contiguous tensor")
        if x_feat.shape[0] != x_noise.shape[0]:
            raise ValueError("x_feat and x_noise must have the same number of rows")

    def _check_sizes(self, sizes):
        for b in sizes:
            if b == 1:                                               # what nn.BatchNorm1d says in the default path (call 2 sees B rows)
                raise ValueError(f"Expected more than 1 value per channel when training, got input size torch.Size([1, {C}])")
            if b < 1:
                raise ValueError("an empty batch")
            if b > self.max_rows:
                raise ValueError(f"a batch of {b} rows: the mini-batch AEGIS step kernel takes at most {self.max_rows}")

    def _ensure(self, total_rows: int, n_batches: int, dev):
        if total_rows > self._rows_cap or self.scratch is None or self.scratch.device != dev:
            self._rows_cap = max(total_rows, self._rows_cap)
            self.scratch = torch.empty(int(self.lib.ggad_aegis_mb_scratch_elems(self._rows_cap)), dtype=torch.float32, device=dev)
            self.p_all = torch.empty(2 * self._rows_cap, dtype=torch.float32, device=dev)
            self.p_gen = torch.empty(self._rows_cap, dtype=torch.float32, device=dev)
        if n_batches > self._stat_cap or self.stats is None or self.stats.device != dev:
            self._stat_cap = max(n_batches, self._stat_cap)
            self.stats = torch.empty(self._stat_cap, 4 * C, dtype=torch.float32, device=dev)
            self.inv_std = torch.empty(self._stat_cap, 2 * C, dtype=torch.float32, device=dev)
            self.losses = torch.empty(self._stat_cap, 2, dtype=torch.float32, device=dev)
        if self.grads is None or self.grads[0].device != dev:
            self.grads = [torch.zeros_like(p.data) for p in self.params()]

    def reserve(self, max_rows: int, n_batches: int):
        """Sizes every buffer for steps of at most `max_rows` rows in statistics slots 0 .. n_batches - 1 (before a capture)."""
        self._check_sizes([int(max_rows)])
        self._ensure(int(max_rows), int(n_batches), self.enc.weight.device)

    def _one_batch_ptr(self, b: int, dev):
        bp = self._bp.get((b, dev))
        if bp is None:
            bp = self._bp[(b, dev)] = torch.tensor([0, b], dtype=torch.int32, device=dev)
        return bp

    # ---- launches
    def _fwd(self, x_feat, x_noise, bp_dev, n_batches, total_rows, max_b, mode, p_all, p_gen, losses, stats, inv_std):
        ps = self.params()
        call("ggad_aegis_mb_fwd_f32", x_feat.data_ptr(), x_noise.data_ptr(), bp_dev.data_ptr(), n_batches, total_rows, max_b, self.F, C,
             *[p.data_ptr() for p in ps], mode, p_all.data_ptr(), 0 if p_gen is None else p_gen.data_ptr(),
             0 if losses is None else losses.data_ptr(), stats.data_ptr(), 0 if mode != 1 else self.scratch.data_ptr(),
             0 if inv_std is None else inv_std.data_ptr())

    def fold(self, n_batches: int, slot: int = 0):
        """Advances running_mean / running_var / num_batches_tracked by the statistics in slots [slot, slot + n_batches)."""
        bn = self._bn()
        call("ggad_aegis_mb_fold_f32", self.stats[slot].data_ptr(), int(n_batches), MOMENTUM, bn.running_mean.data_ptr(),
             bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr())

    def step(self, x_feat, x_noise, out=None, slot: int = 0, fold: bool = True):
        """Forward and backward of one batch from its two aggregates.  Returns (loss_dis, loss_g) -- views of `out` (2 floats, default
        an own buffer) -- and leaves the gradient of loss_dis + loss_g in the `.grad` of the seven tensors (persistent buffers;
        every other parameter of the model keeps the `.grad` it had).  fold=False leaves the running buffers to a later
        `fold(n, slot0)` over the slots the steps wrote."""
        self._check_rows(x_feat, x_noise)
        b = int(x_feat.shape[0])
        self._check_sizes([b])
        dev = x_feat.device
        self._ensure(b, slot + 1, dev)
        if out is None:
            out = self.losses[slot]
        elif out.dtype != torch.float32 or out.numel() != 2 or not out.is_contiguous() or out.device != dev:
            raise ValueError("out: expected 2 contiguous float32 values on the GPU")
        bp = self._one_batch_ptr(b, dev)
        stats, inv_std = self.stats[slot], self.inv_std[slot]
        self._fwd(x_feat, x_noise, bp, 1, b, b, 1, self.p_all, self.p_gen, out, stats, inv_std)
        ps = self.params()
        call("ggad_aegis_mb_bwd_f32", x_feat.data_ptr(), x_noise.data_ptr(), bp.data_ptr(), b, b, self.F, C, ps[1].data_ptr(),
             ps[3].data_ptr(), ps[4].data_ptr(), ps[5].data_ptr(), self.p_all.data_ptr(), self.p_gen.data_ptr(), stats.data_ptr(),
             self.scratch.data_ptr(), inv_std.data_ptr(), *[g.data_ptr() for g in self.grads])
        for p, g in zip(ps, self.grads):
            p.grad = g
        if fold:
            self.fold(1, slot)
        return out[0], out[1]

    def forward_many(self, x_feat, x_noise, batch_ptr, mode: int = 0, fold: bool = True):
        """One launch over the batches `batch_ptr` (host int array, n + 1 row offsets into the two tables) cuts, then one fold.
        mode 0 returns a dict: p_all (2 T: batch i at 2 batch_ptr[i], real rows then noise rows), p_gen (T), losses (n, 2),
        stats (n, 256);  mode 2 (scores) returns p of the real rows (T), in table order."""
        self._check_rows(x_feat, x_noise)
        bp = np.asarray(batch_ptr, dtype=np.int64).reshape(-1)
        n = len(bp) - 1
        if n < 1 or bp[0] != 0 or bp[-1] != x_feat.shape[0]:
            raise ValueError("batch_ptr: expected n + 1 >= 2 offsets from 0 to the number of rows")
        self._check_sizes(np.diff(bp).tolist())
        if mode not in (0, 2):
            raise ValueError("mode: 0 (every output) or 2 (scores)")
        dev, t = x_feat.device, int(bp[-1])
        self._ensure(2, n, dev)
        bp_dev = torch.from_numpy(bp.astype(np.int32)).to(dev)
        max_b = int(np.diff(bp).max())
        stats = self.stats[:n]
        if mode == 2:
            p = torch.empty(t, dtype=torch.float32, device=dev)
            self._fwd(x_feat, x_noise, bp_dev, n, t, max_b, 2, p, None, None, stats, None)
            out = p
        else:
            out = {"p_all": torch.empty(2 * t, dtype=torch.float32, device=dev), "p_gen": torch.empty(t, dtype=torch.float32, device=dev),
                   "losses": torch.empty(n, 2, dtype=torch.float32, device=dev)}
            self._fwd(x_feat, x_noise, bp_dev, n, t, max_b, 0, out["p_all"], out["p_gen"], out["losses"], stats, None)
            out["stats"] = stats.clone()
        if fold:
            self.fold(n, 0)
        return out

    def discriminate(self, x_feat, x_noise):
        """(logits_all (2B, 1), logits_gen (B, 1), label (2B)) as `GCNEncoder.discriminate` returns them (no autograd graph: training
        goes through `step`)."""
        b = int(x_feat.shape[0]) if isinstance(x_feat, torch.Tensor) and x_feat.dim() == 2 else 0
        out = self.forward_many(x_feat, x_noise, [0, b])
        label = torch.cat([torch.zeros(b, device=x_feat.device), torch.ones(b, device=x_feat.device)])
        return out["p_all"].view(2 * b, 1), out["p_gen"].view(b, 1), label

    def to_prob(self, x_feat, x_noise):
        """The real rows' half of the logits, (B, 1)."""
        logits, _, _ = self.discriminate(x_feat, x_noise)
        return logits[:int(len(logits) / 2)]

    def score_many(self, x_feat, x_noise, batch_ptr):
        """`to_prob` of every batch `batch_ptr` cuts, concatenated (T): one forward launch and one fold."""
        return self.forward_many(x_feat, x_noise, batch_ptr, mode=2)
