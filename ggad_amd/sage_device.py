"""Device path of the GraphSAGE comparison model: neighbour sampling by the native `random.sample` (`csrc/sampler.cpp`) and the whole
step -- gather, sampled mean, encoder, classifier, cross entropy and the two weight gradients -- in the kernels of `csrc/sage.hip`.

What `MeanAggregator.forward` / `Encoder.forward` do per batch with a python set per row, `random.sample` and `sorted` per row, two
index uploads, a segment mean, a feature gather, `torch.cat`, two `LinearFn` products, torch's cross entropy and the autograd chain
of all of these becomes: one native sampler call (a B x k table of ids and the row lengths), one upload, `ggad_sage_fwd_f32` and
`ggad_sage_bwd_f32`.  Adam stays `FlatAdam`.

Parity with the set path: the draws are bit-exact -- same samples, same position of the `random` stream afterwards -- for graphs
given as CSR and for dicts whose sets were filled in ascending id order (`synth.csr_to_adj_lists`, what `Encoder.forward` builds from
a `DeviceGraph`): `random.sample` walks a set in its iteration order, which depends on the order of insertion, and only the
ascending one is restated natively.  A dict of sets filled in another order still trains, on other (equally distributed) samples.
The arithmetic differs from the set path's in summation order only.

A row without neighbours gives what `ggad_seg_mean` gives for an empty list: 0 * (1 / 0) = NaN in the neighbour half of
`combined`, hence NaN scores for that row, as in the reference (its dense mask row is 0 / 0).

The epoch path (`sage_epoch.py`, config key `sage_epoch`) builds on this object: it samples and trains whole epochs without returning
to the host between steps, and uses `presample` to draw a validation sweep's table while the device still trains.

There is no fallback: shapes outside `ggad_sage_supported` (1 <= feat_dim <= 64, 1 <= embed_dim <= 64, two classes), `gcn=True` and
`num_sample=None` raise at construction."""
from __future__ import annotations

import random

import numpy as np
import torch

from . import _lib
from ._lib import call
from .graph import DeviceGraph
from .sampler import PyCompatRandom


def _dptr(t, dtype, what: str, numel: int) -> int:
    """Device pointer of a tensor handed to a `ggad_sage_*` entry point; anything the C ABI cannot read raises before a launch."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or not t.is_cuda or t.numel() != numel:
        raise ValueError(f"{what}: expected a contiguous {dtype} tensor of {numel} elements on the GPU")
    return t.data_ptr()


class SageBatch:
    """One sampled batch on the device: `nodes` (B), `cnt` (B), `nbr` (B x k) and optionally `labels` (B), all int32, cut from one
    uploaded block.  Built by `SageDevice.upload`, which range-checks everything on the host."""

    def __init__(self, block: torch.Tensor, b: int, k: int, with_labels: bool):
        self.b, self.k = int(b), int(k)
        self.nodes, self.cnt = block[:b], block[b:2 * b]
        self.labels = block[2 * b:3 * b] if with_labels else None
        self.nbr = block[3 * b:3 * b + b * k].view(b, k)


class SageDevice:
    """Held by `Encoder` when it is given one: the CSR graph, the feature table and the generator the samples are drawn from.

    ``rng=None``: every call continues python's global stream (`random.getstate()` in, `random.setstate()` out) -- slow (624 words
    each way per call) but drop-in.  ``rng`` a `PyCompatRandom`: the samples are drawn from it."""

    def __init__(self, graph: DeviceGraph, features, feat_dim: int, embed_dim: int, num_sample, rng=None, gcn: bool = False,
                 num_classes: int = 2):
        lib = _lib.load()
        if gcn:
            raise ValueError("the GraphSAGE device path has no gcn=True encoder")
        if num_sample is None:
            raise ValueError("the GraphSAGE device path needs num_sample (an integer): it samples every row of degree >= num_sample")
        if int(num_sample) != num_sample or int(num_sample) < 1:
            raise ValueError("num_sample must be a positive integer")
        if not lib.ggad_sage_supported(int(feat_dim), int(embed_dim), int(num_classes)):
            raise ValueError(f"the GraphSAGE step kernel takes 1 <= feat_dim <= 64, 1 <= embed_dim <= {int(lib.ggad_max_embed_dim())} "
                             f"and 2 classes; got ({feat_dim}, {embed_dim}, {num_classes})")
        if not isinstance(graph, DeviceGraph):
            raise ValueError("the GraphSAGE device path takes a DeviceGraph")
        table = features.weight if hasattr(features, "weight") else features
        if table.dim() != 2 or table.shape[1] != feat_dim or table.dtype != torch.float32 or not table.is_contiguous():
            raise ValueError("feature table: expected a contiguous float32 (N, feat_dim) tensor")
        if not table.is_cuda:
            raise ValueError("the GraphSAGE device path needs its feature table on the GPU")
        if graph.n > table.shape[0]:
            raise ValueError("the graph has more nodes than the feature table has rows")
        col = graph.col_host
        if len(col) and (int(col.min()) < 0 or int(col.max()) >= graph.n):
            raise ValueError(f"the graph holds a column outside [0, {graph.n})")
        if rng is not None and not isinstance(rng, PyCompatRandom):
            raise ValueError("rng must be a PyCompatRandom or None")
        self.graph, self.table = graph, table.detach()
        self.F, self.D, self.k = int(feat_dim), int(embed_dim), int(num_sample)
        self.rng = rng
        self.ws = torch.empty(int(lib.ggad_sage_bwd_workspace_elems(self.F, self.D)), dtype=torch.float32, device=table.device)
        self.last = {}                                             # buffers of the latest forward / backward (tests, profiling)
        self._ahead = None                                         # a table drawn by `presample` for the next `sample` call

    # ---- host side
    def sample(self, nodes):
        """(nodes, nbr, cnt) as numpy: the sample table of `nodes`, in list order, on the configured stream."""
        nodes = np.asarray(nodes.detach().cpu().numpy() if isinstance(nodes, torch.Tensor) else nodes, dtype=np.int64).reshape(-1)
        g = self.graph
        ahead, self._ahead = self._ahead, None
        if ahead is not None:
            if not np.array_equal(ahead[0], nodes):
                raise RuntimeError("a table sampled ahead was drawn for other nodes than the next call asks for: the `random` "
                                   "stream would be out of order")
            return ahead
        if len(nodes) == 0 or nodes.min() < 0 or nodes.max() >= g.n:
            raise ValueError(f"batch nodes must be a non-empty list of ids in [0, {g.n})")
        if self.rng is not None:
            nbr, cnt = self.rng.sample_rows(g.rowptr_host, g.col_host, nodes, self.k)
        else:
            rng = PyCompatRandom.from_python_state(random.getstate())
            nbr, cnt = rng.sample_rows(g.rowptr_host, g.col_host, nodes, self.k)
            random.setstate(rng.to_python_state())
        return nodes, nbr, cnt

    def presample(self, nodes) -> None:
        """Draws the table of `nodes` NOW and keeps it for the next `sample` call, which must ask for the same ids: the epoch path
        (sage_epoch.py) samples a validation sweep while the device still trains.  The draws are the ones that call would make."""
        self._ahead = None
        self._ahead = self.sample(nodes)

    def upload(self, nodes, nbr, cnt, labels=None) -> SageBatch:
        """Checks a sample table on the host -- every id a row of the feature table, every length in [0, k], labels in {0, 1} --
        and uploads it as one block."""
        nodes = np.asarray(nodes, dtype=np.int64).reshape(-1)
        nbr = np.asarray(nbr)
        cnt = np.asarray(cnt, dtype=np.int64).reshape(-1)
        b, n = len(nodes), self.graph.n
        if b == 0 or nbr.ndim != 2 or nbr.shape[0] != b or len(cnt) != b or nbr.shape[1] < 1:
            raise ValueError("sample table: expected nodes (B), nbr (B, k), cnt (B) with B >= 1")
        k = int(nbr.shape[1])
        if nodes.min() < 0 or nodes.max() >= n:
            raise ValueError(f"batch nodes must be ids in [0, {n})")
        if cnt.min() < 0 or cnt.max() > k:
            raise ValueError(f"row lengths must lie in [0, {k}]")
        used = np.arange(k)[None, :] < cnt[:, None]
        ids = nbr[used]
        if len(ids) and (ids.min() < 0 or ids.max() >= n):
            raise ValueError(f"the sample table holds an id outside [0, {n})")
        block = np.empty(3 * b + b * k, dtype=np.int32)
        block[:b], block[b:2 * b] = nodes, cnt
        block[2 * b:3 * b] = 0
        if labels is not None:
            labels = np.asarray(labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else labels).reshape(-1)
            if len(labels) != b or not np.isin(labels, (0, 1)).all():
                raise ValueError("labels: expected B values in {0, 1}")
            block[2 * b:3 * b] = labels
        block[3 * b:] = nbr.reshape(-1)
        return SageBatch(torch.from_numpy(block).to(self.table.device), b, k, labels is not None)

    def batch(self, nodes, labels=None) -> SageBatch:
        return self.upload(*self.sample(nodes), labels=labels)

    # ---- launches
    def forward(self, batch: SageBatch, w_enc: torch.Tensor, w_cls: torch.Tensor) -> dict:
        """`ggad_sage_fwd_f32`: combined (B, 2F), emb (B, D), scores (B, 2); with labels also loss (1 + B: the mean, then the
        rows' own) and dscores (B, 2)."""
        b, k, f, d = batch.b, batch.k, self.F, self.D
        dev = self.table.device
        pn, pc = _dptr(batch.nodes, torch.int32, "nodes", b), _dptr(batch.cnt, torch.int32, "cnt", b)
        pb = _dptr(batch.nbr, torch.int32, "nbr", b * k)
        pl = 0 if batch.labels is None else _dptr(batch.labels, torch.int32, "labels", b)
        pe, pw = _dptr(w_enc, torch.float32, "encoder weight", d * 2 * f), _dptr(w_cls, torch.float32, "classifier weight", 2 * d)
        out = {"combined": torch.empty(b, 2 * f, dtype=torch.float32, device=dev),
               "emb": torch.empty(b, d, dtype=torch.float32, device=dev),
               "scores": torch.empty(b, 2, dtype=torch.float32, device=dev)}
        loss = dsc = None
        if batch.labels is not None:
            loss = out["loss"] = torch.empty(1 + b, dtype=torch.float32, device=dev)
            dsc = out["dscores"] = torch.empty(b, 2, dtype=torch.float32, device=dev)
        call("ggad_sage_fwd_f32", self.table.data_ptr(), f, pn, pb, pc, b, k, pe, d, pw, pl, out["combined"].data_ptr(),
             out["emb"].data_ptr(), out["scores"].data_ptr(), 0 if loss is None else loss.data_ptr(),
             0 if dsc is None else dsc.data_ptr())
        self.last = dict(out, batch=batch)
        return out

    def backward(self, combined, emb, dscores, w_cls):
        """`ggad_sage_bwd_f32`: (d_enc (D, 2F), d_cls (2, D))."""
        b, f, d = int(combined.shape[0]), self.F, self.D
        d_enc = torch.empty(d, 2 * f, dtype=torch.float32, device=combined.device)
        d_cls = torch.empty(2, d, dtype=torch.float32, device=combined.device)
        call("ggad_sage_bwd_f32", _dptr(combined, torch.float32, "combined", b * 2 * f), _dptr(emb, torch.float32, "emb", b * d),
             _dptr(dscores, torch.float32, "dscores", b * 2), _dptr(w_cls, torch.float32, "classifier weight", 2 * d), b, f, d,
             self.ws.data_ptr(), d_enc.data_ptr(), d_cls.data_ptr())
        return d_enc, d_cls


class SageScoresFn(torch.autograd.Function):
    """scores (B, 2) of a sampled batch; the gradient goes to the two weights (the feature table is frozen)."""

    @staticmethod
    def forward(ctx, w_enc, w_cls, dev, batch):
        out = dev.forward(batch, w_enc.detach(), w_cls.detach())
        ctx.save_for_backward(out["combined"], out["emb"], w_cls.detach())
        ctx.dev = dev
        return out["scores"]

    @staticmethod
    def backward(ctx, dscores):
        combined, emb, w_cls = ctx.saved_tensors
        d_enc, d_cls = ctx.dev.backward(combined, emb, dscores.contiguous().float(), w_cls)
        return d_enc, d_cls, None, None


class SageStepFn(torch.autograd.Function):
    """The mean cross entropy of a sampled, labelled batch.  Forward and both weight gradients are produced in `forward` (in the manner
    of `_FusedBatchLoss`); `backward` scales them by the incoming gradient."""

    @staticmethod
    def forward(ctx, w_enc, w_cls, dev, batch):
        if batch.labels is None:
            raise ValueError("SageStepFn needs a labelled batch")
        wc = w_cls.detach()
        out = dev.forward(batch, w_enc.detach(), wc)
        d_enc, d_cls = dev.backward(out["combined"], out["emb"], out["dscores"], wc)
        ctx.save_for_backward(d_enc, d_cls)
        return out["loss"][0].clone()

    @staticmethod
    def backward(ctx, g):
        d_enc, d_cls = ctx.saved_tensors
        return d_enc * g, d_cls * g, None, None
