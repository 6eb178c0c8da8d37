"""Keep the best epoch's weights on the device (csrc/select.hip).

    keeper = BestKeeper(model.parameters(), n_epochs, which="auroc", labels_u8=y_val, rows=idx_val)
    ... every epoch, after the optimiser step (inside a captured epoch or not):   keeper.step(model.score(feats, adj))
    ... after training:   keeper.best_epoch, keeper.best_value, keeper.curve(), keeper.load_into(model), keeper.state_dict(model)

`step` is launches only -- a gather of the validation rows, `ggad_rank_metrics_f32` (AUROC / AP as exact counts into eight device
doubles), `ggad_select_decide_f64` (one thread: is this epoch the best so far?) and `ggad_select_copy_f32` per <= 16 parameters
(snapshot them if it is) -- with no host synchronisation and no allocation a capture cannot hold, so the hand-off replays as part of
the training epoch's hipGraph.  Everything the launches touch between epochs is allocated in the constructor, outside any capture.
The strict `>` of the decision keeps the EARLIEST of equal epochs; an epoch whose metric is NaN or whose status is not 0 (one class
only, a NaN score, ...) never wins."""
from __future__ import annotations

import ctypes
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

WHICH = {"auroc": 0, "ap": 1}


class BestKeeper:
    def __init__(self, params, n_epochs, which="auroc", *, labels_u8, rows):
        if which not in WHICH:
            raise ValueError(f"BestKeeper: which = {which!r} is neither 'auroc' nor 'ap'")
        self.params = [p for p in params]
        if not self.params:
            raise ValueError("BestKeeper: no parameters to keep")
        dev = self.params[0].device
        for p in self.params:
            if p.dtype != torch.float32 or p.device != dev or dev.type != "cuda" or not p.is_contiguous():
                raise ValueError("BestKeeper keeps contiguous float32 parameters on one GPU")
        assert not torch.cuda.is_current_stream_capturing(), "BestKeeper allocates: build it before the epoch is captured"
        self.which, self.n_epochs, self.dev = which, int(n_epochs), dev
        lib = _lib.load()
        self.rows = torch.as_tensor(np.asarray(rows, dtype=np.int64).reshape(-1), device=dev)
        labels = labels_u8.detach().cpu().numpy() if isinstance(labels_u8, torch.Tensor) else np.asarray(labels_u8)
        labels = np.ascontiguousarray(labels.reshape(-1).astype(np.uint8))
        if labels.shape != tuple(self.rows.shape):
            raise ValueError(f"BestKeeper: {labels.size} labels for {self.rows.numel()} validation rows")
        if labels.size == 0:
            raise ValueError("BestKeeper: the validation list is empty")
        cap = int(lib.ggad_rank_metrics_max_pos())
        n_pos = int((labels == 1).sum())
        if n_pos > cap:
            raise ValueError(f"BestKeeper: the validation list holds {n_pos} positives, more than ggad_rank_metrics_max_pos() = {cap} "
                             "(ggad_rank_metrics_f32 sorts them in one workgroup; rank_wide is not wired in here)")
        n = int(self.rows.numel())
        with torch.cuda.device(dev):
            self.labels = torch.from_numpy(labels).to(dev)
            self.snapshot = [torch.empty_like(p.data) for p in self.params]        # (arbitrary bits until an epoch is taken)
            self.state4 = torch.tensor([float("nan"), -1.0, 0.0, 0.0], dtype=torch.float64, device=dev)
            self.curve_buf = torch.full((max(1, self.n_epochs), 3), float("nan"), dtype=torch.float64, device=dev)
            self.out8 = torch.zeros(8, dtype=torch.float64, device=dev)
            self.ws = torch.empty(max(1, int(lib.ggad_rank_metrics_workspace_elems(n))), dtype=torch.int32, device=dev)
        self._group = int(lib.ggad_select_max_tensors())

    # ------------------------------------------------------------------ per epoch: launches only
    def step(self, scores):
        """`scores`: the (N,) float32 device scores of all nodes under the weights just updated."""
        if scores.dtype != torch.float32 or scores.dim() != 1 or scores.device != self.dev:
            raise ValueError("BestKeeper.step takes the 1-D float32 scores of all nodes on the parameters' GPU")
        val = scores.index_select(0, self.rows)
        n = int(val.numel())
        _lib.call("ggad_rank_metrics_f32", _lib.ptr(val), _lib.ptr(self.labels), n, 0.0, _lib.ptr(self.out8), _lib.ptr(self.ws))
        _lib.call("ggad_select_decide_f64", _lib.ptr(self.out8), WHICH[self.which], _lib.ptr(self.state4), _lib.ptr(self.curve_buf),
                  self.n_epochs)
        copy_if_taken(self.params, self.snapshot, self.state4, self._group)

    # ------------------------------------------------------------------ after training: one read-back each
    def _state(self):
        return self.state4.cpu().tolist()

    @property
    def best_epoch(self) -> int:
        return int(self._state()[1])

    @property
    def best_value(self) -> float:
        return float(self._state()[0])

    def curve(self) -> np.ndarray:
        """(epochs seen, 3) float64: validation AUROC, AP and the metric kernels' status of every epoch stepped so far."""
        both = torch.cat([self.state4, self.curve_buf.reshape(-1)]).cpu().numpy()
        seen = min(int(both[2]), self.n_epochs)
        return both[4:].reshape(-1, 3)[:seen].copy()

    def _require_taken(self):
        if self.best_epoch < 0:
            raise RuntimeError("BestKeeper: no epoch was taken (every validation metric so far was NaN or had a non-zero status): "
                               "there is no snapshot to use")

    def load_into(self, model=None):
        """Copy the snapshot into the parameters it was taken from (`model`: for symmetry with `state_dict`; the parameters are the
        ones handed to the constructor)."""
        self._require_taken()
        with torch.no_grad():
            for p, s in zip(self.params, self.snapshot):
                p.data.copy_(s)

    def state_dict(self, model):
        """`model.state_dict()` with the snapshot's values in place of every kept parameter (clones; other entries as they are)."""
        self._require_taken()
        at = {id(p): i for i, p in enumerate(self.params)}
        names = {name: at[id(p)] for name, p in model.named_parameters() if id(p) in at}
        out = OrderedDict()
        for key, v in model.state_dict().items():
            out[key] = self.snapshot[names[key]].clone() if key in names else v.detach().clone()
        return out


def copy_if_taken(src, dst, state4, group=None):
    """`ggad_select_copy_f32` over the tensor lists `src` -> `dst` in groups of at most ggad_select_max_tensors(): every group follows
    the same word state4[3], which the one `ggad_select_decide_f64` before them wrote."""
    if group is None:
        group = int(_lib.load().ggad_select_max_tensors())
    for i0 in range(0, len(src), group):
        s, d = src[i0:i0 + group], dst[i0:i0 + group]
        n = len(s)
        arr = ctypes.c_void_p * n
        _lib.call("ggad_select_copy_f32", n, arr(*[_lib.ptr(t.data) for t in s]), arr(*[_lib.ptr(t) for t in d]),
                  (ctypes.c_int64 * n)(*[t.numel() for t in s]), _lib.ptr(state4))
