"""Epoch path of the GraphSAGE comparison model (config key `sage_epoch`, on top of `sage_device`): a whole epoch is sampled by ONE
native call (`ggad_sage_sched_epoch`, csrc/sampler.cpp), uploaded once and trained as one chain of launches that never returns to
the host -- per step `k_sage_fwd`, `k_sage_bwd_part` and `k_sage_sum_adam` (csrc/sage.hip), the last of which adds the partial
gradients, applies Adam to both weights and stores the step's loss.  After one eager epoch the chain is a captured graph: one
stream, strictly linear, the per-step row counts its constants (they follow from n_train, batch_size, n_pseudo and num_batches
alone).  Weights, Adam moments, step counters and losses stay in HBM; the host reads the epoch's losses once.

Nothing in an epoch depends on the device's results, so while the device runs the host samples whatever the `random` stream is
asked for next: the next epoch's table (into the other of two pinned tables) or a validation sweep (`SageDevice.presample`).  The
draws stay in the step path's order: same batches, same samples, same generator state after every epoch.

The kernel works in place on the parameters and on `FlatAdam`'s own state tensors, so the optimiser state equals what the step path
leaves and a run may switch paths between epochs.  There is no fallback: what the kernels cannot take raises at construction."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import call
from .fullgraph import FlatAdam
from .sage_device import SageDevice, _dptr
from .sampler import PyCompatRandom


class SageEpoch:
    """Built once per training run.  ``idx_train`` / ``idx_pool``: contiguous int64 arrays, shuffled IN PLACE by every epoch exactly
    as `rng.shuffle` shuffles them on the step path.  ``run_epoch(ahead)`` trains one epoch and returns its `num_batches` losses."""

    def __init__(self, sage: SageDevice, w_enc, w_cls, optimizer: FlatAdam, idx_train, idx_pool, labels, batch_size: int,
                 n_pseudo: int, num_batches: int, capture: bool = True):
        lib = _lib.load()
        if not isinstance(sage, SageDevice) or not isinstance(sage.rng, PyCompatRandom):
            raise ValueError("the GraphSAGE epoch path needs a SageDevice that samples from a PyCompatRandom (rng=...)")
        if not isinstance(optimizer, FlatAdam) or not any(p is w_enc for p in optimizer.params) or \
                not any(p is w_cls for p in optimizer.params):
            raise ValueError("the GraphSAGE epoch path updates the FlatAdam that holds the encoder and the classifier weight")
        f, d, k, g = sage.F, sage.D, sage.k, sage.graph
        if tuple(w_enc.shape) != (d, 2 * f) or tuple(w_cls.shape) != (2, d):
            raise ValueError(f"expected an encoder weight ({d}, {2 * f}) and a classifier weight (2, {d})")
        dev = sage.table.device
        self._pw = (_dptr(w_enc.data, torch.float32, "encoder weight", d * 2 * f), _dptr(w_cls.data, torch.float32, "classifier weight", 2 * d))
        bs, n_pseudo, nb = int(batch_size), int(n_pseudo), int(num_batches)
        if bs < 1 or n_pseudo < 0 or nb < 1:
            raise ValueError("expected batch_size >= 1, n_pseudo >= 0 and num_batches >= 1")
        for name, a in (("idx_train", idx_train), ("idx_pool", idx_pool)):
            if not isinstance(a, np.ndarray) or a.dtype != np.int64 or a.ndim != 1 or not a.flags.c_contiguous:
                raise ValueError(f"{name}: expected a contiguous one-dimensional int64 array (it is shuffled in place)")
            if len(a) and (int(a.min()) < 0 or int(a.max()) >= g.n):
                raise ValueError(f"{name} holds an id outside [0, {g.n})")
        lab = np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int64)
        if len(lab) < g.n:
            raise ValueError("labels: expected one label per node of the graph")
        for a in (idx_train, idx_pool):
            if len(a) and not np.isin(lab[a], (0, 1)).all():
                raise ValueError("labels: expected values in {0, 1}")
        rowptr, col = g.rowptr_host, g.col_host
        if rowptr.dtype != np.int32 or col.dtype != np.int32 or not rowptr.flags.c_contiguous or not col.flags.c_contiguous or \
                len(rowptr) != g.n + 1 or int(rowptr[-1]) != len(col):
            raise ValueError("the graph's host CSR is not a contiguous int32 (rowptr, col) pair")
        if len(col) > 1:                                           # every row strictly ascending: a descent may only sit at a row start
            starts = np.zeros(len(col), dtype=bool)
            starts[rowptr[:-1][np.diff(rowptr) > 0]] = True
            if not (starts[1:] | (col[1:] > col[:-1])).all():
                raise ValueError("a CSR row is not strictly ascending (the sets the set path samples from are filled in ascending order)")
        n_train, n_pool = len(idx_train), len(idx_pool)
        n_p = min(n_pseudo, n_pool)
        lens = [max(0, min((b + 1) * bs, n_train) - b * bs) + n_p for b in range(nb)]
        if min(lens) < 1:
            raise ValueError("a batch of the epoch has no rows (num_batches * batch_size passes the train list and the pool is empty)")
        self.sage, self.opt, self.capture = sage, optimizer, bool(capture)
        self.train, self.pool, self.labels = idx_train, idx_pool, lab
        self.bs, self.n_pseudo, self.nb, self.b_max, self.k = bs, n_pseudo, nb, bs + n_pseudo, k
        self.stride = self.b_max * (3 + k)
        self.lens = np.array(lens, dtype=np.int32)
        self._lens_c = (ctypes.c_int32 * nb)(*lens)
        # Adam state: FlatAdam's own tensors, created here exactly as its first step creates them
        st = []
        for p in (w_enc, w_cls):
            s = optimizer.state.get(p)
            if s is None:
                s = optimizer.state[p] = (torch.zeros_like(p.data), torch.zeros_like(p.data),
                                          torch.zeros(1, dtype=torch.int32, device=p.device))
            st.append(s)
        self._st = st
        bm = self.b_max
        self.table = torch.empty(nb * self.stride, dtype=torch.int32, device=dev)
        self.combined = torch.empty(bm, 2 * f, dtype=torch.float32, device=dev)
        self.emb = torch.empty(bm, d, dtype=torch.float32, device=dev)
        self.scores = torch.empty(bm, 2, dtype=torch.float32, device=dev)
        self.dscores = torch.empty(bm, 2, dtype=torch.float32, device=dev)
        self.rowloss = torch.empty(bm, dtype=torch.float32, device=dev)
        self.ws = torch.empty(int(lib.ggad_sage_bwd_workspace_elems(f, d)), dtype=torch.float32, device=dev)
        self.loss_log = torch.zeros(nb, dtype=torch.float32, device=dev)
        self.host = [torch.empty(nb * self.stride, dtype=torch.int32).pin_memory() for _ in range(2)]
        self._host_np = [h.numpy() for h in self.host]
        self._ready = None                                         # slot of a table sampled ahead
        self._slot = 0
        self._checked = False
        self.graph = None
        self.epochs_run = self.replays = 0

    # ---- host side
    def sample(self, slot: int) -> None:
        """One epoch's shuffles and sample tables into pinned table `slot`."""
        g = self.sage.graph
        _, lens = self.sage.rng.sage_epoch(g.rowptr_host, g.col_host, self.labels, self.train, self.pool, self.bs, self.n_pseudo,
                                           self.nb, self.k, out=self._host_np[slot], checked=self._checked)
        if not np.array_equal(lens, self.lens):
            raise RuntimeError("the scheduler's row counts differ from the constants of the captured epoch")
        self._checked = True                                       # a shuffle moves ids, it does not change them

    # ---- launches
    def _enqueue(self) -> None:
        s, (pe, pc), (se, sc) = self.sage, self._pw, self._st
        call("ggad_sage_epoch_f32", s.table.data_ptr(), s.F, self.table.data_ptr(), self.stride, self._lens_c, self.nb, self.b_max,
             self.k, s.D, pe, se[0].data_ptr(), se[1].data_ptr(), se[2].data_ptr(), pc, sc[0].data_ptr(), sc[1].data_ptr(),
             sc[2].data_ptr(), self.opt.lr, self.opt.wd, self.combined.data_ptr(), self.emb.data_ptr(), self.scores.data_ptr(),
             self.rowloss.data_ptr(), self.dscores.data_ptr(), self.ws.data_ptr(), self.loss_log.data_ptr())

    def run_epoch(self, ahead=None) -> np.ndarray:
        """One epoch: sample (unless the table was sampled ahead), one upload, the chain -- eager the first time, then one replay
        of its capture -- and, while the device runs, ``ahead``: "epoch" samples the next epoch's table, a callable is called
        (a validation sweep's `SageDevice.presample`), None does nothing.  Returns the epoch's losses (float32, one per step)."""
        if self._ready is None:
            self.sample(self._slot)
        else:
            self._slot, self._ready = self._ready, None
        self.table.copy_(self.host[self._slot], non_blocking=True)
        if self.capture and self.epochs_run >= 1:
            if self.graph is None:
                torch.cuda.synchronize()
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph):
                    self._enqueue()
            self.graph.replay()
            self.replays += 1
        else:
            self._enqueue()
        if ahead == "epoch":
            self.sample(1 - self._slot)                            # the upload of the other table ended with the last epoch's read
            self._ready = 1 - self._slot
        elif callable(ahead):
            ahead()
        elif ahead is not None:
            raise ValueError('ahead: "epoch", a callable or None')
        losses = self.loss_log.cpu().numpy().copy()                # the one wait of the epoch
        self.epochs_run += 1
        return losses
