"""Batch sampler: bit-exact CPython ``random`` semantics, native speed.

The reference draws its DGraph batches with ``random.shuffle`` inside the timed loop
(`src/model_handler.py:314` once per epoch over ~1.05 M ids, `:341` once per BATCH over the
55,275-id pseudo-anomaly pool = 28 ms/batch in CPython, a ~7 K nodes/s ceiling for any backend).
``PyCompatRandom`` wraps the MT19937 in libggad_hip.so (`ggad_mt_*`), reproducing the same
permutations for the same seed so that batches are identical to the reference's.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib


class PyCompatRandom:
    def __init__(self, seed: int = 0):
        self._lib = _lib.load()
        self._h = self._lib.ggad_mt_new()
        if not self._h:
            raise MemoryError("ggad_mt_new")
        self.seed(seed)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.ggad_mt_free(h)

    def seed(self, seed: int) -> None:
        seed = abs(int(seed))
        if seed >= 2 ** 64:
            raise ValueError("seeds >= 2^64 are not supported by the native sampler")
        _lib.check(self._lib.ggad_mt_seed_u64(self._h, seed), "ggad_mt_seed_u64")

    @classmethod
    def from_python_state(cls, state) -> "PyCompatRandom":
        """Continue a CPython stream: ``state = random.getstate()``."""
        version, internal, _gauss = state
        if version != 3:
            raise ValueError("unsupported random state version")
        self = cls(0)
        arr = (ctypes.c_uint32 * 624)(*internal[:624])
        _lib.check(self._lib.ggad_mt_set_state(self._h, arr, int(internal[624])), "ggad_mt_set_state")
        return self

    def to_python_state(self):
        arr = (ctypes.c_uint32 * 624)()
        idx = ctypes.c_int32(0)
        _lib.check(self._lib.ggad_mt_get_state(self._h, arr, ctypes.byref(idx)), "ggad_mt_get_state")
        return (3, tuple(int(x) for x in arr) + (int(idx.value),), None)

    def shuffle(self, a: np.ndarray) -> None:
        """random.shuffle(list) on a contiguous int64 array, in place."""
        if a.dtype != np.int64 or not a.flags.c_contiguous:
            raise ValueError("shuffle wants a contiguous int64 array")
        p = a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        _lib.check(self._lib.ggad_mt_shuffle_i64(self._h, p, a.shape[0]), "ggad_mt_shuffle_i64")

    def getrandbits32(self) -> int:
        return int(self._lib.ggad_mt_getrandbits32(self._h))

    # ---- neighbour sampling of the GraphSAGE baseline (`random.sample` over python sets, csrc/sampler.cpp)
    def pyset_order(self, keys) -> np.ndarray:
        """Iteration order of ``set(int(c) for c in keys)`` for strictly ascending, non-negative int32 keys."""
        return pyset_order(keys)

    def sample_rows(self, rowptr: np.ndarray, col: np.ndarray, nodes, num_sample: int):
        """``sorted(random.sample(tuple(adj[v]), num_sample))`` for every v of ``nodes`` in list order, where ``adj[v]`` is the set
        filled with CSR row v in ascending order; a row shorter than ``num_sample`` is taken whole and draws nothing.  Returns
        ``(nbr, cnt)``: (len(nodes), num_sample) int32 padded with -1, and the row lengths.  One call may cover any number of
        batches: the stream depends only on the order of the rows."""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        nodes = np.ascontiguousarray(np.asarray(nodes, dtype=np.int64).reshape(-1))
        k = int(num_sample)
        if k < 1:
            raise ValueError("num_sample must be a positive integer")
        n_nodes = len(rowptr) - 1
        if n_nodes < 1 or int(rowptr[-1]) != len(col):
            raise ValueError("rowptr is not a CSR row pointer of col")
        if len(nodes) and (nodes.min() < 0 or nodes.max() >= n_nodes):
            raise ValueError(f"node ids must lie in [0, {n_nodes})")
        nbr = np.empty((len(nodes), k), dtype=np.int32)
        cnt = np.empty(len(nodes), dtype=np.int32)
        rc = self._lib.ggad_mt_sample_rows(self._h, rowptr.ctypes.data, col.ctypes.data, n_nodes, nodes.ctypes.data, len(nodes), k,
                                           sample_setsize(k), nbr.ctypes.data, cnt.ctypes.data)
        if rc != 0:
            raise ValueError("ggad_mt_sample_rows: a CSR row is not strictly ascending and non-negative (the sets the set path "
                             "samples from are filled in ascending order)")
        return nbr, cnt

    def sage_epoch(self, rowptr: np.ndarray, col: np.ndarray, labels: np.ndarray, train: np.ndarray, pool: np.ndarray, batch_size: int,
                   n_pseudo: int, num_batches: int, num_sample: int, out: np.ndarray = None, checked: bool = False):
        """One epoch of the GraphSAGE device path's schedule in one native call (`ggad_sage_sched_epoch`): ``shuffle(train)``, then
        per batch ``shuffle(pool)``, nodes = ``train[i0:i1] ++ pool[:n_pseudo]`` and their `sample_rows` table.  ``train`` / ``pool``
        (contiguous int64) are shuffled in place.  Returns ``(table, lens)``: table is (num_batches, b_max * (3 + k)) int32 with
        b_max = batch_size + n_pseudo, a row holding nodes[b_max], cnt[b_max], labels[b_max] and nbr[b_max * k]; lens the row
        counts.  ``out``: a contiguous int32 array of that size to write into.  ``checked``: an earlier call on the same graph and
        arrays succeeded, the id and row scans are skipped.  A refusal raises ValueError and draws nothing."""
        for a in (train, pool):
            if not isinstance(a, np.ndarray) or a.dtype != np.int64 or a.ndim != 1 or not a.flags.c_contiguous:
                raise ValueError("train / pool: contiguous one-dimensional int64 arrays (they are shuffled in place)")
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        labels = np.ascontiguousarray(labels, dtype=np.int64)
        k, n_nodes = int(num_sample), len(rowptr) - 1
        if n_nodes < 1 or int(rowptr[-1]) != len(col) or len(labels) < n_nodes:
            raise ValueError("rowptr is not a CSR row pointer of col, or labels is shorter than the graph")
        b_max = int(batch_size) + int(n_pseudo)
        stride = b_max * (3 + max(k, 0))
        if out is None:
            out = np.empty(max(int(num_batches), 0) * stride, dtype=np.int32)
        if out.dtype != np.int32 or not out.flags.c_contiguous or out.size != max(int(num_batches), 0) * stride:
            raise ValueError("out: a contiguous int32 array of num_batches * b_max * (3 + k) elements")
        lens = np.empty(max(int(num_batches), 0), dtype=np.int32)
        rc = self._lib.ggad_sage_sched_epoch(self._h, train.ctypes.data, len(train), pool.ctypes.data, len(pool), int(batch_size),
                                             int(n_pseudo), int(num_batches), rowptr.ctypes.data, col.ctypes.data, n_nodes,
                                             labels.ctypes.data, k, sample_setsize(k) if k >= 1 else 21, int(bool(checked)),
                                             out.ctypes.data, stride, lens.ctypes.data)
        if rc != 0:
            raise ValueError("ggad_sage_sched_epoch refused the epoch before any draw: an id outside the graph in train or pool, "
                             "num_sample < 1, a CSR row that is not strictly ascending, or a batch without rows")
        return out.reshape(int(num_batches), stride), lens


def sample_setsize(k: int) -> int:
    """The population size up to which `random.sample` copies the population into a pool (CPython Lib/random.py), evaluated with
    the interpreter's own expression so that no floating-point logarithm is restated in C."""
    from math import ceil, log
    setsize = 21
    if k > 5:
        setsize += 4 ** ceil(log(k * 3, 4))
    return setsize


def pyset_order(keys) -> np.ndarray:
    keys = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1)
    out = np.empty(len(keys), dtype=np.int32)
    rc = _lib.load().ggad_pyset_order_i32(keys.ctypes.data, len(keys), out.ctypes.data)
    if rc != 0:
        raise ValueError("ggad_pyset_order_i32 wants strictly ascending, non-negative int32 keys")
    return out
