"""Full-graph GGAD on one MI355X: kernel choice + autograd wrappers over the HIP kernels (the device CSR and its host-side launch
plans are in csr.py).

The reference keeps `adj` and `raw_adj` as dense (1,N,N) tensors and multiplies them densely
(`run.py:98-110`, `model.py:31,151-155`, `run.py:182-188`).  Here they are CSR in HBM
(`FullGraphAdj`), every product is an edge-parallel HIP kernel and autograd only chains those kernels:

    GcnLayerFn   X W^T (MFMA GEMM) -> A_hat . (CSR SpMM, fused bias + PReLU) ; backward = PReLU' , A_hat^T SpMM, GEMMs
    LinearFn     nn.Linear without bias (+ fused ReLU)                       ; backward = two GEMMs
    SpmmRowsFn   A_hat[abn, :] @ emb  (outlier generation, model.py:151-155) ; backward = static transposed sub-CSR
    GgadLossFn   BCE + local-affinity margin + reconstruction (run.py:165-210), affinity as
                 aff_j = r_inv_j <e_hat_j, (R^T e_hat)_j>  evaluated only where the loss reads it
"""
from __future__ import annotations

import os
from collections import namedtuple
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, ptr_rows
from .csr import Csr, _dev_f32, _dev_i32


def _capturing(dev) -> bool:
    return dev.type == "cuda" and torch.cuda.is_current_stream_capturing()


class FullGraphAdj:
    """Everything the full-graph step needs from the two adjacency matrices, built once on the host.

    ``adj_norm``  = normalize_adj(A) + I  (`utils.py:47-54`, `run.py:101`)   -> A_hat and A_hat^T
    ``raw``       = A + I                 (`run.py:100`)                      -> R^T (column view) and 1/colsum
    """

    def __init__(self, adj_norm, raw, device):
        import scipy.sparse as sp
        self.dev = torch.device(device)
        ticket_block(self.dev)                                   # exists before any capture of an epoch on this graph
        an = sp.csr_matrix(adj_norm)
        self.n = an.shape[0]
        self.A = Csr(an, self.dev)
        at = an.T.tocsr()
        self.symmetric = (abs(an - at).nnz == 0)
        self.At = self.A if self.symmetric else Csr(at, self.dev)
        rw = sp.csr_matrix(raw)
        self.raw_host = rw
        self.Rt = Csr(rw.T.tocsr(), self.dev)                   # row j of R^T = column j of raw_adj
        colsum = np.asarray(rw.astype(np.float32).sum(0)).reshape(-1).astype(np.float32)   # torch.sum(raw_adj, 0), fp32
        with np.errstate(divide="ignore"):
            r_inv = np.float32(1.0) / colsum
        r_inv[np.isinf(r_inv)] = 0.0                            # run.py:185-186
        self.r_inv_host = r_inv
        self._abn: Dict[tuple, tuple] = {}
        self._loss: Dict[tuple, tuple] = {}
        self._head: Dict[tuple, object] = {}
        self._ax: Dict[str, object] = {}                         # cached A_hat X of the constant input layer (`cached_aggregate`)
        self._devc: Dict[str, torch.Tensor] = {}                 # small per-node device vectors (`r_inv_dev`, `arange_dev`)

    def r_inv_dev(self) -> torch.Tensor:
        """1 / colsum(raw) (inf -> 0) on the device, one value per node."""
        t = self._devc.get("r_inv")
        if t is None:
            t = self._devc["r_inv"] = _dev_f32(self.r_inv_host, self.dev)
        return t

    def arange_dev(self) -> torch.Tensor:
        t = self._devc.get("arange")
        if t is None:
            t = self._devc["arange"] = torch.arange(self.n, dtype=torch.int32, device=self.dev)
        return t

    @classmethod
    def with_adjacency(cls, base: "FullGraphAdj", rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor):
        """`base` with another A_hat, taken from device arrays (canonical CSR: `Csr.from_device`) that are SYMMETRIC by construction
        (TAM's truncated graphs, `tam_utils.DeviceNsgt.step`): A_hat is its own transpose and nothing is re-checked on the host.
        Everything of the raw adjacency -- `Rt`, `r_inv`, `raw_host`, the small device vectors -- and the `TamHead`s cached on `base` so
        far are base's own objects; what depends on A_hat (row plans, the cached A_hat X) starts empty."""
        self = cls.__new__(cls)
        self.dev, self.n = base.dev, base.n
        self.A = Csr.from_device(rowptr, col, val, (base.n, base.n))
        self.symmetric = True
        self.At = self.A
        self.raw_host, self.Rt, self.r_inv_host = base.raw_host, base.Rt, base.r_inv_host
        self._abn, self._loss, self._ax = {}, {}, {}
        self._head = {k: h for k, h in base._head.items() if k[0] == "tam"}       # (the GGAD head structs hold row plans of A_hat)
        self._devc = base._devc
        return self

    @classmethod
    def from_dense(cls, adj, raw_adj, device):
        import scipy.sparse as sp
        a = adj.detach().cpu().numpy() if isinstance(adj, torch.Tensor) else np.asarray(adj)
        r = raw_adj.detach().cpu().numpy() if isinstance(raw_adj, torch.Tensor) else np.asarray(raw_adj)
        return cls(sp.csr_matrix(a.reshape(a.shape[-2], a.shape[-1])), sp.csr_matrix(r.reshape(r.shape[-2], r.shape[-1])),
                   device)

    def abn_structs(self, abn_idx) -> Tuple[torch.Tensor, Csr]:
        """SpMM plan for the rows A_hat[abn, :] and the transposed sub-matrix (N x A) for its backward."""
        key = tuple(int(i) for i in abn_idx)
        s = self._abn.get(key)
        if s is None:
            idx = np.asarray(key, dtype=np.int64)
            sub = self.A.host[idx, :]
            s = (self.A.plan(idx, key=("rows", key)), Csr(sub.T.tocsr(), self.dev))
            self._abn[key] = s
        return s

    def head_structs(self, normal_idx, abn_idx):
        """Device index lists of the training head (`model.py:140-182`) and their inverse maps (position of node i in the list, -1 if
        absent) for `GgadHeadFn`; None when a list holds a node twice (the fused head assumes duplicate-free lists, as `run.py` draws them)."""
        nrm = np.ascontiguousarray(np.asarray(normal_idx, dtype=np.int64))         # C-speed key: no per-element Python work per forward
        abn = np.ascontiguousarray(np.asarray(abn_idx, dtype=np.int64))
        key = (nrm.size, abn.size, hash(nrm.tobytes()), hash(abn.tobytes()))
        s = self._head.get(key)
        if s is not None and s is not False and not (np.array_equal(s["nrm_host"], nrm) and np.array_equal(s["abn_host"], abn)):
            s = None                                                                 # (hash collision)
        if s is None:
            if len(np.unique(nrm)) != len(nrm) or len(np.unique(abn)) != len(abn) or len(abn) == 0:
                s = False
            else:
                nrm_pos = np.full(self.n, -1, dtype=np.int32)
                abn_pos = np.full(self.n, -1, dtype=np.int32)
                nrm_pos[nrm] = np.arange(len(nrm), dtype=np.int32)
                abn_pos[abn] = np.arange(len(abn), dtype=np.int32)
                rows_plan, sub_t = self.abn_structs(abn_idx)
                s = dict(nrm=_dev_i32(nrm, self.dev), abn=_dev_i32(abn, self.dev), nrm_pos=_dev_i32(nrm_pos, self.dev),
                         abn_pos=_dev_i32(abn_pos, self.dev), n_nrm=len(nrm), n_abn=len(abn), rows_plan=rows_plan, sub_t=sub_t,
                         nrm_host=nrm, abn_host=abn)
            if len(self._head) >= 8:
                self._head.clear()
            self._head[key] = s
        return s or None

    def loss_structs(self, normal_idx, abn_idx):
        """J = normal_idx ++ abn_idx (the rows whose affinity the loss reads) and R[:, J] as an N x |J| CSR."""
        key = (tuple(int(i) for i in normal_idx), tuple(int(i) for i in abn_idx))
        s = self._loss.get(key)
        if s is None:
            J = np.asarray(key[0] + key[1], dtype=np.int64)
            sub = self.Rt.host[J, :]                            # |J| x N : rows of R^T
            # position of every row in the normal / abnormal segment of J (-1: not there): the backward adds c_j S_j to the rows J inside
            # the row-normalisation's backward launch (round 6) instead of a scatter launch per segment
            n_rows = self.Rt.host.shape[1]
            pos_n = np.full(n_rows, -1, dtype=np.int32)
            pos_a = np.full(n_rows, -1, dtype=np.int32)
            nn_ = len(key[0])
            pos_n[J[:nn_]] = np.arange(nn_, dtype=np.int32)
            pos_a[J[nn_:]] = np.arange(nn_, len(J), dtype=np.int32)
            seg_unique = len(np.unique(J[:nn_])) == nn_ and len(np.unique(J[nn_:])) == len(J) - nn_
            # a node twice INSIDE a list (never drawn by run.py): the scatter-add of c_j S_j onto the rows J goes in rounds, round k
            # holding the k-th occurrence of every node -- duplicate-free, so no two waves of one launch write the same row
            rounds = None
            if not seg_unique:
                order = np.argsort(J, kind="stable")
                first = np.concatenate(([True], J[order][1:] != J[order][:-1]))
                start = np.maximum.accumulate(np.where(first, np.arange(len(J)), 0))
                occ = np.empty(len(J), dtype=np.int64)
                occ[order] = np.arange(len(J)) - start
                rounds = [(_dev_i32(np.flatnonzero(occ == k), self.dev), _dev_i32(J[occ == k], self.dev)) for k in range(int(occ.max()) + 1)]
            s = dict(J=_dev_i32(J, self.dev), n_normal=len(key[0]), n_out=len(key[1]), distinct=bool(len(np.unique(J)) == len(J)),
                     r_inv_J=_dev_f32(self.r_inv_host[J], self.dev), RJ=Csr(sub.T.tocsr(), self.dev),
                     Rt_plan=self.Rt.plan(J, key=("rows", key)), pos_n=_dev_i32(pos_n, self.dev), pos_a=_dev_i32(pos_a, self.dev),
                     seg_unique=bool(seg_unique), rounds=rounds)
            self._loss[key] = s
        return s


# ------------------------------------------------------------------------------------------------ kernels
def gemm(A: torch.Tensor, B: torch.Tensor, trans_a: bool, trans_b: bool, bias=None, relu: bool = False, out=None) -> torch.Tensor:
    """C = op(A) op(B) on the matrix cores; A, B row-major 2-D fp32.  `out`: an (M, N) destination with unit column stride (its
    row stride may exceed N: `padded_rows`)."""
    A, B = A.contiguous(), B.contiguous()
    M, K = (A.shape[1], A.shape[0]) if trans_a else (A.shape[0], A.shape[1])
    K2, N = (B.shape[1], B.shape[0]) if trans_b else (B.shape[0], B.shape[1])
    if K != K2:
        raise ValueError("gemm shape mismatch")
    sam, sak = (1, A.shape[1]) if trans_a else (A.shape[1], 1)
    sbk, sbn = (1, B.shape[1]) if trans_b else (B.shape[1], 1)
    C = out if out is not None else torch.empty(M, N, dtype=torch.float32, device=A.device)
    if tuple(C.shape) != (M, N) or C.stride(1) != 1 or C.stride(0) < N or C.dtype != torch.float32:
        raise ValueError("gemm: out must be (M, N) fp32 with unit column stride")
    lib = _lib.load()
    ws_n = int(lib.ggad_gemm_workspace_elems(M, N, K))
    ws = torch.empty(ws_n, dtype=torch.float32, device=A.device) if ws_n else None
    call("ggad_gemm_f32", ptr(A), ptr(B), ptr_rows(C), M, N, K, sam, sak, sbk, sbn, C.stride(0), ptr(bias) if bias is not None else 0,
         1 if relu else 0, ptr(ws) if ws is not None else 0)
    return C


_XS_WORKSPACE = {}
Route = namedtuple("Route", "kind tables")          # what `spmm_route` returns: "rowline" / "ring" / "panel" / "sliced" / "rowslice" / "seg" + its plan


def _use_sliced(csr: Csr, p, X: torch.Tensor) -> bool:
    """Dense neighbourhoods gathered from an operand that does not fit an XCD's L2: the XCD-sliced kernel (fullgraph.hip).
    GGAD_SPMM_SLICED=0 / 1 forces the choice (A/B measurements)."""
    force = os.environ.get("GGAD_SPMM_SLICED")
    if force is not None:
        return force == "1"
    w = X.shape[1]
    return w >= 64 and X.shape[0] * w * 4 >= (6 << 20) and p["n_seg"] > 0 and p.get("nnz", csr.nnz) >= 24 * p["n_seg"]


def _use_rowslice(csr: Csr, p, X: torch.Tensor) -> bool:
    """Sparse neighbourhoods gathered from a wide operand that no XCD's L2 holds (Reddit, Photo): the column-sliced six-rows-per-wave
    kernel (k_spmm_rowslice).  GGAD_SPMM_ROWSLICE=0 / 1 forces the choice (A/B measurements)."""
    force = os.environ.get("GGAD_SPMM_ROWSLICE")
    if force is not None:
        return force == "1"
    w = X.shape[1]
    # A smaller operand too when the rows are short (< 32 entries per output row: the transposed loss-row products of Reddit / Photo, a
    # 1.4-2.2 MB operand, took the segment kernel + its combine: Photo 0.555 -> 0.542 ms, Reddit 0.496 -> 0.488); with longer rows the
    # segment kernel stays (Amazon / T-Finance: +0.5 / +1.2 % with this kernel, scripts/rowslice_threshold_ab.sh)
    if w < 160:
        return False
    nnz = p.get("nnz", csr.nnz)
    # (short rows AND short columns: the transposed head product of T-Finance has 7 entries per output row but 540 per source row)
    return X.shape[0] * w * 4 >= (4 << 20) or (nnz < 32 * max(int(p["n_out"]), 1) and nnz < 64 * max(int(X.shape[0]), 1))


def _use_rowline(X: torch.Tensor) -> bool:
    """A row-strided operand the line-granular kernel (k_spmm_rowslice<8, 8, true>) takes as it is: 128-byte aligned rows."""
    return bool(_lib.load().ggad_spmm_rowline_supported(ptr_rows(X), X.stride(0), X.shape[1], X.shape[0]))


def padded_rows(n_rows: int, W: int, dev, consumer=None):
    """An (n_rows, W) fp32 matrix for a producer kernel to fill.  When the product that will read it -- `consumer` = (csr, plan) --
    is one of the sparse-neighbourhood products (what `_use_rowslice` selects: Reddit, Photo), its rows start on 128-byte lines
    (a view of a matrix with the row stride rounded up to 32 floats; the padding columns are never read) and `spmm` then runs the
    line-granular kernel; a plain contiguous matrix otherwise.  GGAD_SPMM_ROWLINE=0: always contiguous."""
    plain = torch.empty(n_rows, W, dtype=torch.float32, device=dev)
    ld = (W + 31) // 32 * 32
    if consumer is not None and ld != W and os.environ.get("GGAD_SPMM_ROWLINE", "1") != "0":
        csr, p = consumer
        p = p if p is not None else csr.plan()
        X = torch.empty(n_rows, ld, dtype=torch.float32, device=dev)[:, :W]
        if spmm_route(csr, p, X).kind == "rowline" and spmm_route(csr, p, plain).kind == "rowslice":      # (only where padding swaps the two)
            return X
    return plain


def _panel_eligible(csr: Csr, p, X: torch.Tensor) -> bool:
    """Products with dense neighbourhoods: candidates for the LDS kernels (k_spmm_ring, k_spmm_panel), which `spmm_route` takes where
    the device has the LDS and a plan can be built.  GGAD_SPMM_PANEL=0 turns them off, =1 forces them wherever a plan can be built."""
    force = os.environ.get("GGAD_SPMM_PANEL")
    if force == "0" or X.shape[0] != csr.shape[1]:
        return False
    nnz = p.get("nnz", csr.nnz)
    # (the floors were 2^20 entries and 64 per output row: the products over Amazon's loss rows -- 1,751 rows x 368 entries, and their transpose
    #  with 54 entries per row -- then took the sliced / segment kernels at ~80 ps per entry: epoch 0.725 against 0.694-0.698 ms with the ring,
    #  scripts/panel_threshold_ab.sh; sparse neighbourhoods (Reddit, Photo: 16 per row) fail the per-row test and keep their kernels)
    min_nnz = int(os.environ.get("GGAD_SPMM_PANEL_MIN_NNZ", str(1 << 18)))
    min_row = int(os.environ.get("GGAD_SPMM_PANEL_MIN_ROW", "32"))
    return force == "1" or (X.shape[1] >= 64 and nnz >= min_row * p["n_out"] and nnz >= min_nnz)


def _lds_kernels(dev) -> Tuple[bool, bool]:
    """(panel, ring): whether `dev` gives a workgroup the LDS of k_spmm_panel (159 KB) / of k_spmm_ring."""
    with torch.cuda.device(dev):
        return bool(_lib.load().ggad_spmm_panel_available()), bool(_lib.load().ggad_spmm_ring_available())


def spmm_route(csr: Csr, p, X: torch.Tensor) -> Route:
    """(kind, tables): the kernel `spmm` runs for the rows `p` (a `csr.plan`) of `csr` times `X`, and the plan its launcher takes.
    The ONLY place that holds the precedence (top to bottom).  The switches are read on every call: nothing is cached
    but the plans.  A ring / panel plan that does not qualify (values that do not factor, fill, rounds, stream size) is None."""
    w = X.shape[1]
    if X.dim() == 2 and X.stride(1) == 1 and X.stride(0) > w and csr.nnz > 0 and _use_rowline(X):
        return Route("rowline", csr.rowslice_plan(p, lines=True))
    if _panel_eligible(csr, p, X):
        panel, ring = _lds_kernels(X.device)          # (without the panel's 159 KB of LDS per workgroup: the sliced kernel)
        kinds = ("ring", "panel") if ring and os.environ.get("GGAD_SPMM_RING", "1") != "0" else ("panel",)
        cache = None if p.get("rows") is None else p.setdefault("panel_cache", {})     # row subset: the plan lives on the segment plan
        for kind in kinds if panel else ():
            plan = (Csr.ring_plan if kind == "ring" else Csr.panel_plan)(csr, (w // 4 + 7) // 8, p.get("rows"), cache)
            if plan is not None:
                return Route(kind, plan)
    if _use_sliced(csr, p, X):
        return Route("sliced", csr.sliced_plan(p))
    if _use_rowslice(csr, p, X):
        return Route("rowslice", csr.rowslice_plan(p))
    return Route("seg", p)


def _xs_workspace(X: torch.Tensor) -> torch.Tensor:
    n_ws = int(_lib.load().ggad_spmm_sliced_workspace_elems(X.shape[0], X.shape[1]))
    key = (str(X.device), torch.cuda.current_stream(X.device).cuda_stream)
    xs = _XS_WORKSPACE.get(key)
    if xs is None or xs.numel() < n_ws:          # one staging buffer per stream: consumed by the launch that follows its fill
        xs = _XS_WORKSPACE[key] = torch.empty(n_ws, dtype=torch.float32, device=X.device)
    return xs


def _part_buffer(p, W: int, dev):
    """Partial sums of the rows that are split into several segments (cached on the plan); None when no row is."""
    part = p.get("part")
    if p["n_multi"] > 0 and (part is None or part.numel() < p["n_seg"] * W):
        part = p["part"] = torch.empty(p["n_seg"] * W, dtype=torch.float32, device=dev)
    return part


# One launcher per kind of `spmm_route`, called as (csr, the route's tables, X, W, opt): nothing but that kernel's arguments.
_LAUNCH = {
    "rowline": lambda csr, rs, X, W, opt: call(
        "ggad_spmm_rowline_f32", ptr(csr.entries()), ptr(rs["unit_tab"]), rs["n_units"], ptr(rs["long_tab"]), rs["n_long"],
        ptr(rs["hub_tab"]), rs["n_hub"], ptr_rows(X), X.stride(0), W, X.shape[0], *opt),
    "ring": lambda csr, pp, X, W, opt: call(
        "ggad_spmm_ring_f32", ptr(pp["wg"]), pp["n_wg"], ptr(pp["wave_sb"]), ptr(pp["idx"]), ptr(pp["ctl"]), ptr(pp["row_tab"]), pp["n_phases"],
        pp["walkers"], ptr(pp["cs"]), ptr(pp["rs"]), ptr(pp["diag"]), ptr(X), W, W, X.shape[0], ptr(_xs_workspace(X)), *opt),
    "panel": lambda csr, pp, X, W, opt: call(
        "ggad_spmm_panel_f32", ptr(pp["wg"]), pp["n_wg"], ptr(pp["dir"]), ptr(pp["stream"]), ptr(pp["row_tab"]), pp["n_chunks"],
        ptr(pp["cs"]), ptr(pp["rs"]), ptr(pp["diag"]), ptr(X), W, W, X.shape[0], ptr(_xs_workspace(X)), *opt),
    "sliced": lambda csr, p, X, W, opt: call(
        "ggad_spmm_sliced_f32", ptr(csr.col), ptr(csr.val), ptr(p["seg_beg"]), ptr(p["seg_end"]), ptr(p["seg_out"]), p["n_seg"],
        ptr(p["multi_row"]), ptr(p["multi_first"]), ptr(p["multi_count"]), p["n_multi"], ptr(X), W, W, X.shape[0], ptr(_xs_workspace(X)),
        *opt, ptr(_part_buffer(p, W, X.device))),
    "rowslice": lambda csr, rs, X, W, opt: call(
        "ggad_spmm_rowslice_f32", ptr(csr.rowptr), ptr(csr.col), ptr(csr.val), ptr(rs["unit_rows"]), ptr(rs["unit_out"]), rs["n_units"],
        ptr(rs["long_rows"]), ptr(rs["long_out"]), rs["n_long"], ptr(rs["hub_rows"]), ptr(rs["hub_out"]), rs["n_hub"], ptr(X), W, W, *opt),
    "seg": lambda csr, p, X, W, opt: call(
        "ggad_spmm_csr_f32", ptr(csr.col), ptr(csr.val), ptr(p["seg_beg"]), ptr(p["seg_end"]), ptr(p["seg_out"]), p["n_seg"],
        ptr(p["multi_row"]), ptr(p["multi_first"]), ptr(p["multi_count"]), p["n_multi"], ptr(X), W, W, *opt, ptr(_part_buffer(p, W, X.device))),
}


def spmm(csr: Csr, X: torch.Tensor, plan=None, bias=None, prelu_a=None, want_pre=False, out=None):
    """out = act(csr[rows] @ X + bias); `plan` = csr.plan(...) selects the rows (default: all).  `out`: destination (and shape of
    the pre-activation copy) with unit column stride; its row stride may exceed W."""
    W = X.shape[1]
    p = plan if plan is not None else csr.plan()
    if out is None:
        out = torch.empty(p["n_out"], W, dtype=torch.float32, device=X.device)
    elif tuple(out.shape) != (p["n_out"], W) or out.dtype != torch.float32:
        raise ValueError("spmm: out must be (rows, W) fp32")
    pre = torch.empty_strided(out.shape, out.stride(), dtype=torch.float32, device=X.device) if want_pre else None
    opt = (ptr(bias), ptr(prelu_a), ptr_rows(out), out.stride(0), ptr_rows(pre) if pre is not None else 0)
    kind, tables = spmm_route(csr, p, X)
    _LAUNCH[kind](csr, tables, X if kind == "rowline" else X.contiguous(), W, opt)      # (padded rows: see padded_rows())
    return (out, pre) if want_pre else out


# ------------------------------------------------------------------------------------------------ autograd
def _reorder_layer(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """A_hat (X W^T) == (A_hat X) W^T: when the layer's input is a constant (the feature matrix: no gradient) narrower than its
    output, A_hat X is computed once and cached, and the layer needs no SpMM at all -- neither forward nor backward (the weight
    gradient is dZ^T (A_hat X)).  T-Finance: F = 10 against H = 300, two of the five N x N x 300 products of an epoch go.
    Same operations, the two products associated the other way round: results agree to fp32 round-off.
    GGAD_GCN_REORDER=0 keeps the reference's order."""
    return (not x.requires_grad) and x.shape[1] < weight.shape[0] and os.environ.get("GGAD_GCN_REORDER", "1") != "0"


def cached_aggregate(adj: "FullGraphAdj", x: torch.Tensor) -> torch.Tensor:
    """A_hat X for a constant X (N x F), computed once per (X storage, version) with the SpMM kernel on zero-padded columns."""
    # the cache entry keeps a reference to the tensor: its storage stays alive, so the caching allocator cannot hand the same
    # address (with version 0) to another tensor of the same shape while the entry exists
    key = (x.data_ptr(), x._version, tuple(x.shape))
    hit = adj._ax.get("key") == key
    if not hit:
        f = x.shape[1]
        fp = (f + 3) // 4 * 4
        xp = x if fp == f else torch.cat((x, torch.zeros(x.shape[0], fp - f, device=x.device)), 1)
        with torch.no_grad():
            ax = spmm(adj.A, xp.contiguous())
        # a second copy with zero columns up to a multiple of 4 (at least 20: two 16-k steps of the slab kernel) when F is not one: the
        # layer's product then takes the slab kernel instead of the generic tiles (Amazon F = 25: 13.1 us, T-Finance F = 10: 23.4 us)
        axp = None
        if f % 4 != 0 and f <= 64 and os.environ.get("GGAD_PAD_FEATURES", "1") != "0":
            wp = max(fp, 20)
            axp = torch.zeros(x.shape[0], wp, dtype=torch.float32, device=x.device)
            axp[:, :f] = ax[:, :f]
        adj._ax = {"key": key, "x": x, "ax": ax[:, :f].contiguous(), "axp": axp}
    return adj._ax["ax"]


def padded_constant(adj: "FullGraphAdj", x: torch.Tensor):
    """A constant layer input (the feature matrix) whose width is not a multiple of 4 -- Photo's 745 -- with zero columns up to the next
    one, made once per (storage, version): the products of that layer then move 16-byte chunks (LDS-DMA tiles, split-K) instead of
    single floats (x W^T 62 -> 56 us, dW = dZ^T x 74 -> 54 us at Photo size, scripts/gemm_k745_time.py).  None when x needs nothing."""
    f = x.shape[1]
    if f % 4 == 0 or f < 32 or x.requires_grad or x.dim() != 2 or os.environ.get("GGAD_PAD_FEATURES", "1") == "0":
        return None
    key = (x.data_ptr(), x._version, tuple(x.shape))
    ent = adj.__dict__.get("_xpad")
    if ent is None or ent["key"] != key:
        xp = torch.zeros(x.shape[0], (f + 3) // 4 * 4, dtype=torch.float32, device=x.device)
        xp[:, :f] = x
        ent = adj.__dict__["_xpad"] = {"key": key, "x": x, "xp": xp}      # (keeps x alive: see cached_aggregate)
    return ent["xp"]


_PRELU_ONE = os.environ.get("GGAD_PRELU_ONE", "1") != "0"            # 0: k_prelu_bwd_v4 + the trailing k_prelu_bwd_final launch (A/B)
_TICKET_BLOCKS: Dict[str, torch.Tensor] = {}


def ticket_block(device) -> torch.Tensor:
    """The device's ticket words of the single-launch reductions (csrc/handoff.h): zeroed int32, as many as the largest user needs.

    Contract: the kernels leave the block zero, and all ticket-bearing launches of a device are ordered on one stream or in one
    captured chain, so they can share it.  Allocated on first use, which must be outside a capture (`FullGraphAdj.__init__` sees
    to it): a tensor made inside one would live in the graph's private pool with a fill node in every replay."""
    device = torch.device(device)
    t = _TICKET_BLOCKS.get(str(device))
    if t is None:
        if _capturing(device):
            raise RuntimeError("ticket_block({}) would allocate inside a stream capture: build the FullGraphAdj (or call "
                               "ticket_block) before capturing".format(device))
        lib = _lib.load()
        n = max(int(lib.ggad_prelu_bwd_one_tickets()), int(lib.ggad_dominant_tickets()), 1)
        t = torch.zeros((n + 3) // 4 * 4, dtype=torch.int32, device=device)
        t = _TICKET_BLOCKS[str(device)] = _TICKET_BLOCKS.setdefault(str(t.device), t)      # "cuda" and "cuda:0": one block
    return t


class GcnLayerFn(torch.autograd.Function):
    """out = PReLU(A_hat (X W^T) + b)   (reference GCN.forward, `model.py:26-35`)."""

    @staticmethod
    def forward(ctx, x, weight, bias, prelu_a, adj: FullGraphAdj):
        ctx.reordered = _reorder_layer(x, weight)
        if ctx.reordered:
            ax = cached_aggregate(adj, x)
            axp = adj._ax.get("axp")
            a_op = ax if axp is None else axp                                # (zero columns behind A_hat X and W: the same sums)
            if axp is None:
                w_op = weight.contiguous()
            else:                                                            # the weight behind zero columns: ONE copy into a kept buffer
                wkey = (weight.data_ptr(), tuple(weight.shape), axp.shape[1])
                ent = adj.__dict__.get("_wpad")
                if ent is None or ent[0] != wkey:
                    ent = adj.__dict__["_wpad"] = (wkey, torch.zeros(weight.shape[0], axp.shape[1], dtype=torch.float32, device=weight.device))
                w_op = ent[1]
                w_op[:, :weight.shape[1]].copy_(weight.detach())
            z = torch.empty(a_op.shape[0], w_op.shape[0], dtype=torch.float32, device=a_op.device)
            out = torch.empty_like(z)
            # product, bias and activation in one launch when the slab kernel takes the shape (ggad_linear_prelu_f32), else two
            rc = _lib.GGAD_E_UNSUPPORTED
            if os.environ.get("GGAD_LINEAR_PRELU_FUSED", "1") != "0":
                rc = int(_lib.load().ggad_linear_prelu_f32(ptr(a_op), a_op.stride(0), ptr(w_op), w_op.stride(0), ptr(bias) if bias is not None else 0,
                                                           ptr(prelu_a), a_op.shape[0], w_op.shape[0], a_op.shape[1], ptr(z), z.stride(0),
                                                           ptr(out), out.stride(0), _lib.current_stream()))
            if rc == _lib.GGAD_E_UNSUPPORTED:                                # nothing was launched: the documented fallback
                z = gemm(a_op, w_op, False, True, bias=bias, out=z)          # (A_hat X) W^T + b
                call("ggad_prelu_fwd_f32", ptr(z), ptr(prelu_a), z.numel(), ptr(out))
            else:
                _lib.check(rc, "ggad_linear_prelu_f32")
            ctx.save_for_backward(ax, weight, z, prelu_a)
        else:
            xq = padded_constant(adj, x)
            if xq is not None:                                               # (zero columns behind x and W: the same sums)
                wq = torch.nn.functional.pad(weight, (0, xq.shape[1] - x.shape[1]))
                t = gemm(xq, wq, False, True, out=padded_rows(x.shape[0], weight.shape[0], x.device, (adj.A, None)))
            else:
                t = gemm(x, weight, False, True, out=padded_rows(x.shape[0], weight.shape[0], x.device, (adj.A, None)))      # seq_fts = fc(seq)   model.py:27
            out, z = spmm(adj.A, t, bias=bias, prelu_a=prelu_a, want_pre=True)   # bmm(adj, .) + bias, act  model.py:31-35
            ctx.save_for_backward(x, weight, z, prelu_a)
        ctx.adj = adj
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight, z, prelu_a = ctx.saved_tensors
        adj = ctx.adj
        g = g.contiguous()
        M, W = z.shape
        lib = _lib.load()
        S = int(lib.ggad_prelu_bwd_splits(M))
        ws = torch.empty(int(lib.ggad_prelu_bwd_one_workspace_elems(M, W)) if _PRELU_ONE else 2 * S * W, dtype=torch.float32, device=z.device)
        dz = torch.empty_like(z) if ctx.reordered else padded_rows(M, W, z.device, (adj.At, None))      # read by A_hat^T dZ below
        db = torch.empty(W, dtype=torch.float32, device=z.device)
        da = torch.empty(1, dtype=torch.float32, device=z.device)
        if _PRELU_ONE:                                                       # round 6: the column reduction inside the same launch
            call("ggad_prelu_bwd_one_f32", ptr(g), ptr(z), ptr(prelu_a), M, W, ptr_rows(dz), dz.stride(0), ptr(db), ptr(da), ptr(ws),
                 ptr(ticket_block(z.device)))
        else:
            call("ggad_prelu_bwd_ld_f32", ptr(g), ptr(z), ptr(prelu_a), M, W, ptr_rows(dz), dz.stride(0), ptr(db), ptr(da), ptr(ws))
        if ctx.reordered:                                                    # x holds A_hat X here
            dw = gemm(dz, x, True, False)                                    # (H x N)(N x F), no transposed product needed
            return None, dw, (db if ctx.has_bias else None), da.view_as(prelu_a), None
        dt = spmm(adj.At, dz)                                                # A_hat^T dZ
        xq = padded_constant(adj, x)
        dw = gemm(dt, x, True, False) if xq is None else gemm(dt, xq, True, False)[:, :x.shape[1]].contiguous()      # (H x N)(N x F)
        dx = gemm(dt, weight, False, False) if ctx.needs_input_grad[0] else None
        return dx, dw, (db if ctx.has_bias else None), da.view_as(prelu_a), None


class LinearFn(torch.autograd.Function):
    """y = [relu](x W^T): nn.Linear(bias=False) of the scorer MLP / fc4 (`model.py:156,176-180`)."""

    @staticmethod
    def forward(ctx, x, weight, relu: bool):
        y = gemm(x, weight, False, True, relu=relu)
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
        dw = gemm(dz, x, True, False)
        return dx, dw, None


def mlp_score_supported(w1: torch.Tensor, w2: torch.Tensor, w3: torch.Tensor) -> bool:
    """The fused scorer-MLP kernels (csrc/mlp.hip) take these weights?  GGAD_MLP_FUSED=0 turns them off (A/B: the three GEMMs)."""
    if os.environ.get("GGAD_MLP_FUSED", "1") == "0" or w3.shape[0] != 1 or w1.shape[0] != w2.shape[1] or w2.shape[0] != w3.shape[1]:
        return False
    return bool(_lib.load().ggad_mlp_score_supported(int(w1.shape[1]), int(w1.shape[0]), int(w2.shape[0])))


def mlp_score_fwd(x: torch.Tensor, w1, w2, w3):
    """(f1, f2, f3) = relu(x W1^T), relu(f1 W2^T), f2 w3^T in ONE launch (model.py:176-180)."""
    x, w1, w2, w3 = x.contiguous(), w1.contiguous(), w2.contiguous(), w3.contiguous()
    r, h = x.shape
    h1, h2 = w1.shape[0], w2.shape[0]
    if w1.shape[1] != h or w2.shape[1] != h1 or tuple(w3.shape) != (1, h2):
        raise ValueError(f"mlp_score shape mismatch: x {tuple(x.shape)}, w1 {tuple(w1.shape)}, w2 {tuple(w2.shape)}, w3 {tuple(w3.shape)}")
    f1 = torch.empty(r, h1, dtype=torch.float32, device=x.device)
    f2 = torch.empty(r, h2, dtype=torch.float32, device=x.device)
    f3 = torch.empty(r, 1, dtype=torch.float32, device=x.device)
    call("ggad_mlp_score_fwd_f32", ptr(x), h, r, h, h1, h2, ptr(w1), ptr(w2), ptr(w3), ptr(f1), ptr(f2), ptr(f3))
    return f1, f2, f3


def mlp_score_dgrad(g3: torch.Tensor, f1, f2, w1, w2, w3, dx_add: Optional[torch.Tensor] = None):
    """(dz2, dz1, dx): the data gradients of the scorer MLP in ONE launch; dx = dz1 W1 (+ dx_add)."""
    g3 = g3.contiguous().reshape(-1)
    r, h1 = f1.shape
    h2, h = f2.shape[1], w1.shape[1]
    if (f2.shape[0] != r or g3.numel() != r or tuple(w1.shape) != (h1, h) or tuple(w2.shape) != (h2, h1) or tuple(w3.shape) != (1, h2)
            or (dx_add is not None and tuple(dx_add.shape) != (r, h))):
        raise ValueError(f"mlp_score_dgrad shape mismatch: g3 {g3.numel()}, f1 {tuple(f1.shape)}, f2 {tuple(f2.shape)}, "
                         f"w1 {tuple(w1.shape)}, w2 {tuple(w2.shape)}, w3 {tuple(w3.shape)}")
    f1, f2 = f1.contiguous(), f2.contiguous()
    dz2, dz1 = torch.empty_like(f2), torch.empty_like(f1)
    dx = torch.empty(r, h, dtype=torch.float32, device=f1.device)
    if dx_add is not None:
        dx_add = dx_add.contiguous()
    call("ggad_mlp_score_dgrad_f32", ptr(g3), r, h, h1, h2, ptr(f1), ptr(f2), ptr(w1.contiguous()), ptr(w2.contiguous()), ptr(w3.contiguous()),
         ptr(dz2), ptr(dz1), ptr(dx), h, ptr(dx_add) if dx_add is not None else 0, h)
    return dz2, dz1, dx


def mlp_score_wgrad(x: torch.Tensor, dz1, f1, dz2, f2, g3):
    """(dW1, dW2, dW3) = (dz1^T x, dz2^T f1, g3^T f2): the three weight gradients of the scorer in one launch + one reduction
    (`ggad_mlp_score_wgrad_f32`; they were three split-K GEMMs + three reductions, 47 us of a Reddit epoch)."""
    r, h = x.shape
    h1, h2 = f1.shape[1], f2.shape[1]
    g3 = g3.contiguous().reshape(-1)
    dz1, f1, dz2, f2 = dz1.contiguous(), f1.contiguous(), dz2.contiguous(), f2.contiguous()
    if tuple(dz1.shape) != (r, h1) or tuple(dz2.shape) != (r, h2) or f1.shape[0] != r or f2.shape[0] != r or g3.numel() != r:
        raise ValueError("mlp_score_wgrad shape mismatch")
    dev = x.device
    dw1 = torch.empty(h1, h, dtype=torch.float32, device=dev)
    dw2 = torch.empty(h2, h1, dtype=torch.float32, device=dev)
    dw3 = torch.empty(1, h2, dtype=torch.float32, device=dev)
    ws = torch.empty(int(_lib.load().ggad_mlp_score_wgrad_workspace_elems(r, h, h1, h2)), dtype=torch.float32, device=dev)
    call("ggad_mlp_score_wgrad_f32", ptr_rows(x), x.stride(0), ptr(dz1), ptr(f1), ptr(dz2), ptr(f2), ptr(g3), r, h, h1, h2,
         ptr(dw1), ptr(dw2), ptr(dw3), ptr(ws))
    return dw1, dw2, dw3


class MlpScoreFn(torch.autograd.Function):
    """f_3 = fc3(relu(fc2(relu(fc1(x))))) (`model.py:176-180`) on the fused kernels: one launch forward, one for the data gradients,
    three split-K GEMMs for the weight gradients."""

    @staticmethod
    def forward(ctx, x, w1, w2, w3):
        f1, f2, f3 = mlp_score_fwd(x, w1, w2, w3)
        ctx.save_for_backward(x, f1, f2, w1, w2, w3)
        return f3

    @staticmethod
    def backward(ctx, g):
        x, f1, f2, w1, w2, w3 = ctx.saved_tensors
        g = g.contiguous()
        dz2, dz1, dx = mlp_score_dgrad(g, f1, f2, w1, w2, w3)
        if os.environ.get("GGAD_MLP_WGRAD_FUSED", "1") != "0" and x.stride(1) == 1:
            dw1, dw2, dw3 = mlp_score_wgrad(x, dz1, f1, dz2, f2, g)
        else:
            dw1, dw2, dw3 = gemm(dz1, x, True, False), gemm(dz2, f1, True, False), gemm(g.reshape(-1, 1), f2, True, False)
        return (dx if ctx.needs_input_grad[0] else None, dw1, dw2, dw3)


class SpmmRowsFn(torch.autograd.Function):
    """A_hat[rows, :] @ emb  (`model.py:151-155`)."""

    @staticmethod
    def forward(ctx, emb, adj: FullGraphAdj, rows_plan, sub_t: Csr):
        ctx.sub_t = sub_t
        return spmm(adj.A, emb, plan=rows_plan)

    @staticmethod
    def backward(ctx, g):
        return spmm(ctx.sub_t, g.contiguous()), None, None, None


_HEAD_LEAN = os.environ.get("GGAD_HEAD_LEAN", "1") != "0"            # 0: the round-5 glue (separate gathers, emb_out as a second N x H tensor)


class GgadHeadFn(torch.autograd.Function):
    """The training forward from `emb` on (`model.py:140-182`) as ONE autograd node:

        emb_abnormal = emb[abn] + noise                                   :141-145
        emb_con      = relu(fc4(A_hat[abn, :] emb))                       :151-156
        emb_combine  = cat(emb[normal], emb_con)                          :159
        f_3          = fc3(relu(fc2(relu(fc1(emb_combine)))))             :176-180
        emb_out      = emb with rows abn replaced by emb_con              :182

    Same products as the op-by-op path (`Model._head_unfused`: `LinearFn`, `SpmmRowsFn`, torch indexing); what is fused is the glue
    -- gather / add / cat / index_copy forward, and in the backward the gradient accumulation over the five consumers of `emb` and
    the three of `emb_con`, which autograd does with one full-tensor kernel per term (~35 launches of 5 us per Reddit epoch).
    The sums of gradient terms are formed in one fixed order (`k_head_con_grad`, `k_head_emb_grad`); autograd's order is another,
    so the two paths agree to fp32 round-off, not bit for bit (tests/test_fullgraph_gpu.py)."""

    @staticmethod
    def forward(ctx, emb, noise, w4, w1, w2, w3, adj: FullGraphAdj, hs):
        emb_in = emb
        emb = emb.contiguous()
        n, h = emb.shape
        dev = emb.device
        na, nn_ = hs["n_abn"], hs["n_nrm"]
        noise = noise.reshape(na, h).contiguous() if noise is not None else None
        emb_abn = torch.empty(na, h, dtype=torch.float32, device=dev)
        comb = torch.empty(nn_ + na, h, dtype=torch.float32, device=dev)
        lean = _HEAD_LEAN and emb_in.is_contiguous()
        if lean:
            # round 6: both row gathers from emb in one launch; emb_con is written by its product straight into the tail of emb_combine
            call("ggad_head_rows_f32", ptr(emb), ptr(hs["abn"]), ptr(noise), na, ptr(hs["nrm"]), nn_, h, ptr(emb_abn), ptr(comb))
            con_pre = spmm(adj.A, emb, plan=hs["rows_plan"])
            emb_con = gemm(con_pre, w4, False, True, relu=True, out=comb[nn_:])
        else:
            call("ggad_head_gather_f32", ptr(emb), ptr(hs["abn"]), ptr(noise), na, h, ptr(emb_abn))
            con_pre = spmm(adj.A, emb, plan=hs["rows_plan"])
            emb_con = gemm(con_pre, w4, False, True, relu=True)
            call("ggad_head_combine_f32", ptr(emb), ptr(hs["nrm"]), nn_, ptr(emb_con), na, h, ptr(comb))
        if mlp_score_supported(w1, w2, w3):
            f1, f2, f3 = mlp_score_fwd(comb, w1, w2, w3)                   # one launch (csrc/mlp.hip)
        else:
            f1 = gemm(comb, w1, False, True, relu=True)
            f2 = gemm(f1, w2, False, True, relu=True)
            f3 = gemm(f2, w3, False, True)
        if lean:
            # emb[:, abn, :] = emb_con in place, as the reference writes it (model.py:182): A rows instead of a second N x H tensor.  Every
            # read of the old rows (emb[abn] + noise, A_hat[abn, :] emb, emb[normal]) is behind us; GcnLayerFn keeps z, not its output
            call("ggad_head_emb_put_f32", ptr(emb_con), ptr(hs["abn"]), na, h, ptr(emb))
            ctx.mark_dirty(emb_in)
            emb_out = emb_in
        else:
            emb_out = torch.empty_like(emb)
            call("ggad_head_emb_out_f32", ptr(emb), ptr(hs["abn_pos"]), ptr(emb_con), n, h, ptr(emb_out))
        ctx.save_for_backward(con_pre, emb_con, comb, f1, f2, w4, w1, w2, w3)
        ctx.hs, ctx.shape = hs, (n, h)
        ctx.set_materialize_grads(False)
        return emb_out, comb, f3, emb_con, emb_abn

    @staticmethod
    def backward(ctx, g_out, g_comb, g_f3, g_con, g_abn):
        con_pre, emb_con, comb, f1, f2, w4, w1, w2, w3 = ctx.saved_tensors
        hs = ctx.hs
        n, h = ctx.shape
        na, nn_ = hs["n_abn"], hs["n_nrm"]
        dev = emb_con.device
        c = lambda t: t.contiguous() if t is not None else None          # noqa: E731
        g_out, g_comb, g_f3, g_con, g_abn = c(g_out), c(g_comb), c(g_f3), c(g_con), c(g_abn)
        dw1 = dw2 = dw3 = None
        d_comb = g_comb
        if g_f3 is not None and mlp_score_supported(w1, w2, w3):           # scorer MLP: data gradients in one launch (+ g_comb)
            dz2, dz1, d_comb = mlp_score_dgrad(g_f3, f1, f2, w1, w2, w3, g_comb)
            if os.environ.get("GGAD_MLP_WGRAD_FUSED", "1") != "0" and comb.stride(1) == 1:
                dw1, dw2, dw3 = mlp_score_wgrad(comb, dz1, f1, dz2, f2, g_f3)       # the three weight gradients: one launch + one reduction
            else:
                dw3 = gemm(g_f3.reshape(-1, 1), f2, True, False)
                dw2 = gemm(dz2, f1, True, False)
                dw1 = gemm(dz1, comb, True, False)
        elif g_f3 is not None:                                             # ... or as LinearFn.backward three times
            dw3 = gemm(g_f3, f2, True, False)
            df2 = gemm(g_f3, w3, False, False)
            dz2 = torch.empty_like(df2)
            call("ggad_relu_bwd_f32", ptr(df2), ptr(f2), df2.numel(), ptr(dz2))
            dw2 = gemm(dz2, f1, True, False)
            df1 = gemm(dz2, w2, False, False)
            dz1 = torch.empty_like(df1)
            call("ggad_relu_bwd_f32", ptr(df1), ptr(f1), df1.numel(), ptr(dz1))
            dw1 = gemm(dz1, comb, True, False)
            d_comb = gemm(dz1, w1, False, False)
            if g_comb is not None:
                d_comb = d_comb + g_comb
        dz4 = torch.empty(na, h, dtype=torch.float32, device=dev)
        tail = d_comb[nn_:] if d_comb is not None else None              # rows of emb_combine that are emb_con (contiguous slice)
        call("ggad_head_con_grad_f32", ptr(g_con), ptr(g_out), ptr(hs["abn"]), ptr(tail), ptr(emb_con), na, h, ptr(dz4))
        dw4 = gemm(dz4, con_pre, True, False)
        g_emb = None
        if ctx.needs_input_grad[0]:
            d_pre = gemm(dz4, w4, False, False)
            sp = spmm(hs["sub_t"], d_pre)
            g_emb = torch.empty(n, h, dtype=torch.float32, device=dev)
            call("ggad_head_emb_grad_f32", ptr(g_out), ptr(hs["abn_pos"]), ptr(hs["nrm_pos"]), ptr(d_comb), ptr(g_abn), ptr(sp), n, h,
                 ptr(g_emb))
        return g_emb, None, dw4, dw1, dw2, dw3, None, None


# GGAD_LOSS_FUSED=0: the round-5 launch sequence of the loss block (A/B measurements; the tests run both)
_LOSS_FUSED = os.environ.get("GGAD_LOSS_FUSED", "1") != "0"


class GgadLossFn(torch.autograd.Function):
    """(total, margin, bce, rec) of `run.py:165-210`; only `total` is differentiable."""

    @staticmethod
    def forward(ctx, emb, logits, emb_con, emb_abn, adj: FullGraphAdj, ls, margin: float):
        ctx.set_materialize_grads(False)       # only `total` is differentiated: no zero tensors for the three other outputs
        emb = emb.contiguous()
        n, h = emb.shape
        dev = emb.device
        inv = torch.empty(n, dtype=torch.float32, device=dev)
        en = torch.empty_like(emb)
        call("ggad_rownorm_f32", ptr(emb), n, h, ptr(inv), ptr(en))                       # run.py:177-180
        J, L = ls["J"], int(ls["J"].numel())
        s_j = spmm(adj.Rt, en, plan=ls["Rt_plan"])                                        # (R^T e_hat)[J]
        aff = torch.empty(L, dtype=torch.float32, device=dev)
        losses = torch.empty(4, dtype=torch.float32, device=dev)
        d_logits = torch.empty(L, dtype=torch.float32, device=dev)
        g_aff = torch.empty(L, dtype=torch.float32, device=dev)
        emb_con, emb_abn, logits = emb_con.contiguous(), emb_abn.contiguous(), logits.contiguous()
        fused = _LOSS_FUSED and ls.get("seg_unique", False) and h <= 1024
        ctx.fused = fused
        if fused:
            # round 6: row dots, recon partials and -- in the last workgroup to finish -- BCE / margin / recon / coefficients: ONE launch
            ws = ls.get("loss_ws_fused")
            if ws is None:
                ws = ls["loss_ws_fused"] = (torch.empty(int(_lib.load().ggad_full_loss_fused_workspace_elems(ls["n_out"], h)),
                                                        dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
            kcol = torch.empty(h, dtype=torch.float32, device=dev)
            call("ggad_full_loss_fused_f32", ptr(en), ptr(J), ptr(s_j), ptr(ls["r_inv_J"]), ls["n_normal"], ls["n_out"], h, ptr(logits),
                 ptr(emb_con), ptr(emb_abn), float(margin), ptr(aff), ptr(kcol), ptr(losses), ptr(d_logits), ptr(g_aff), ptr(ws[0]), ptr(ws[1]))
            ctx.save_for_backward(en, inv, s_j, g_aff, d_logits, kcol, emb_con, emb_abn)
        else:
            call("ggad_rowdot_f32", ptr(en), ptr(J), ptr(s_j), L, h, ptr(ls["r_inv_J"]), ptr(aff))   # run.py:182-188
            dD = torch.empty_like(emb_con)
            ws = ls.get("loss_ws")
            if ws is None:
                ws = ls["loss_ws"] = torch.empty(int(_lib.load().ggad_full_loss_workspace_elems(ls["n_out"], h)), dtype=torch.float32,
                                                 device=dev)
            call("ggad_full_loss_f32", ptr(logits), ptr(aff), ls["n_normal"], ls["n_out"], ptr(emb_con), ptr(emb_abn), h,
                 float(margin), ptr(losses), ptr(d_logits), ptr(g_aff), ptr(dD), ptr(ws))
            ctx.save_for_backward(en, inv, s_j, g_aff, d_logits, dD)
        ctx.adj, ctx.ls = adj, ls
        ctx.affinity = aff
        return losses[0], losses[1], losses[2], losses[3]

    @staticmethod
    def backward(ctx, g_total, g_margin, g_bce, g_rec):
        adj, ls = ctx.adj, ctx.ls
        J, L, nn_ = ls["J"], int(ls["J"].numel()), ls["n_normal"]
        if g_total is None:
            return None, None, None, None, None, None, None
        if g_total.dtype != torch.float32:
            g_total = g_total.to(torch.float32)
        g_total = g_total.reshape(1)
        if ctx.fused:
            en, inv, s_j, g_aff, d_logits, kcol, emb_con, emb_abn = ctx.saved_tensors
            n, h = en.shape
            c, dl = torch.empty_like(g_aff), torch.empty_like(d_logits)                   # c = d total / d (e_hat_j . S_j)
            d_con, d_abn = torch.empty_like(emb_con), torch.empty_like(emb_con)
            xc = torch.empty(L, h, dtype=torch.float32, device=en.device)                 # c_j e_hat_j
            call("ggad_full_loss_bwd_fused_f32", ptr(g_total), ptr(g_aff), ptr(ls["r_inv_J"]), ptr(d_logits), ptr(en), ptr(J), L, h,
                 ptr(emb_con), ptr(emb_abn), ptr(kcol), ls["n_out"], ptr(c), ptr(dl), ptr(xc), ptr(d_con), ptr(d_abn))
            den = spmm(ls["RJ"], xc)                                                      # sum_j R_ij c_j e_hat_j
            d_emb = torch.empty_like(en)
            call("ggad_rownorm_bwd_add_f32", ptr(en), ptr(inv), ptr(den), ptr(ls["pos_n"]), ptr(ls["pos_a"]), ptr(c), ptr(s_j), n, h,
                 ptr(d_emb))                                                              # + c_j S_j on the rows J, then the normalisation's VJP
            return d_emb, dl, d_con, d_abn, None, None, None
        en, inv, s_j, g_aff, d_logits, dD = ctx.saved_tensors
        n, h = en.shape
        c, dl = torch.empty_like(g_aff), torch.empty_like(d_logits)                       # c = d total / d (e_hat_j . S_j)
        d_con, d_abn = torch.empty_like(dD), torch.empty_like(dD)
        g_total = g_total.contiguous()
        call("ggad_full_loss_bwd_scale_f32", ptr(g_total), ptr(g_aff), ptr(ls["r_inv_J"]), ptr(d_logits), ptr(dD), L, dD.numel(),
             ptr(c), ptr(dl), ptr(d_con), ptr(d_abn))
        xc = torch.empty(L, h, dtype=torch.float32, device=en.device)
        call("ggad_rows_scale_f32", ptr(en), ptr(J), ptr(c), L, h, 0, ptr(xc))            # c_j e_hat_j
        den = spmm(ls["RJ"], xc)                                                          # sum_j R_ij c_j e_hat_j
        # + c_j S_j on rows J
        if ls.get("distinct"):                                                            # no node in both lists (run.py's draws): one launch
            call("ggad_rows_scale_f32", ptr(s_j), ptr(J), ptr(c), L, h, 1, ptr(den))
        elif ls.get("rounds") is not None:                                                # a node twice inside a list: round by round
            for pos, rows in ls["rounds"]:
                k = int(pos.numel())
                c_k = torch.empty(k, dtype=torch.float32, device=en.device)
                s_k = torch.empty(k, h, dtype=torch.float32, device=en.device)
                call("ggad_rows_scale_f32", ptr(c), ptr(pos), 0, k, 1, 0, ptr(c_k))      # c[pos], S[pos]: gathers (coefficient 1)
                call("ggad_rows_scale_f32", ptr(s_j), ptr(pos), 0, k, h, 0, ptr(s_k))
                call("ggad_rows_scale_f32", ptr(s_k), ptr(rows), ptr(c_k), k, h, 1, ptr(den))
        else:                                                                             # normal and abnormal segments are each duplicate-free
            call("ggad_rows_scale_f32", ptr(s_j), ptr(J), ptr(c), nn_, h, 1, ptr(den))
            call("ggad_rows_scale_f32", s_j.data_ptr() + 4 * nn_ * h, J.data_ptr() + 4 * nn_, c.data_ptr() + 4 * nn_, L - nn_, h, 1,
                 ptr(den))
        d_emb = torch.empty_like(en)
        call("ggad_rownorm_bwd_f32", ptr(en), ptr(inv), ptr(den), n, h, ptr(d_emb))
        return d_emb, dl, d_con, d_abn, None, None, None


def ggad_loss(emb, logits, emb_con, emb_abnormal, adj: FullGraphAdj, ls, margin: float):
    """`GgadLossFn` on what `Model.forward` returns ((1, N, H), (1, L, 1), (A, H), (1, A, H)): the 2-D views are reshapes, whose
    backward is a view again -- `emb[0]` / `logits[0, :, 0]` cost a zero-fill and a copy of the whole tensor each in autograd."""
    h = emb.shape[-1]
    return GgadLossFn.apply(emb.reshape(-1, h), logits.reshape(-1), emb_con, emb_abnormal.reshape(-1, h), adj, ls, margin)


_ADAM_TICKETS = os.environ.get("GGAD_ADAM_TICKETS", "1") != "0"      # 0: the trailing k_bump_multi launch of round 5 (A/B)


class FlatAdam:
    """torch.optim.Adam semantics (lr, weight_decay, betas .9/.999, eps 1e-8) executed by the HIP Adam kernel on
    the parameters that received a gradient (params with ``grad is None`` are skipped, as torch does)."""

    def __init__(self, params: Sequence[torch.nn.Parameter], lr: float, weight_decay: float = 0.0):
        self.params = [p for p in params]
        self.lr, self.wd = float(lr), float(weight_decay)
        self.state = {}

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def step(self):
        """One multi-tensor launch per <= 16 parameters with a gradient (the step counters advance inside it)."""
        import ctypes
        todo = []
        for p in self.params:
            if p.grad is None:
                continue
            st = self.state.get(p)
            if st is None:
                st = self.state[p] = (torch.zeros_like(p.data), torch.zeros_like(p.data),
                                      torch.zeros(1, dtype=torch.int32, device=p.device))
            todo.append((p, st, p.grad.contiguous()))
        cap = int(_lib.load().ggad_adam_multi_max())
        if todo and getattr(self, "_tickets", None) is None:
            # one zeroed ticket word per tensor slot and launch group: the last workgroup of a tensor advances its step counter (round 6:
            # no trailing launch); allocated once, outside any capture (the first steps of every caller are eager)
            self._tickets = torch.zeros((len(self.params) + cap - 1) // cap * cap, dtype=torch.int32, device=todo[0][0].device)
        for i0 in range(0, len(todo), cap):
            part = todo[i0:i0 + cap]
            n = len(part)
            arr = ctypes.c_void_p * n
            call("ggad_adam_multi_f32", n, arr(*[ptr(p.data) for p, _, _ in part]), arr(*[ptr(st[0]) for _, st, _ in part]),
                 arr(*[ptr(st[1]) for _, st, _ in part]), arr(*[ptr(g) for _, _, g in part]),
                 (ctypes.c_int64 * n)(*[p.numel() for p, _, _ in part]), arr(*[ptr(st[2]) for _, st, _ in part]), self.lr, self.wd,
                 self._tickets.data_ptr() + 4 * i0 if _ADAM_TICKETS else 0)
