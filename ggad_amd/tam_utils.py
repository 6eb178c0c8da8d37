"""Host / device helpers of the full-graph TAM comparison model (`tam.py`, `utils_tam.py` of the reference) on CSR matrices.

The reference holds the adjacency, the distance table and every truncated graph as dense N x N tensors and walks them row by
row in Python; here they are CSR and HIP kernels do everything per epoch.  The once-per-cut truncation has two paths that give
the same graphs, bit for bit, and leave numpy's stream at the same position: scipy on the host (`graph_nsgt` +
`normalize_adj_tensor`, the default) and `DeviceNsgt` (csrc/tam_nsgt.hip, `tam.py --device_cut`), which keeps the current graph
as a byte mask over the entries of A + I and leaves only three small rounding-sensitive quantities to the host (the fp32 mean
of the live distances, the per-row thresholds with their random draws, colsum^-1/2):

    load_mat / split_nodes            `utils_tam.py:140-179`   (python `random` driven split, incl. its index quirk)
    calc_distance                     `utils_tam.py:190-199`   -> `ggad_edge_dist_f32`, one value per stored entry of A + I
    graph_nsgt                        `utils_tam.py:222-240`   -> vectorised over rows, same draws from numpy's stream
    normalize_adj_tensor              `utils_tam.py:45-53`
    DeviceNsgt                        both of the above        -> `ggad_tam_nsgt_*` (opt-in; thresholds from `nsgt_thresholds` too)
    max_message / inference           `tam.py:113-146`         -> `AffinityFn` (HIP row-normalise, CSR SpMM, row dots)
                                                               -> opt-in: `TamHeadFn` / `max_message_fused` (csrc/tam.hip)
"""
from __future__ import annotations

import random as _pyrandom
from typing import List, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr
from .fullgraph import FullGraphAdj, spmm
from .fullgraph_script import capture


def split_nodes(ano_labels: np.ndarray, rng=_pyrandom) -> Tuple[List[int], np.ndarray]:
    """(normal_label_idx, idx_test) of `load_mat` (`utils_tam.py:163-179`): 30 / 10 / 60 % split of a shuffled index list, 80 %
    of the normal training nodes, plus int(0.15 * #anomalies) nodes taken from the SHUFFLED list at the positions of the
    anomalies (`:172` -- the reference's "contamination" are therefore random nodes; kept)."""
    ano_labels = np.asarray(ano_labels)
    n = len(ano_labels)
    all_idx = list(range(n))
    rng.shuffle(all_idx)
    n_train, n_val = int(n * 0.3), int(n * 0.1)
    idx_train, idx_test = all_idx[:n_train], all_idx[n_train + n_val:]
    all_normal = [i for i in idx_train if ano_labels[i] == 0]
    normal = all_normal[: int(len(all_normal) * 0.8)]
    real_abnormal = np.array(all_idx)[np.argwhere(ano_labels == 1).squeeze()].tolist()
    add_rate = 0.15 * len(real_abnormal)
    rng.shuffle(real_abnormal)
    add = real_abnormal[:int(add_rate)]
    return normal + add, np.setdiff1d(idx_test, add, False)


def load_mat(dataset: str, root: str = "./data"):
    """`load_mat` of `utils_tam.py:140-179`: (adj, feat, ano_labels, str_ano_labels, attr_ano_labels, normal_label_idx, idx_test)."""
    import scipy.io as sio
    import scipy.sparse as sp
    data = sio.loadmat("{}/{}.mat".format(root, dataset))
    label = data["Label"] if ("Label" in data) else data["gnd"]
    attr = data["Attributes"] if ("Attributes" in data) else data["X"]
    network = data["Network"] if ("Network" in data) else data["A"]
    adj, feat = sp.csr_matrix(network), sp.lil_matrix(attr)
    ano = np.squeeze(np.array(label))
    str_l = np.squeeze(np.array(data["str_anomaly_label"])) if "str_anomaly_label" in data else None
    attr_l = np.squeeze(np.array(data["attr_anomaly_label"])) if "str_anomaly_label" in data else None
    normal, idx_test = split_nodes(ano)
    return adj, feat, ano, str_l, attr_l, normal, idx_test


def calc_distance(raw, feats: torch.Tensor) -> np.ndarray:
    """Attribute distance of every stored entry of `raw` (scipy CSR of A + I, sorted indices), aligned with `raw.indices`.
    The reference's N x N `dis_array` holds exactly these values at the non-zero positions of raw_adj and 0 elsewhere."""
    return calc_distance_dev(raw, feats).cpu().numpy()


def calc_distance_dev(raw, feats: torch.Tensor) -> torch.Tensor:
    """`calc_distance` with the values left on the device (what `DeviceNsgt` reads)."""
    dev = feats.device
    x = feats.reshape(-1, feats.shape[-1]).contiguous().float()
    rp = torch.from_numpy(raw.indptr.astype(np.int32)).to(dev)
    ci = torch.from_numpy(raw.indices.astype(np.int32)).to(dev)
    out = torch.empty(raw.nnz, dtype=torch.float32, device=dev)
    call("ggad_edge_dist_f32", ptr(rp), ptr(ci), ptr(x), raw.shape[0], x.shape[1], ptr(out))
    return out


def nsgt_thresholds(mx: np.ndarray, cnt: np.ndarray, mean_dis, nprandom=np.random) -> np.ndarray:
    """The cut threshold of every row (`utils_tam.py:228-236`), shared by `graph_nsgt` and `DeviceNsgt.step` so that the two cannot
    drift apart.  `mx[i]` / `cnt[i]`: the largest distance and the number of the current entries of row i (mx of an empty row is not
    read); `mean_dis`: the fp32 mean of the current non-zero distances.  A row with entries whose largest distance exceeds the mean
    takes ONE number from numpy's global stream, in row order, and gets mean + u (max - mean) in fp32; every other row gets +inf
    (nothing is farther than that: the row keeps all its entries)."""
    n = len(cnt)
    rows = np.nonzero(np.asarray(cnt) > 0)[0]
    mxr = np.asarray(mx, dtype=np.float32)[rows]
    qual = mxr > mean_dis
    u = nprandom.random_sample(int(qual.sum()))                  # one draw per qualifying row, in row order
    thr = np.full(n, np.inf, dtype=np.float32)
    mean32 = np.float32(mean_dis)
    thr[rows[qual]] = (mxr[qual] - mean32).astype(np.float32) * u.astype(np.float32) + mean32
    return thr


def _nsgt_mean(nz: np.ndarray):
    """fp32 mean of the non-zero distances in torch's summation order (the reference's `torch.mean`); nan without any."""
    return torch.from_numpy(nz).mean().numpy() if len(nz) else np.float32("nan")


def graph_nsgt(raw, dis_vals: np.ndarray, adj, nprandom=np.random):
    """One truncation step (`graph_nsgt`, `utils_tam.py:222-240`).  `raw`: scipy CSR of the ORIGINAL A + I (sorted indices) with
    `dis_vals` = the distance of each of its entries (`calc_distance`); `adj`: scipy CSR pattern of the current graph (a subset
    of `raw`'s pattern).  Per row with at least one neighbour whose largest distance exceeds the mean non-zero distance over
    the current entries, ONE number is taken from numpy's global stream (in row order, like the reference's loop) and the
    row's entries farther than mean + u (max - mean) are cut; an entry survives if either direction survives (adj + adj.T).
    Returns the new CSR pattern (data = 1)."""
    import scipy.sparse as sp
    adj = sp.csr_matrix(adj)
    adj.sort_indices()
    n = adj.shape[0]
    deg = np.diff(adj.indptr)
    key_raw = np.repeat(np.arange(n, dtype=np.int64), np.diff(raw.indptr)) * n + raw.indices
    key_adj = np.repeat(np.arange(n, dtype=np.int64), deg) * n + adj.indices
    pos = np.searchsorted(key_raw, key_adj)
    if len(pos) and (pos.max() >= len(key_raw) or not np.array_equal(key_raw[pos], key_adj)):
        raise ValueError("graph_nsgt: the current graph has an entry the original one lacks")
    dis = np.asarray(dis_vals, dtype=np.float32)[pos]
    mean_dis = _nsgt_mean(dis[dis != 0])
    rows = np.nonzero(deg > 0)[0]
    mx = np.zeros(n, dtype=np.float32)
    if len(rows):
        mx[rows] = np.maximum.reduceat(dis, adj.indptr[rows])
    thr = nsgt_thresholds(mx, deg, mean_dis, nprandom)
    keep = ~(dis > np.repeat(thr, deg))
    cut = sp.csr_matrix((keep.astype(np.float32), adj.indices.copy(), adj.indptr.copy()), shape=adj.shape)
    cut.eliminate_zeros()                                        # (in place: hence the copies above)
    sym = (cut + cut.T).tocsr()
    sym.data[:] = 1.0
    sym.sort_indices()
    return sym


def normalize_adj_tensor(adj):
    """`normalize_adj_tensor` (`utils_tam.py:45-53`) on a scipy CSR 0/1 matrix: entries r_i r_j with r = colsum^-1/2 (inf -> 0),
    evaluated in fp32 like the reference's dense tensors."""
    import scipy.sparse as sp
    adj = sp.csr_matrix(adj, dtype=np.float32)
    colsum = torch.from_numpy(np.asarray(adj.sum(0)).reshape(-1).astype(np.float32))
    r = torch.pow(colsum, -0.5)
    r[torch.isinf(r)] = 0.0
    r = r.numpy()
    rows = np.repeat(np.arange(adj.shape[0]), np.diff(adj.indptr))
    vals = (r[rows] * (adj.data * r[adj.indices]).astype(np.float32)).astype(np.float32)
    return sp.csr_matrix((vals, adj.indices.copy(), adj.indptr.copy()), shape=adj.shape)


class _NsgtStatic:
    """What every tree of a run shares: the CSR of raw = A + I with its distances and transpose map on the device, the scratch of a
    step (steps run one after the other on one stream) and the pinned staging buffer of the distances."""

    def __init__(self, raw, dis_vals, device):
        import scipy.sparse as sp
        dev = torch.device(device)
        raw = sp.csr_matrix(raw)
        if raw.shape[0] != raw.shape[1]:
            raise ValueError("DeviceNsgt needs a square adjacency")
        if not raw.has_canonical_format:
            raw = raw.copy()
            raw.sum_duplicates()
            raw.sort_indices()
        if raw.nnz >= 2 ** 31:
            raise ValueError("matrix too large for int32 CSR")
        n, nnz = int(raw.shape[0]), int(raw.nnz)
        self.dev, self.n, self.nnz = dev, n, nnz
        self.indptr, self.indices = raw.indptr.astype(np.int64), raw.indices.astype(np.int32)
        self.rowptr = torch.from_numpy(raw.indptr.astype(np.int32)).to(dev)
        self.col = torch.from_numpy(self.indices).to(dev)
        if isinstance(dis_vals, torch.Tensor):
            self.dis = dis_vals.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        else:
            self.dis = torch.from_numpy(np.ascontiguousarray(dis_vals, dtype=np.float32).reshape(-1)).to(dev)
        if self.dis.numel() != nnz:
            raise ValueError("DeviceNsgt: one distance per stored entry of raw is needed")
        self.tpos = torch.empty(max(1, nnz), dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        call("ggad_tam_nsgt_transpose_map", ptr(self.rowptr), ptr(self.col), n, ptr(self.tpos), ptr(status))
        if int(status.item()) != 0:
            raise ValueError("DeviceNsgt needs a raw adjacency with a symmetric pattern (the reference's adj + adj.T would leave the "
                             "pattern of A + I otherwise); use the host path (`graph_nsgt` / `normalize_adj_tensor`) for this graph")
        self.keep = torch.empty(max(1, nnz), dtype=torch.uint8, device=dev)
        self.nz = torch.empty(max(1, nnz), dtype=torch.float32, device=dev)          # the live non-zero distances, CSR order
        self.nz_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        self.scan_ws = torch.empty(max(1, int(_lib.load().ggad_scan_workspace_elems(n))), dtype=torch.int32, device=dev)
        self.stat_mx = torch.empty(max(1, n), dtype=torch.float32, device=dev)
        self.thr = torch.empty(max(1, n), dtype=torch.float32, device=dev)
        self.r = torch.empty(max(1, n), dtype=torch.float32, device=dev)
        self.stage = torch.empty(max(1, nnz), dtype=torch.float32, pin_memory=True)
        self.stage_np = self.stage.numpy()

    def rowstat(self, alive, stat_i):
        """(cnt, mx, nzcnt) of the rows of the graph `alive` on the host; the two counts stay in `stat_i` (2 x n int32) on the device."""
        call("ggad_tam_nsgt_rowstat", ptr(self.rowptr), ptr(self.dis), ptr(alive), self.n, ptr(stat_i[0]), ptr(self.stat_mx),
             ptr(stat_i[1]))
        si = stat_i.cpu().numpy()
        return si[0, :self.n].copy(), self.stat_mx.cpu().numpy()[:self.n], si[1, :self.n].copy()


class DeviceNsgt:
    """`graph_nsgt` + `normalize_adj_tensor` of one tree on the device (csrc/tam_nsgt.hip).  `raw`: scipy CSR of A + I with a SYMMETRIC
    pattern (ValueError otherwise); `dis_vals`: the distance of each of its entries (`calc_distance`, or `calc_distance_dev`'s tensor).
    The current graph is a byte per entry of raw; a `step` is a few streaming passes over them and gives exactly what the host path
    gives: the same pattern, the same bits in every normalised value, numpy's stream at the same position.  Three quantities are
    rounding-sensitive and therefore come from the host calls `graph_nsgt` / `normalize_adj_tensor` make: the fp32 mean of the live
    non-zero distances (torch's summation order over the vector the device compacts), the thresholds (`nsgt_thresholds`, O(n)) and
    r = colsum^-1/2 (`torch.pow` on the n live row counts -- the column sums, the pattern being symmetric)."""

    def __init__(self, raw, dis_vals, device, _static=None):
        s = self._s = _static if _static is not None else _NsgtStatic(raw, dis_vals, device)
        self.alive = torch.ones(max(1, s.nnz), dtype=torch.uint8, device=s.dev)
        if _static is None:                        # per row: live entries / live non-zero distances (device), + the maximum (host)
            self._stat_i = torch.empty((2, max(1, s.n)), dtype=torch.int32, device=s.dev)
            s.stat0 = s.rowstat(self.alive, self._stat_i)
            s.stat0_i = self._stat_i.clone()
        else:
            self._stat_i = s.stat0_i.clone()
        self._stat = s.stat0

    def fork(self) -> "DeviceNsgt":
        """Another tree over the same raw graph: shares the static part, owns a fresh all-alive mask."""
        return DeviceNsgt(None, None, None, _static=self._s)

    def step(self, nprandom=np.random):
        """One truncation round: advances the mask and returns (rowptr, col, val), device tensors of the truncated, normalised graph
        (canonical CSR, int32 / int32 / fp32)."""
        s = self._s
        n, dev = s.n, s.dev
        cnt, mx, nzc = self._stat
        args = (ptr(s.rowptr), ptr(s.col), ptr(s.dis), ptr(self.alive), n)
        tot = int(nzc.sum())
        call("ggad_tam_nsgt_compact", *args, 0, ptr(self._stat_i[1]), None, ptr(s.nz_ptr), None, ptr(s.nz), ptr(s.scan_ws))
        s.stage[:tot].copy_(s.nz[:tot], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        mean_dis = _nsgt_mean(s.stage_np[:tot])
        s.thr[:n].copy_(torch.from_numpy(nsgt_thresholds(mx, cnt, mean_dis, nprandom)))
        call("ggad_tam_nsgt_cut", ptr(s.rowptr), ptr(s.dis), ptr(s.tpos), ptr(s.thr), n, s.nnz, ptr(self.alive), ptr(s.keep))
        cnt, mx, nzc = self._stat = s.rowstat(self.alive, self._stat_i)
        r = torch.pow(torch.from_numpy(cnt.astype(np.float32)), -0.5)      # colsum = live row count: the pattern is symmetric
        r[torch.isinf(r)] = 0.0
        s.r[:n].copy_(r)
        total = int(cnt.sum())
        rowptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        col = torch.empty(total, dtype=torch.int32, device=dev)
        val = torch.empty(total, dtype=torch.float32, device=dev)
        call("ggad_tam_nsgt_compact", *args, 1, ptr(self._stat_i[0]), ptr(s.r), ptr(rowptr), ptr(col), ptr(val), ptr(s.scan_ws))
        return rowptr, col, val

    def pattern(self):
        """The current graph as a host scipy CSR (data = 1), like `graph_nsgt` returns it."""
        import scipy.sparse as sp
        s = self._s
        live = self.alive[:s.nnz].cpu().numpy().astype(bool)
        rows = np.repeat(np.arange(s.n, dtype=np.int64), np.diff(s.indptr))[live]
        indptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=s.n)))).astype(np.int32)
        m = sp.csr_matrix((np.ones(int(live.sum()), np.float32), s.indices[live], indptr), shape=(s.n, s.n))
        m.has_sorted_indices = True
        return m


class AffinityFn(torch.autograd.Function):
    """message_i = r_inv_i <e_hat_i, (R e_hat)_i> for every node: the row sums of (e_hat e_hat^T) * raw_adj divided by the column
    sums of raw_adj (`tam.py:113-127`), without the N x N product.  `adj.Rt` is used as R: TAM's raw adjacency is symmetric
    (`FullGraphAdj` built from A + I).  Rows of zero norm give 0 (the reference's `max_message` zeroes their NaN products)."""

    @staticmethod
    def forward(ctx, emb, adj: FullGraphAdj):
        emb = emb.contiguous()
        n, h = emb.shape
        dev = emb.device
        inv = torch.empty(n, dtype=torch.float32, device=dev)
        en = torch.empty_like(emb)
        call("ggad_rownorm_f32", ptr(emb), n, h, ptr(inv), ptr(en))
        s = spmm(adj.Rt, en)
        r_inv = adj.r_inv_dev()
        aff = torch.empty(n, dtype=torch.float32, device=dev)
        call("ggad_rowdot_f32", ptr(en), None, ptr(s), n, h, ptr(r_inv), ptr(aff))
        ctx.save_for_backward(en, inv, s, r_inv)
        ctx.adj = adj
        return aff

    @staticmethod
    def backward(ctx, g):
        en, inv, s, r_inv = ctx.saved_tensors
        adj = ctx.adj
        n, h = en.shape
        c = (g * r_inv).contiguous()                                     # d loss / d <e_hat_i, S_i>
        ar = adj.arange_dev()
        xc = torch.empty_like(en)
        call("ggad_rows_scale_f32", ptr(en), ptr(ar), ptr(c), n, h, 0, ptr(xc))          # c_i e_hat_i
        den = spmm(adj.Rt, xc)                                           # R^T (c . e_hat)  (R symmetric)
        call("ggad_rows_scale_f32", ptr(s), ptr(ar), ptr(c), n, h, 1, ptr(den))           # + c_i S_i
        d_emb = torch.empty_like(en)
        call("ggad_rownorm_bwd_f32", ptr(en), ptr(inv), ptr(den), n, h, ptr(d_emb))
        return d_emb, None


def inference(emb: torch.Tensor, adj: FullGraphAdj) -> torch.Tensor:
    """`inference` (`tam.py:136-146`): the affinity of every node."""
    return AffinityFn.apply(emb.reshape(-1, emb.shape[-1]), adj)


def max_message(emb: torch.Tensor, adj: FullGraphAdj, normal_label_idx) -> Tuple[torch.Tensor, torch.Tensor]:
    """`max_message` (`tam.py:113-133`): (- sum of the min-max normalised affinity over the labelled normal nodes, that vector)."""
    m = AffinityFn.apply(emb.reshape(-1, emb.shape[-1]), adj)
    m = (m - torch.min(m)) / (torch.max(m) - torch.min(m))
    idx = normal_label_idx if isinstance(normal_label_idx, torch.Tensor) else torch.as_tensor(
        np.asarray(normal_label_idx, dtype=np.int64), device=m.device)
    return -torch.sum(m.index_select(0, idx.reshape(-1).long())), m


class TamHead:
    """What the fused head (csrc/tam.hip) needs besides the embedding, built ONCE per (adj, normal_label_idx), outside any capture:
    cnt (occurrences of every node in the index list -- `split_nodes` can list a node twice), K = len(list), the hub list of R and
    the zeroed workspace.  The backward of the kernels gathers with R where the composed path multiplies by R^T, so R must be
    symmetric in pattern and values: checked here on the host; an asymmetric R raises ValueError."""

    def __init__(self, adj: FullGraphAdj, normal_label_idx):
        R = adj.Rt
        host = R.host
        if host.shape[0] != host.shape[1] or abs(host - host.T).nnz != 0:
            raise ValueError("the fused TAM head needs a symmetric raw adjacency (pattern and values); use the composed path "
                             "(`max_message` / `train_cut(..., fused=False)`) for this graph")
        lib = _lib.load()
        dev = adj.dev
        n = int(host.shape[0])
        idx = normal_label_idx.detach().cpu().numpy() if isinstance(normal_label_idx, torch.Tensor) else np.asarray(normal_label_idx)
        idx = idx.reshape(-1).astype(np.int64)
        if len(idx) and (idx.min() < 0 or idx.max() >= n):
            raise IndexError("normal_label_idx holds a node outside the graph")
        self.adj, self.n = adj, n
        self.k_total = float(len(idx))
        self.cnt = torch.from_numpy(np.bincount(idx, minlength=n).astype(np.float32)).to(dev)
        hub_len = int(lib.ggad_tam_head_hub_len())
        deg = np.diff(host.indptr)
        hubs = np.nonzero(deg > hub_len)[0]
        pp = np.concatenate(([0], np.cumsum(-(-deg[hubs] // hub_len)))).astype(np.int32)
        self.n_hub, self.n_pieces = int(len(hubs)), int(pp[-1])
        self.hub_rows = torch.from_numpy(hubs.astype(np.int32)).to(dev) if self.n_hub else None
        self.hub_pp = torch.from_numpy(pp).to(dev) if self.n_hub else None
        self.r_inv = adj.r_inv_dev()
        self._ws = {}

    def workspace(self, h: int) -> torch.Tensor:
        """The zeroed workspace for width h (created on first use: in an eager epoch, before any capture)."""
        w = self._ws.get(h)
        if w is None:
            elems = int(_lib.load().ggad_tam_head_workspace_elems(self.n, h, self.n_hub, self.n_pieces))
            w = self._ws[h] = torch.zeros(max(1, elems), dtype=torch.float32, device=self.adj.dev)
        return w

    def _args(self, emb):
        R = self.adj.Rt
        n, h = emb.shape
        return (ptr(R.rowptr), ptr(R.col), ptr(R.val), ptr(emb), ptr(self.r_inv), ptr(self.cnt), self.k_total, n, h,
                ptr(self.hub_rows), ptr(self.hub_pp), self.n_hub, self.n_pieces)


class TamHeadFn(torch.autograd.Function):
    """(loss, m, a) of the fused head: a = the raw affinity (`inference`), m its min-max normalisation, loss = -sum of m over the index
    list.  Only the loss carries a gradient (to emb).  `want_m=False` skips the launch that writes m (m is then None)."""

    @staticmethod
    def forward(ctx, emb, head: TamHead, want_m: bool):
        emb = emb.contiguous()
        n, h = emb.shape
        if n != head.n:
            raise ValueError("embedding rows != nodes of the head's graph")
        if not _lib.load().ggad_tam_head_supported(n, h):
            raise ValueError(f"the fused TAM head takes 1 <= h <= {int(_lib.load().ggad_tam_head_max_dim())}, not h = {h}")
        dev = emb.device
        a = torch.empty(n, dtype=torch.float32, device=dev)
        scal = torch.empty(8, dtype=torch.float32, device=dev)
        m = torch.empty(n, dtype=torch.float32, device=dev) if want_m else None
        inv = torch.empty(n, dtype=torch.float32, device=dev)
        call("ggad_tam_head_fwd_f32", *head._args(emb), ptr(a), ptr(scal), ptr(m), ptr(inv), ptr(head.workspace(h)))
        ctx.save_for_backward(emb, a, scal, inv)
        ctx.head = head
        loss = scal[0]
        if want_m:
            ctx.mark_non_differentiable(m, a)
            return loss, m, a
        ctx.mark_non_differentiable(a)
        return loss, None, a

    @staticmethod
    def backward(ctx, g, _gm, _ga):
        emb, a, scal, inv = ctx.saved_tensors
        head = ctx.head
        g = g.contiguous().float()
        d_emb = torch.empty_like(emb)
        call("ggad_tam_head_bwd_f32", *head._args(emb), ptr(a), ptr(scal), ptr(inv), ptr(g), ptr(d_emb),
             ptr(head.workspace(emb.shape[1])))
        return d_emb, None, None


def tam_head(adj: FullGraphAdj, normal_label_idx) -> TamHead:
    """The `TamHead` of (adj, normal_label_idx), cached on adj (keyed by the list's contents)."""
    idx = normal_label_idx.detach().cpu().numpy() if isinstance(normal_label_idx, torch.Tensor) else np.asarray(normal_label_idx)
    key = ("tam", idx.astype(np.int64).tobytes())
    head = adj._head.get(key)
    if head is None:
        head = adj._head[key] = TamHead(adj, idx)
    return head


def max_message_fused(emb: torch.Tensor, adj: FullGraphAdj, normal_label_idx, head: "TamHead" = None, want_m: bool = True):
    """`max_message` and `inference` in the fused kernels of csrc/tam.hip: (loss, m, a) with a = `inference(emb, adj)` and (loss, m)
    = `max_message(emb, adj, normal_label_idx)`.  `head`: a `TamHead` built beforehand (`train_cut` does; otherwise it is looked up
    on `adj`, which copies a device index list to the host).  R must be symmetric: ValueError otherwise."""
    if head is None:
        head = tam_head(adj, normal_label_idx)
    return TamHeadFn.apply(emb.reshape(-1, emb.shape[-1]), head, bool(want_m))


def normalize_score(ano_score: np.ndarray) -> np.ndarray:
    return (ano_score - np.min(ano_score)) / (np.max(ano_score) - np.min(ano_score))             # utils_tam.py:56-59


def train_cut(model, optimiser, features: torch.Tensor, adj: FullGraphAdj, normal_label_idx, num_epoch: int, use_graph: bool = True,
              log_every: int = 0, fused: bool = False, head: "TamHead" = None):
    """The epoch loop of one truncation round (`tam.py:186-201`): forward, `max_message` loss, `inference`, backward, Adam step.
    The reference calls `zero_grad()` ONCE per round (`:182`), so the gradients of a round accumulate from epoch to epoch;
    the caller does the same (this function never clears them).  After two eager epochs the epoch (forward, both affinity
    passes, backward into the accumulating gradients, fused Adam) is captured into one hipGraph and replayed.
    `fused=True`: the loss comes from `max_message_fused` and the round's message is that call's raw affinity; the second
    `inference` pass (which recomputes the same numbers from the same embedding) is not run.  `head`: with `fused`, a `TamHead` of
    (the raw adjacency of adj, normal_label_idx) built beforehand, used instead of a new one (it does not depend on the round's graph).
    Returns (losses [num_epoch] fp32 tensor on the device, message of the last epoch)."""
    dev = features.device
    idx = torch.as_tensor(np.asarray(normal_label_idx, dtype=np.int64), device=dev)
    losses = torch.zeros(max(1, int(num_epoch)), dtype=torch.float32, device=dev)
    state = {}
    if not fused:
        head = None
    elif head is None:
        head = TamHead(adj, normal_label_idx)

    def epoch():
        node_emb, feat1, feat2 = model.forward(features, adj)
        if fused:
            loss, _, state["message"] = max_message_fused(node_emb[0], adj, idx, head=head, want_m=False)
        else:
            loss, _ = max_message(node_emb[0], adj, idx)
            with torch.no_grad():
                state["message"] = inference(node_emb[0].detach(), adj)
        loss.backward()
        optimiser.step()
        return loss.detach()

    model.train()
    n_eager = min(int(num_epoch), 2 if use_graph else int(num_epoch))
    for e in range(n_eager):
        losses[e] = epoch()
        if log_every and e % log_every == 0:
            print("mean_loss is {}".format(losses[e].item()))
    left = int(num_epoch) - n_eager
    if left > 0:
        static_loss = torch.zeros((), dtype=torch.float32, device=dev)

        def captured_epoch():
            static_loss.copy_(epoch())
            return state["message"]

        graph, static_msg = capture(captured_epoch)
        # the capture does not execute: every remaining epoch is one replay
        for e in range(n_eager, int(num_epoch)):
            graph.replay()
            losses[e] = static_loss
            if log_every and e % log_every == 0:
                print("mean_loss is {}".format(losses[e].item()))
        state["message"] = static_msg
    return losses[:int(num_epoch)], state["message"]
