"""Why is this node in the ranked list?  The exact attribution of the mini-batch GGAD inference logit (config key `explain`).

The inference score has no bias and one ReLU (`k_score`, csrc/step.hip):

    a_i = W x1_i        z_i = sum_d w_d relu(a_i[d])        score_i = sigmoid(z_i)
    x1_i = sum_{j in N(i)+{i}} omega_ij feat[j]             omega_ij = (1 / sqrt(r_i)) / sqrt(c_j)

`r_i`: the size of the closed row; `c_j`: the rows, with multiplicity, of row i's slice of `batch_size` ids whose closed row holds j
(quirk 2, `oracle.aggregate_batch`).  With `g_i[f] = sum_d w_d [a_i[d] > 0] W[d, f]` the logit is linear where the ReLU pattern holds:

    z_i = sum_f g_i[f] x1_i[f]                    per feature
    z_i = sum_j omega_ij (g_i . feat[j])          per neighbour

Both sums are complete (they add up to the logit: no baseline, no sampling, no approximation) and exact ON THE CURRENT ReLU PATTERN:
they explain the logit the model computed, not what it would compute for another input (a counterfactual may switch units).  The
listed neighbours are the SIGNED greatest contributions: what pushed the score up.  `ggad_explain_f32` (csrc/explain.hip) computes both
from the CSR graph, the feature table, the scored id list and the engine's parameter block -- no plan, no cached row -- one workgroup
per explained position.  Model 'GCN' (GGAD) of the mini-batch program only: the full-graph model (PReLU, biases, two layers) has no
such identity and is not served.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib


@dataclass
class Explanation:
    """`explain`'s outputs for K positions, all on the device.  `pos` int32 (K,): the explained positions of the scored list; `logit`
    float32 (K,): z, `sigmoid(logit)` is the score; `feature` float32 (K, F): g[f] x1[f], each row sums to its logit; `closed_size`
    int32 (K,): |N(i) + {i}|; `nbr_id` int64 / `nbr_contrib` float32 / `nbr_colcount` int32 (K, m): the m greatest per-neighbour
    contributions (signed, equal values by ascending id) with their node ids and column counts c_j, padded with -1 / 0 / 0 where the
    closed row is shorter; `rest` float32 (K,): the sum of the contributions that are not listed, so that
    `nbr_contrib.sum(1) + rest` is the logit again.  `rows_workspace`: the rows longer than `ggad_explain_lds_rows()` (the hubs).
    `workspace` / `stride`: the kernel's workspace, which holds EVERY neighbour's contribution and count (`neighbours(k)`)."""
    pos: torch.Tensor
    logit: torch.Tensor
    feature: torch.Tensor
    closed_size: torch.Tensor
    nbr_id: torch.Tensor
    nbr_contrib: torch.Tensor
    nbr_colcount: torch.Tensor
    rest: torch.Tensor
    m: int
    rows: int
    rows_workspace: int
    workspace: torch.Tensor
    stride: int

    def neighbours(self, k: int):
        """(t_j float32, c_j int32) of EVERY entry of the closed row of explained row `k`, in ascending node id: views of the
        workspace at the offsets include/ggad_hip.h documents."""
        K, S, r = int(self.pos.numel()), self.stride, int(self.closed_size[k])
        t = self.workspace[k * S:k * S + r].view(torch.float32)
        return t, self.workspace[K * S + k * S:K * S + k * S + r]

    def completeness(self) -> float:
        """max over the rows of |z - (sum of the listed t_j + rest)|, on the device's own numbers."""
        if not self.logit.numel():
            return 0.0
        return float((self.logit - (self.nbr_contrib.sum(1) + self.rest)).abs().max())


def check_m(m, who: str, lib=None) -> None:
    """`ValueError` unless 1 <= m <= ggad_explain_max_nbrs() (asked of the library: no GPU needed)."""
    lib = lib or _lib.load()
    cap = int(lib.ggad_explain_max_nbrs())
    if isinstance(m, bool) or int(m) != m or not 1 <= int(m) <= cap:
        raise ValueError(f"{who}: m = {m} is outside 1..ggad_explain_max_nbrs() = {cap} (the neighbours listed per row)")


def _device_ints(x, what: str, dtype, dev) -> torch.Tensor:
    """`x` as a contiguous 1-D `dtype` tensor on `dev`: a tensor must already be there (a CPU tensor is refused, as `top_k` refuses
    CPU scores); anything else (a list, a numpy array) is uploaded."""
    if isinstance(x, torch.Tensor):
        if x.device.type != "cuda":
            raise ValueError(f"explain takes {what} on a GPU (there is no CPU path)")
        if x.dtype not in (torch.int32, torch.int64) or x.dim() != 1:
            raise ValueError(f"explain takes {what} as a 1-D int32 or int64 tensor")
        return x.to(device=dev, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(-1), dtype=np.int64)).to(device=dev, dtype=dtype)


def explain(model, ids, batch_size: int, positions, m: int, workspace: torch.Tensor = None) -> Explanation:
    """Explain the scores of `positions` (indices into `ids`, normally `Ranked.pos`; a `Ranked` is taken as its `pos`) of a sweep of
    `model` (the mini-batch `GCN`) over `ids` in slices of `batch_size`: one `ggad_explain_f32` call under the engine's CURRENT
    weights and one read-back of its four meta words (before it, one of three integers: the range of the positions and the longest
    explained row, which sizes the workspace).  `workspace`: an int32 device tensor to use if it is large enough (its content does
    not matter).  `ValueError` for `m` outside 1..ggad_explain_max_nbrs(), a position outside the list, a CPU tensor, a model
    without the mini-batch engine, or a NaN feature or weight on an explained row."""
    lib = _lib.load()
    check_m(m, "explain", lib)
    m = int(m)
    if int(batch_size) != batch_size or int(batch_size) < 1:
        raise ValueError(f"explain: batch_size = {batch_size} is not a positive integer")
    positions = getattr(positions, "pos", positions)
    for what, x in (("positions", positions), ("ids", ids)):
        if isinstance(x, torch.Tensor) and x.device.type != "cuda":
            raise ValueError(f"explain takes {what} on a GPU (there is no CPU path)")
    if not isinstance(positions, torch.Tensor):                  # host positions: checked before anything touches the device
        pa = np.asarray(positions).reshape(-1)
        n_ids = int(ids.numel()) if isinstance(ids, torch.Tensor) else int(np.asarray(ids).size)
        if pa.size and (int(pa.min()) < 0 or int(pa.max()) >= n_ids):
            raise ValueError(f"explain: positions {int(pa.min())}..{int(pa.max())} reach outside the scored list of {n_ids} ids")
    enc = getattr(model, "enc", None)
    eng = getattr(enc, "engine", None)
    if eng is None or not hasattr(eng, "params") or not hasattr(enc, "adj_lists"):
        raise ValueError("explain serves the mini-batch GGAD model (`GCN` with its `GCNEncoder`): the attribution is exact for its "
                         "bias-free one-ReLU score only")
    from .graphsage import _as_graph
    dev = eng.dev
    feat = enc.features.weight.data
    graph = _as_graph(enc.adj_lists, feat.shape[0], dev)
    if feat.dim() != 2 or feat.shape[1] != eng.F or not feat.is_contiguous() or feat.dtype != torch.float32:
        raise ValueError("explain: the feature table is not the contiguous float32 (N, F) table of the engine")
    ids = _device_ints(ids, "ids", torch.int64, dev)
    pos = _device_ints(positions, "positions", torch.int32, dev)
    n, K = int(ids.numel()), int(pos.numel())
    with torch.cuda.device(dev):
        stride = 1
        if K:
            p64 = pos.long()
            lo, hi = p64.min(), p64.max()
            node = ids[p64.clamp(0, max(0, n - 1))].clamp(0, graph.n - 1) if n else p64.clamp(0, 0)
            deg = (graph.rowptr[node + 1] - graph.rowptr[node]).max() if n else lo
            lo, hi, deg = (int(v) for v in torch.stack([lo, hi, deg.long()]).cpu().tolist())
            if lo < 0 or hi >= n:
                raise ValueError(f"explain: positions {lo}..{hi} reach outside the scored list of {n} ids")
            stride = deg + 1
        need = max(1, int(lib.ggad_explain_workspace_elems(stride, K, m)))
        if workspace is None or workspace.numel() < need or workspace.dtype != torch.int32 or workspace.device != dev:
            workspace = torch.empty(need, dtype=torch.int32, device=dev)
        F = eng.F
        out = Explanation(pos=pos, logit=torch.empty(K, dtype=torch.float32, device=dev),
                          feature=torch.empty((K, F), dtype=torch.float32, device=dev),
                          closed_size=torch.empty(K, dtype=torch.int32, device=dev),
                          nbr_id=torch.empty((K, m), dtype=torch.int64, device=dev),
                          nbr_contrib=torch.empty((K, m), dtype=torch.float32, device=dev),
                          nbr_colcount=torch.empty((K, m), dtype=torch.int32, device=dev),
                          rest=torch.empty(K, dtype=torch.float32, device=dev), m=m, rows=0, rows_workspace=0, workspace=workspace,
                          stride=stride)
        meta = torch.empty(4, dtype=torch.int64, device=dev)
        eng.sync_params()
        _lib.call("ggad_explain_f32", _lib.ptr(graph.rowptr), _lib.ptr(graph.col), graph.n, _lib.ptr(feat), _lib.ptr(eng.params), eng.D, F,
                  _lib.ptr(ids), n, int(batch_size), _lib.ptr(pos), K, m, stride, _lib.ptr(out.logit), _lib.ptr(out.feature),
                  _lib.ptr(out.closed_size), _lib.ptr(out.nbr_id), _lib.ptr(out.nbr_contrib), _lib.ptr(out.nbr_colcount),
                  _lib.ptr(out.rest), _lib.ptr(meta), _lib.ptr(workspace))
        status, out.rows, out.rows_workspace, _ = (int(v) for v in meta.cpu().tolist())
    if status == 3:
        raise ValueError("explain: a feature or a weight of an explained row is NaN")
    if status == 5:
        raise ValueError("explain: a position is outside the scored list, or an id of an explained slice is not a node of the graph")
    if status != 0:
        raise _lib.GgadKernelError(f"ggad_explain_f32 reported status {status}")
    return out


def write_explained(path, ranked, explanation: Explanation) -> None:
    """The `.npz` of config key `explain_out`: `node` int64 and `score` float32 of the `Ranked` list, and beside them, row for row,
    `logit`, `feature`, `closed_size`, `nbr_id`, `nbr_contrib`, `nbr_colcount`, `rest` of the `Explanation` of `ranked.pos`.  Entries
    are stored with a fixed date (`write_ranked`'s writer), so equal explanations give equal files byte for byte."""
    from .metrics import write_npz_fixed_date
    e = explanation
    if int(e.logit.shape[0]) != int(ranked.ids.shape[0]):
        raise ValueError("write_explained: the explanation does not cover the ranked list row for row")
    arrays = {"node": ranked.ids.cpu().numpy().astype(np.int64), "score": ranked.scores.cpu().numpy().astype(np.float32),
              "logit": e.logit.cpu().numpy().astype(np.float32), "feature": e.feature.cpu().numpy().astype(np.float32),
              "closed_size": e.closed_size.cpu().numpy().astype(np.int32), "nbr_id": e.nbr_id.cpu().numpy().astype(np.int64),
              "nbr_contrib": e.nbr_contrib.cpu().numpy().astype(np.float32),
              "nbr_colcount": e.nbr_colcount.cpu().numpy().astype(np.int32), "rest": e.rest.cpu().numpy().astype(np.float32)}
    write_npz_fixed_date(path, arrays)
