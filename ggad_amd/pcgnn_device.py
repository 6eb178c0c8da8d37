"""Device path of the PC-GNN comparison model: `InterAgg` on relation graphs kept as CSR in HBM (`DeviceGraph`).

What `layers.IntraAgg.forward` does per batch and relation with python sets, `np.unique` and a dense B x U mask runs here as HIP
kernels (`csrc/pcgnn.hip`): the neighbourhood plan (U in ascending id order, `pos`, the column counts), the fused hop kernel
(gather, aggregate, project by the relation's weight held in LDS, ReLU) for both the batch rows and the rows of U, and the mean
of the 2-hop embeddings over the batch rows with its transpose for the backward.  `combined` and `affinity` are sums over U, so
the order of U does not change them.  |U| is never read back: buffers have the capacity min(N, sum of the batch
rows' degrees), known from `rowptr_host`, and the rows past |U| are zeros.  There is no fallback: shapes the hop kernel does not
take raise at construction.

Opt-in on top (`fused`, config key `pcgnn_fused`): what follows the relations -- both 3D -> D projections, the norms, the affinity,
the class scores, `PCALayer.loss` and all their gradients -- runs in `csrc/pcgnn_head.hip` (`PcgnnHeadFn`, four launches; one for
`to_prob`) instead of torch ops, without `argwhere` or any other wait for the device."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._lib import call
from .fullgraph import LinearFn, gemm
from .graph import DeviceGraph
from .graphsage import _node_array


def check_relation(rowptr, col) -> None:
    """Host-only check of one CSR relation, once at construction: every row non-empty, sorted and duplicate-free (an empty row makes
    the reference's own mean 0 / 0), every column a node id.  Raises `ValueError` naming the first offending row."""
    rowptr = np.asarray(rowptr, dtype=np.int64).reshape(-1)
    col = np.asarray(col, dtype=np.int64).reshape(-1)
    n = len(rowptr) - 1
    if n < 1 or rowptr[0] != 0 or rowptr[-1] != len(col) or (np.diff(rowptr) < 0).any():
        raise ValueError("relation graph: rowptr is not a CSR row pointer of col")
    if len(col) and (col.min() < 0 or col.max() >= n):
        e = int(np.flatnonzero((col < 0) | (col >= n))[0])
        raise ValueError(f"relation graph: row {int(np.searchsorted(rowptr, e, side='right') - 1)} holds column {int(col[e])}, "
                         f"outside [0, {n})")
    bad = []
    empty = np.flatnonzero(np.diff(rowptr) == 0)
    if len(empty):
        bad.append((int(empty[0]), "is empty (the reference's mean over it is 0 / 0)"))
    if len(col) > 1:
        step = np.diff(col)
        inner = np.ones(len(col) - 1, dtype=bool)                  # pairs (e, e + 1) inside one row
        starts = rowptr[1:-1]
        starts = starts[(starts > 0) & (starts < len(col))]
        inner[starts - 1] = False
        for mask, what in ((inner & (step < 0), "is not sorted"), (inner & (step == 0), "holds a duplicate")):
            e = np.flatnonzero(mask)
            if len(e):
                bad.append((int(np.searchsorted(rowptr, e[0], side="right") - 1), what))
    if bad:
        row, what = min(bad)
        raise ValueError(f"relation graph: row {row} {what}")


def _dptr(t, dtype, what: str) -> int:
    """Device pointer of a tensor handed to a `ggad_pcgnn_*` entry point; anything the C ABI cannot read raises before a launch."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f"{what}: expected a contiguous {dtype} tensor on the GPU")
    return t.data_ptr()


class RelationPlan:
    """The neighbourhood plan of one batch on one relation, as tensors: `unique` (cap, ascending ids, -1 past |U|), `row_count`
    (cap, |N(u)|, 0 past |U|), `n_unique` (1), and views of the relation's N-sized scratch that hold until `release()`: `pos`
    (index in U, -1 outside) and `col_count` (c_v, 0 where no row of U has v)."""

    def __init__(self, state, batch, cap):
        self.state, self.batch, self.cap = state, batch, int(cap)
        dev = state.pos.device
        self.unique = torch.empty(self.cap, dtype=torch.int32, device=dev)
        self.row_count = torch.empty(self.cap, dtype=torch.int32, device=dev)
        self.n_unique = torch.empty(1, dtype=torch.int32, device=dev)
        self.pos, self.col_count = state.pos, state.cnt
        self.released = False

    def release(self) -> None:
        """Puts the relation's scratch back (pos = -1, counts = 0) by walking the rows of U again."""
        if self.released:
            return
        g = self.state.graph
        call("ggad_pcgnn_plan_reset", g.rowptr.data_ptr(), g.col.data_ptr(), self.unique.data_ptr(), self.n_unique.data_ptr(),
             self.cap, self.state.pos.data_ptr(), self.state.cnt.data_ptr())
        self.released = True
        self.pos = self.col_count = None
        self.state.open_plan = None


class RelationState:
    """One relation graph and its N-sized integer scratch, which is clean (bitmap 0, pos -1, counts 0) between batches."""

    def __init__(self, graph: DeviceGraph):
        if not isinstance(graph, DeviceGraph):
            raise ValueError("the device path of PC-GNN takes DeviceGraph relations")
        check_relation(graph.rowptr_host, graph.col_host)
        if graph.device.type != "cuda":
            raise ValueError("the device path of PC-GNN needs its relation graphs on the GPU")
        self.graph = graph
        lib = _lib.load()
        dev = graph.device
        self.scan = torch.zeros(int(lib.ggad_pcgnn_scan_elems(graph.n)), dtype=torch.int32, device=dev)
        self.pos = torch.full((graph.n,), -1, dtype=torch.int32, device=dev)
        self.cnt = torch.zeros(graph.n, dtype=torch.int32, device=dev)
        self.open_plan = None
        self.last = {}                                             # buffers of the latest forward / backward (tests, profiling)

    def capacity(self, nodes: np.ndarray) -> int:
        """Rows of every |U|-sized buffer for this batch: min(N, sum of the batch rows' degrees), from the host row pointer."""
        return int(min(self.graph.n, int(self.graph.deg_host[nodes].sum())))

    def upload(self, nodes) -> torch.Tensor:
        nodes = _node_array(nodes)
        if len(nodes) == 0 or nodes.min() < 0 or nodes.max() >= self.graph.n:
            raise ValueError(f"batch nodes must be a non-empty list of ids in [0, {self.graph.n})")
        return torch.from_numpy(nodes.astype(np.int32)).to(self.graph.device)

    def plan(self, batch: torch.Tensor, cap: int) -> RelationPlan:
        """Builds the plan of the device batch `batch` (int32 ids); the caller releases it before the next one."""
        if self.open_plan is not None:
            self.open_plan.release()
        if cap < 1 or cap > self.graph.n:
            raise ValueError("plan capacity must be in [1, N]")
        g = self.graph
        p = RelationPlan(self, batch, cap)
        call("ggad_pcgnn_plan", g.rowptr.data_ptr(), g.col.data_ptr(), g.n, _dptr(batch, torch.int32, "batch"), int(batch.numel()),
             p.cap, self.scan.data_ptr(), self.pos.data_ptr(), self.cnt.data_ptr(), p.unique.data_ptr(), p.row_count.data_ptr(),
             p.n_unique.data_ptr())
        self.open_plan = p
        return p


class PcgnnRelationFn(torch.autograd.Function):
    """(T1, NB) of one relation: T1 = relu(A1 W) on the batch rows, NB = the batch rows' mean of T2 = relu(A2 W) over U.  The
    gradient goes to W only (the feature table is frozen): dW = [A1; A2]^T [dZ1; dZ2], one product over B + cap rows whose
    padding rows are zeros on both sides."""

    @staticmethod
    def forward(ctx, weight, state, feat, batch, cap):
        g = state.graph
        f, d = int(weight.shape[0]), int(weight.shape[1])
        b = int(batch.numel())
        w = weight.detach()
        plan = state.plan(batch, cap)
        a = torch.empty(b + cap, f, dtype=torch.float32, device=feat.device)       # [A1; A2]
        t = torch.empty(b + cap, d, dtype=torch.float32, device=feat.device)       # [T1; T2]
        nb = torch.empty(b, d, dtype=torch.float32, device=feat.device)
        fp, wp = _dptr(feat, torch.float32, "feature table"), _dptr(w, torch.float32, "relation weight")
        rp, cp, bp = g.rowptr.data_ptr(), g.col.data_ptr(), batch.data_ptr()
        call("ggad_pcgnn_hop_f32", fp, f, rp, cp, bp, 0, b, 0, wp, d, a.data_ptr(), t.data_ptr())
        call("ggad_pcgnn_hop_f32", fp, f, rp, cp, plan.unique.data_ptr(), plan.n_unique.data_ptr(), cap, state.cnt.data_ptr(), wp, d,
             a[b:].data_ptr(), t[b:].data_ptr())
        call("ggad_pcgnn_nb_fwd_f32", t[b:].data_ptr(), d, rp, cp, bp, b, state.pos.data_ptr(), nb.data_ptr())
        plan.release()
        ctx.save_for_backward(a, t, batch, plan.unique, plan.n_unique)
        ctx.state, ctx.dims = state, (b, cap, f, d)
        state.last = {"plan": plan, "a": a, "t": t, "nb": nb, "batch_rows": b}
        return t[:b], nb

    @staticmethod
    def backward(ctx, dt1, dnb):
        a, t, batch, unique, n_unique = ctx.saved_tensors
        b, cap, f, d = ctx.dims
        g = ctx.state.graph
        dz = torch.empty(b + cap, d, dtype=torch.float32, device=a.device)         # [dZ1; dZ2]
        dt1 = torch.zeros(b, d, device=a.device) if dt1 is None else dt1.contiguous()
        dnb = torch.zeros(b, d, device=a.device) if dnb is None else dnb.contiguous()
        call("ggad_relu_bwd_f32", _dptr(dt1, torch.float32, "dT1"), t.data_ptr(), b * d, dz.data_ptr())
        call("ggad_pcgnn_nb_bwd_f32", _dptr(dnb, torch.float32, "dNB"), t[b:].data_ptr(), d, g.rowptr.data_ptr(), g.col.data_ptr(),
             batch.data_ptr(), b, unique.data_ptr(), n_unique.data_ptr(), cap, dz[b:].data_ptr())
        ctx.state.last["dz"] = dz
        return gemm(a, dz, True, False), None, None, None, None


def _head_args(t1s, nbs, weight, cls_weight, labels):
    """Shapes and pointers of one head call, checked on the host before any launch: (B, D, the nine input pointers)."""
    if len(t1s) != 3 or len(nbs) != 3:
        raise ValueError("the PC-GNN head takes three relations")
    if not isinstance(t1s[0], torch.Tensor) or t1s[0].dim() != 2:
        raise ValueError("T1 of relation 0: expected a (B, D) tensor")
    b, d = int(t1s[0].shape[0]), int(t1s[0].shape[1])
    lib = _lib.load()
    if not lib.ggad_pcgnn_head_supported(b, d):
        raise ValueError(f"the PC-GNN head kernels take B >= 1 and 1 <= embed_dim <= {int(lib.ggad_max_embed_dim())}; got ({b}, {d})")
    ptrs = []
    for name, group in (("T1", t1s), ("NB", nbs)):
        for r, t in enumerate(group):
            ptrs.append(_dptr(t, torch.float32, f"{name} of relation {r}"))
            if tuple(t.shape) != (b, d):
                raise ValueError(f"{name} of relation {r}: expected shape ({b}, {d}), got {tuple(t.shape)}")
    ptrs.append(_dptr(weight, torch.float32, "InterAgg.weight"))
    ptrs.append(_dptr(cls_weight, torch.float32, "PCALayer.weight"))
    if tuple(weight.shape) != (3 * d, d) or tuple(cls_weight.shape) != (2, d):
        raise ValueError(f"the PC-GNN head takes InterAgg.weight ({3 * d}, {d}) and PCALayer.weight (2, {d}); got "
                         f"{tuple(weight.shape)} and {tuple(cls_weight.shape)}")
    if labels is None:
        ptrs.append(0)
    else:
        ptrs.append(_dptr(labels, torch.int64, "labels"))
        if labels.numel() != b:
            raise ValueError(f"labels: expected {b} entries, got {labels.numel()}")
    return b, d, ptrs


def pcgnn_head_forward(t1s, nbs, weight, cls_weight):
    """(scores (B, 2), affinity (B)) of the head in ONE launch (`ggad_pcgnn_head_f32` without a loss): nothing else is written and
    no gradient buffer exists."""
    b, d, ptrs = _head_args(t1s, nbs, weight, cls_weight, None)
    dev = weight.device
    scores = torch.empty(b, 2, dtype=torch.float32, device=dev)
    affinity = torch.empty(b, dtype=torch.float32, device=dev)
    call("ggad_pcgnn_head_f32", *ptrs, b, d, scores.data_ptr(), affinity.data_ptr(), *([0] * 10))
    return scores, affinity


class PcgnnHeadFn(torch.autograd.Function):
    """(total (1), constraint (1), scores (B, 2), affinity (B)) of `InterAgg`'s two projections, the cosine affinity, the class
    scores and `PCALayer.loss`, from the three relations' (T1, NB), `InterAgg.weight`, `PCALayer.weight` and int64 labels.  All
    eight gradients of `total` are computed by the forward call (four launches, csrc/pcgnn_head.hip) into one flat buffer and scaled
    by the incoming gradient in `backward`; only `total` is differentiable.  `buffers`: optional dict that receives the outputs, the
    flat gradient buffer and the workspace, all flat float32 (or supplies pre-filled ones under the same keys: the determinism test);
    the workspace starts with `combined` and `neigh`, B x D each."""

    @staticmethod
    def forward(ctx, t1_0, nb_0, t1_1, nb_1, t1_2, nb_2, weight, cls_weight, labels, buffers=None):
        t1s, nbs = [t.detach() for t in (t1_0, t1_1, t1_2)], [t.detach() for t in (nb_0, nb_1, nb_2)]
        w, wc = weight.detach(), cls_weight.detach()
        b, d, ptrs = _head_args(t1s, nbs, w, wc, labels)
        dev = w.device
        lib = _lib.load()
        buffers = {} if buffers is None else buffers
        sizes = [b * d] * 6 + [3 * d * d, 2 * d]

        def buf(key, n):
            t = buffers.get(key)
            if t is None:
                t = buffers[key] = torch.empty(n, dtype=torch.float32, device=dev)
            _dptr(t, torch.float32, key)
            if t.numel() != n:
                raise ValueError(f"{key}: expected {n} floats, got {t.numel()}")
            return t
        scores, affinity, loss = buf("scores", 2 * b), buf("affinity", b), buf("loss", 2)
        grads = buf("grads", sum(sizes))
        ws = buf("ws", int(lib.ggad_pcgnn_head_workspace_elems(b, d)))
        offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
        gp = [grads.data_ptr() + 4 * o for o in offs[:8]]
        # flat order: dT1_0, dT1_1, dT1_2, dNB_0, dNB_1, dNB_2, dW, dW_cls
        call("ggad_pcgnn_head_f32", *ptrs, b, d, scores.data_ptr(), affinity.data_ptr(), loss.data_ptr(), *gp, ws.data_ptr())
        ctx.grads, ctx.offs, ctx.dims = grads, offs, (b, d)
        scores, affinity = scores.view(b, 2), affinity
        total, constraint = loss[0:1], loss[1:2]
        ctx.mark_non_differentiable(constraint, scores, affinity)
        return total, constraint, scores, affinity

    @staticmethod
    def backward(ctx, g, _gc, _gs, _ga):
        b, d = ctx.dims
        flat = ctx.grads * g                                       # one launch for all eight
        o = ctx.offs
        shapes = [(b, d)] * 6 + [(3 * d, d), (2, d)]
        dt1_0, dt1_1, dt1_2, dnb_0, dnb_1, dnb_2, dw, dwc = (flat[o[i]:o[i + 1]].view(shapes[i]) for i in range(8))
        return dt1_0, dnb_0, dt1_1, dnb_1, dt1_2, dnb_2, dw, dwc, None, None


class PcgnnDevice:
    """What `InterAgg` holds when every relation is a `DeviceGraph`: one `RelationState` per relation, checked once.  `fused`: the
    head behind the relations (both 3D -> D projections, the affinity, the class scores, `PCALayer.loss` and their backward) runs in
    csrc/pcgnn_head.hip instead of torch ops; off, nothing here changes."""

    def __init__(self, features, feat_dim: int, embed_dim: int, graphs, fused: bool = False):
        lib = _lib.load()
        if not lib.ggad_pcgnn_supported(int(feat_dim), int(embed_dim)):
            raise ValueError(f"the PC-GNN hop kernel takes 1 <= feat_dim <= {int(lib.ggad_pcgnn_max_feat_dim())} and "
                             f"1 <= embed_dim <= {int(lib.ggad_max_embed_dim())}; got ({feat_dim}, {embed_dim})")
        table = features.weight
        if table.dim() != 2 or table.shape[1] != feat_dim:
            raise ValueError("feature table width differs from feat_dim")
        for g in graphs:
            if isinstance(g, DeviceGraph) and (g.n > table.shape[0] or g.device != table.device):
                raise ValueError("a relation graph has more nodes than the feature table has rows, or lives on another device")
        self.states = [RelationState(g) for g in graphs]
        self.fused = bool(fused)
        self.last_head = {}

    def relations(self, inter, nodes):
        """([T1_0, T1_1, T1_2], [NB_0, NB_1, NB_2]) of the batch from the CSR relations."""
        nodes = _node_array(nodes)
        feat = inter.features.weight.data
        batch = self.states[0].upload(nodes)
        r_feats, nb_feats = [], []
        for agg, st in zip((inter.intra_agg1, inter.intra_agg2, inter.intra_agg3), self.states):
            if st.graph.n != self.states[0].graph.n:
                st.upload(nodes)                                   # (range check against this relation's own size)
            t1, nb = PcgnnRelationFn.apply(agg.weight, st, feat, batch, st.capacity(nodes))
            r_feats.append(t1)
            nb_feats.append(nb)
        return r_feats, nb_feats

    def forward(self, inter, nodes):
        """`InterAgg.forward` from the CSR relations: (combined.t(), affinity)."""
        r_feats, nb_feats = self.relations(inter, nodes)
        wt = inter.weight.t().contiguous()
        combined = LinearFn.apply(torch.cat(r_feats, dim=1), wt, True)
        neigh = LinearFn.apply(torch.cat(nb_feats, dim=1), wt, True)
        cn = combined / torch.norm(combined, dim=-1, keepdim=True)
        cn = torch.where(torch.isnan(cn), torch.full_like(cn, 0), cn)
        nn_ = neigh / torch.norm(neigh, dim=-1, keepdim=True)
        nn_ = torch.where(torch.isnan(nn_), torch.full_like(nn_, 0), nn_)
        affinity = (nn_ * cn).sum(1)
        return combined.t(), affinity

    def head_loss(self, inter, cls_weight, nodes, labels):
        """`PCALayer.loss` on the fused route: (total (1), constraint (1)); `labels`: int64 device tensor, one per node."""
        r_feats, nb_feats = self.relations(inter, nodes)
        buffers = {}
        total, constraint, _, _ = PcgnnHeadFn.apply(r_feats[0], nb_feats[0], r_feats[1], nb_feats[1], r_feats[2], nb_feats[2],
                                                    inter.weight, cls_weight, labels.reshape(-1), buffers)
        self.last_head = buffers                                   # buffers of the latest training call (tests, profiling)
        return total, constraint

    def head_forward(self, inter, cls_weight, nodes):
        """`PCALayer.forward` on the fused route, forward only: (scores (B, 2), affinity (B)), no graph recorded."""
        with torch.no_grad():
            r_feats, nb_feats = self.relations(inter, nodes)
            return pcgnn_head_forward(r_feats, nb_feats, inter.weight.detach(), cls_weight.detach())
