"""Sparse restatement of the PC-GNN arithmetic (three relations -> InterAgg -> PCALayer) in a chosen dtype, on the CPU with torch
autograd.  Not a test: the helper the PC-GNN device tests measure against (float64 = the reference value, float32 = the yardstick
for what float32 arithmetic costs).

Per relation, with N(.) the CSR rows and b_0 .. b_{B-1} the batch (a node listed twice is two rows):
    U = union of N(b_i), ascending;  r_u = |N(u)|;  c_v = |{u in U : v in N(u)}|
    A1[i] = mean_{v in N(b_i)} X[v]                      T1 = relu(A1 W_r)
    A2[u] = sum_{v in N(u)} X[v] (1 / sqrt r_u) / sqrt c_v   T2 = relu(A2 W_r)
    NB[i] = mean_{u in N(b_i)} T2[u]
combined = relu([T1_1 | T1_2 | T1_3] W), neigh = relu([NB_1 | NB_2 | NB_3] W), affinity = row-wise cosine (NaN -> 0),
scores = combined W_head^T, loss = cross entropy + 5 max(0, 1 - (mean affinity of label 0 - mean affinity of label 1))."""
import numpy as np
import torch

PARAMS = ("inter1.weight", "inter1.intra_agg1.weight", "inter1.intra_agg2.weight", "inter1.intra_agg3.weight", "weight")


def plan_numpy(rowptr, col, batch):
    """The integer plan of one relation: (U ascending, pos (N, -1 outside U), row_count (|U|), col_count (N, 0 where unused))."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(rowptr) - 1
    batch = np.asarray(batch, dtype=np.int64)
    in_u = np.zeros(n, dtype=bool)
    for b in batch:
        in_u[col[rowptr[b]:rowptr[b + 1]]] = True
    unique = np.flatnonzero(in_u)
    pos = np.full(n, -1, dtype=np.int64)
    pos[unique] = np.arange(len(unique))
    row_count = rowptr[unique + 1] - rowptr[unique]
    col_count = np.zeros(n, dtype=np.int64)
    for u in unique:
        col_count[col[rowptr[u]:rowptr[u + 1]]] += 1
    return unique, pos, row_count, col_count


def _entries(rowptr, col, rows):
    """(row index, column) of every entry of the listed CSR rows, row after row."""
    deg = rowptr[rows + 1] - rowptr[rows]
    seg = np.repeat(np.arange(len(rows)), deg)
    offs = np.arange(int(deg.sum())) - np.repeat(np.cumsum(deg) - deg, deg)
    return seg, col[np.repeat(rowptr[rows], deg) + offs], deg


def _relation(rowptr, col, batch, x, w, dtype):
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    batch = np.asarray(batch, dtype=np.int64)
    unique, pos, row_count, col_count = plan_numpy(rowptr, col, batch)
    seg1, col1, deg1 = _entries(rowptr, col, batch)
    seg2, col2, _ = _entries(rowptr, col, unique)
    one = torch.ones((), dtype=dtype)
    w1 = (one / torch.from_numpy(deg1).to(dtype))[torch.from_numpy(seg1)]
    r_u = torch.from_numpy(row_count).to(dtype)[torch.from_numpy(seg2)]
    c_v = torch.from_numpy(col_count[col2]).to(dtype)
    w2 = (one / torch.sqrt(r_u)) / torch.sqrt(c_v)
    s1, s2 = torch.from_numpy(seg1), torch.from_numpy(seg2)
    a1 = torch.zeros(len(batch), x.shape[1], dtype=dtype).index_add_(0, s1, x[torch.from_numpy(col1)] * w1[:, None])
    a2 = torch.zeros(len(unique), x.shape[1], dtype=dtype).index_add_(0, s2, x[torch.from_numpy(col2)] * w2[:, None])
    t1 = torch.relu(a1 @ w)
    t2 = torch.relu(a2 @ w)
    nb = torch.zeros(len(batch), w.shape[1], dtype=dtype).index_add_(0, s1, t2[torch.from_numpy(pos[col1])] * w1[:, None])
    return t1, nb


def evaluate(relations, feat, batch, labels, weights, dtype=torch.float64, objective=None):
    """`relations`: three (rowptr, col); `weights`: dict over PARAMS (numpy).  Returns numpy float64 arrays: combined (B, D),
    affinity (B), loss (2: total, constraint), prob_gnn (B, 2) and grad.<name> for every parameter.  `objective(scores, affinity)`
    replaces the PC-GNN loss as the scalar that is differentiated (a batch without both labels has no finite loss: the mean
    affinity of the missing label is 0 / 0); the constraint slot of `loss` is then 0."""
    x = torch.from_numpy(np.asarray(feat)).to(dtype)
    p = {k: torch.from_numpy(np.asarray(weights[k])).to(dtype).requires_grad_(True) for k in PARAMS}
    labels = torch.from_numpy(np.asarray(labels, dtype=np.int64))
    t1s, nbs = [], []
    for k, (rowptr, col) in enumerate(relations):
        t1, nb = _relation(rowptr, col, batch, x, p[f"inter1.intra_agg{k + 1}.weight"], dtype)
        t1s.append(t1)
        nbs.append(nb)
    combined = torch.relu(torch.cat(t1s, 1) @ p["inter1.weight"])
    neigh = torch.relu(torch.cat(nbs, 1) @ p["inter1.weight"])
    cn = combined / torch.norm(combined, dim=-1, keepdim=True)
    cn = torch.where(torch.isnan(cn), torch.zeros_like(cn), cn)
    nn_ = neigh / torch.norm(neigh, dim=-1, keepdim=True)
    nn_ = torch.where(torch.isnan(nn_), torch.zeros_like(nn_), nn_)
    affinity = (nn_ * cn).sum(1)
    scores = combined @ p["weight"].t()
    if objective is None:
        xent = torch.nn.functional.cross_entropy(scores, labels)
        con = (1 - (affinity[labels == 0].mean() - affinity[labels == 1].mean())).clamp_min(0)
        loss = xent + 5 * con
    else:
        loss, con = objective(scores, affinity), torch.zeros((), dtype=dtype)
    loss.backward()
    out = {"combined": combined, "affinity": affinity, "loss": torch.stack([loss, con]), "prob_gnn": torch.sigmoid(scores)}
    out.update({"grad." + k: p[k].grad for k in PARAMS})
    return {k: v.detach().to(torch.float64).numpy() for k, v in out.items()}
