#!/usr/bin/env python3
"""Generate the full-graph AnomalyDAE fixtures from the *imported* reference `model_AnomalyDAE.py`.

Runs only where the reference tree is present (see make_golden.py).  The reference imports `dgl` (unused) and
`torch_geometric.nn.GATConv`; the first is stubbed empty, the second by `PygGATConv` below, a restatement of
torch_geometric 2.1.0 (the version the reference pins).  `anomalyDAE.py` has no `__main__` guard and needs dgl and a
dataset file, so its training loop is restated here line by line.  Inputs come from `ggad_amd.synth`; the fixtures are data.

    python tests/golden/make_golden_anomalydae.py       # writes tests/golden/fullgraph_anomalydae{,_planted}.npz
"""
from __future__ import annotations

import math
import os
import random
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from ggad_amd import synth  # noqa: E402


def _glorot(t):
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    t.data.uniform_(-a, a)


class PygLinear(nn.Module):
    """torch_geometric.nn.dense.Linear(in, out, bias=False, weight_initializer='glorot') of PyG 2.1.0: the constructor calls
    reset_parameters(), which draws the weight glorot-uniform (`inits.glorot`: U(-a, a), a = sqrt(6 / (fan_in + fan_out)))."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels))
        self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        _glorot(self.weight)

    def forward(self, x):
        return x @ self.weight.t()


class PygGATConv(nn.Module):
    """torch_geometric 2.1.0 `GATConv(in_channels, out_channels)` with every default, restated.  Assumptions:

    - heads = 1, concat = True, negative_slope = 0.2, dropout = 0, add_self_loops = True, edge_dim = None, bias = True;
    - `lin_src` = Linear(in, out, bias=False, glorot) is drawn by its own constructor; `lin_dst` is the same module; then
      `reset_parameters()` re-draws it through `lin_src` and again through `lin_dst` (three draws of one weight in all);
    - `att_src`, `att_dst` of shape (1, 1, out) are then drawn glorot (in that order), `bias` (out,) is zeros;
    - forward: x_src = x_dst = lin_src(x); alpha_src = (x_src * att_src).sum(-1), alpha_dst likewise; `remove_self_loops` drops
      the edges with source == target, `add_self_loops` appends one loop (i, i) per node after the remaining edges;
    - edge e = (j -> i) (edge_index[0] = source j, [1] = target i): alpha_e = leaky_relu(alpha_src[j] + alpha_dst[i], 0.2),
      softmax over the edges of each target: exp(alpha - max) / (sum + 1e-16), the max taken per target (softmax is
      shift-invariant, so its gradient through the max is zero; it is treated as a constant);
    - message alpha_e * x_src[j], summed at the target ('add' aggregation), concatenated heads (a view for one head), + bias.
    """

    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        if kwargs:
            raise ValueError("the stub restates the defaults only")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, 1
        self.lin_src = PygLinear(in_channels, out_channels)
        self.lin_dst = self.lin_src
        self.att_src = nn.Parameter(torch.empty(1, 1, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, 1, out_channels))
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        self.lin_src.reset_parameters()
        self.lin_dst.reset_parameters()
        _glorot(self.att_src)
        _glorot(self.att_dst)
        self.bias.data.fill_(0.0)

    def forward(self, x, edge_index):
        n, C = x.shape[0], self.out_channels
        x_src = self.lin_src(x).view(-1, 1, C)
        a_src = (x_src * self.att_src).sum(-1)
        a_dst = (x_src * self.att_dst).sum(-1)
        ei = torch.as_tensor(edge_index, dtype=torch.long).reshape(2, -1)
        ei = ei[:, ei[0] != ei[1]]
        loop = torch.arange(n, dtype=torch.long)
        src = torch.cat([ei[0], loop])
        dst = torch.cat([ei[1], loop])
        alpha = torch.nn.functional.leaky_relu(a_src[src] + a_dst[dst], 0.2)           # (E, 1)
        amax = torch.full((n, 1), -math.inf, dtype=alpha.dtype).scatter_reduce(0, dst.view(-1, 1), alpha.detach(), "amax",
                                                                              include_self=True)
        ex = (alpha - amax[dst]).exp()
        den = torch.zeros((n, 1), dtype=alpha.dtype).index_add(0, dst, ex)
        p = ex / (den[dst] + 1e-16)
        out = torch.zeros((n, 1, C), dtype=x_src.dtype).index_add(0, dst, p.unsqueeze(-1) * x_src[src])
        return out.view(-1, C) + self.bias


def dense_gat(h, w, att_src, att_dst, bias, adj):
    """The same layer as a dense masked softmax: target i aggregates over {r != i : adj[r, i] > 0} + {i}."""
    y = h @ w.t()
    als, ald = y @ att_src.reshape(-1), y @ att_dst.reshape(-1)
    n = y.shape[0]
    eye = torch.eye(n, dtype=torch.bool)
    mask = ((adj > 0) & ~eye) | eye                                               # mask[r, i]: edge r -> i
    e = torch.nn.functional.leaky_relu(als[:, None] + ald[None, :], 0.2)
    e = e.masked_fill(~mask, -math.inf)
    p = torch.softmax(e, dim=0)                                                    # over the sources r of each target i
    return p.t() @ y + bias


def _stub_modules():
    sys.modules["dgl"] = types.ModuleType("dgl")
    tg = types.ModuleType("torch_geometric")
    tgnn = types.ModuleType("torch_geometric.nn")
    tgnn.GATConv = PygGATConv
    tgnn.GCNConv = object
    tg.nn = tgnn
    sys.modules["torch_geometric"] = tg
    sys.modules["torch_geometric.nn"] = tgnn


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _inputs(n, n_entries, f, seed, self_loop_frac, isolated, planted=None):
    rowptr, col = synth.make_graph(n, n_entries, seed, kind="powerlaw", max_degree=n // 4, self_loop_frac=self_loop_frac)
    feat = synth.make_features(n, f, seed)
    ano = synth.make_labels(n, 0.1, seed)
    if planted:
        rowptr, col, feat = synth.plant_anomalies(rowptr, col, feat, ano, seed, **planted)
    if isolated:
        # the last node loses its entries (its own row and the other rows' entries to it): a node with only the added self loop
        import scipy.sparse as sp
        a = synth.csr_to_scipy(rowptr, col, n).tolil()
        a[n - 1, :] = 0
        a[:, n - 1] = 0
        a = sp.csr_matrix(a)
        a.eliminate_zeros()
        rowptr, col = a.indptr.astype(np.int64), a.indices.astype(np.int64)
    return rowptr, col, feat, ano


def _split(n, ano, seed):
    random.seed(seed)
    all_idx = list(range(n))
    random.shuffle(all_idx)
    idx_train, idx_test = all_idx[:int(n * 0.3)], all_idx[int(n * 0.3) + int(n * 0.1):]
    normal = [i for i in idx_train if ano[i] == 0]
    return normal, idx_test


def _prep(rowptr, col, feat, n, f, rutils):
    import scipy.sparse as sp
    adj_sp = synth.csr_to_scipy(rowptr, col, n)
    feats_dense, _ = rutils.preprocess_features(sp.lil_matrix(feat))                # anomalyDAE.py:80-81
    adj_norm = rutils.normalize_adj(adj_sp)                                          # :92-93
    features = torch.FloatTensor(np.asarray(feats_dense)[np.newaxis])
    adj = torch.FloatTensor(np.asarray((adj_norm + sp.eye(n)).todense())[np.newaxis])
    return features, adj


def model_case(tag, n, n_entries, f, n_h, seed, k_steps, lr, self_loop_frac, isolated):
    from model_AnomalyDAE import Model            # /root/reference/model_AnomalyDAE.py
    import utils as rutils                        # /root/reference/utils.py
    rowptr, col, feat, ano = _inputs(n, n_entries, f, seed, self_loop_frac, isolated)
    normal_idx, idx_test = _split(n, ano, seed)
    features, adj = _prep(rowptr, col, feat, n, f, rutils)
    torch.manual_seed(seed)
    model = Model(f, n_h, "prelu", 1, "avg")
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0.0)
    out = {f"{tag}.{k}": v for k, v in dict(n=n, f=f, n_h=n_h, seed=seed, lr=lr, rowptr=rowptr, col=col, feat_raw=feat, ano=ano,
                                             features=_np(features[0]), idx_test=np.array(idx_test),
                                             normal_idx=np.array(normal_idx)).items()}
    for k, v in model.state_dict().items():
        out[f"{tag}.init.{k}"] = _np(v).copy()
    losses, scores = [], []
    for step in range(k_steps):                  # anomalyDAE.py:130-145
        model.train()
        opt.zero_grad()
        loss, score = model(features, adj, normal_idx, idx_test)
        loss.backward()
        if step == 0:
            x = torch.squeeze(features)
            xhat, s_ = model.model_enc(x, torch.tensor(np.array(
                [(i, j) for i in range(n) for j in np.flatnonzero(_np(adj[0, i]) > 0)])).T)
            adj2 = torch.squeeze(adj)
            nrm = normal_idx
            attr = torch.sqrt(torch.sum((x[nrm] - xhat[nrm]) ** 2, 1))
            stru = torch.sqrt(torch.sum((adj2[nrm] - s_[nrm]) ** 2, 1))
            out.update({f"{tag}.z": _np(model.emb), f"{tag}.xhat": _np(xhat), f"{tag}.attr": _np(attr), f"{tag}.stru": _np(stru),
                        f"{tag}.loss0": np.float64(loss.item()), f"{tag}.score_test0": _np(score)})
            for k, p in model.named_parameters():
                if p.grad is not None:
                    out[f"{tag}.grad.{k}"] = _np(p.grad).copy()
        losses.append(loss.item())
        scores.append(_np(score))
        opt.step()
    out[f"{tag}.losses"] = np.array(losses, dtype=np.float64)
    out[f"{tag}.scores"] = np.stack(scores)
    for k, v in model.state_dict().items():
        out[f"{tag}.final.{k}"] = _np(v).copy()
    print(tag, "losses", losses)
    return out


def planted_case(n=600, n_entries=5000, f=32, n_h=64, seed=2, num_epoch=100, lr=3e-3):
    """The restated loop of anomalyDAE.py on planted anomalies: AUROC / AP of the epoch's training-forward test scores every 5."""
    from model_AnomalyDAE import Model
    import utils as rutils
    from sklearn.metrics import average_precision_score, roc_auc_score
    rowptr, col, feat, ano = _inputs(n, n_entries, f, seed, 0.0, False, planted=dict(scale=0.25, rewire=0.5))
    normal_idx, idx_test = _split(n, ano, seed)
    features, adj = _prep(rowptr, col, feat, n, f, rutils)
    torch.manual_seed(seed)
    model = Model(f, n_h, "prelu", 1, "avg")
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0.0)
    yt = ano[np.array(idx_test)]
    epochs, aucs, aps, losses = [], [], [], []
    for epoch in range(num_epoch):
        model.train()
        opt.zero_grad()
        loss, score = model(features, adj, normal_idx, idx_test)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        if epoch % 5 == 0:
            sc = _np(score)
            epochs.append(epoch)
            aucs.append(roc_auc_score(yt, sc))
            aps.append(average_precision_score(yt, sc, average="macro", pos_label=1, sample_weight=None))
    print("planted auc", aucs[0], "->", aucs[-1], "ap", aps[0], "->", aps[-1])
    return dict(n=n, f=f, n_h=n_h, seed=seed, lr=lr, num_epoch=num_epoch, rowptr=rowptr, col=col, feat_raw=feat, ano=ano,
                features=_np(features[0]), idx_test=np.array(idx_test), normal_idx=np.array(normal_idx),
                eval_epochs=np.array(epochs), auc=np.array(aucs), ap=np.array(aps), losses=np.array(losses))


def main():
    if not os.path.isdir(REF):
        sys.exit("reference tree not present; the fixtures can only be regenerated where it is")
    _stub_modules()
    sys.path.insert(0, REF)
    torch.set_num_threads(4)
    out = {"cases": np.array(["a", "b"])}
    out.update(model_case("a", n=301, n_entries=2400, f=10, n_h=64, seed=1, k_steps=5, lr=5e-4, self_loop_frac=0.0, isolated=False))
    out.update(model_case("b", n=293, n_entries=2600, f=93, n_h=48, seed=3, k_steps=5, lr=1e-3, self_loop_frac=0.1, isolated=True))
    np.savez_compressed(os.path.join(HERE, "fullgraph_anomalydae.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "fullgraph_anomalydae_planted.npz"), **planted_case())


if __name__ == "__main__":
    main()
