#!/usr/bin/env python3
"""Generate the full-graph DOMINANT fixtures from the *imported* reference `model_domaint.py`.

Runs only where the reference tree is present (see make_golden.py).  The reference imports `torch_geometric.nn.GCN`; it is stubbed
by `PygGCN` below (built on `PygLinear` of make_golden_anomalydae.py), `dgl` is stubbed empty, `.cuda()` is an identity and
everything runs on the CPU.  `dominant.py` has no `__main__` guard and needs dgl and a dataset file, so its training loop is
restated here line by line.  Inputs come from `ggad_amd.synth`; the fixtures are data.

    python tests/golden/make_golden_dominant.py     # writes tests/golden/fullgraph_dominant{,_planted}.npz
"""
from __future__ import annotations

import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from make_golden_aegis import _np, _split  # noqa: E402
from make_golden_anomalydae import PygLinear  # noqa: E402
from make_golden_gaan import _inputs  # noqa: E402


class PygGCNConv(nn.Module):
    """torch_geometric 2.1.0 `GCNConv(in_channels, out_channels)` with every default, restated.  Assumptions:

    - improved = False, cached = False, add_self_loops = True, normalize = True, bias = True, aggr = 'add';
    - `lin` = Linear(in, out, bias=False, weight_initializer='glorot') draws its weight in its own constructor; `bias` (out,) is
      registered after it; then `reset_parameters()` draws lin's weight AGAIN and zeroes the bias (two draws per conv).  state_dict
      order: `bias`, then `lin.weight`;
    - forward(x, edge_index) with edge_weight None: gcn_norm gives every edge weight 1, `add_remaining_self_loops` keeps the loops
      present (weight 1) and adds one (weight 1) on every node without one; deg = scatter-add of the weights at the TARGET
      edge_index[1]; norm_e = deg[src]^-1/2 w_e deg[dst]^-1/2 (inf -> 0);
    - x = lin(x); out[dst] += norm_e x[src] over the edges (source edge_index[0] -> target edge_index[1]); out + bias.
    """

    def __init__(self, in_channels, out_channels, **kwargs):
        super().__init__()
        if kwargs:
            raise ValueError("the stub restates the defaults only")
        self.lin = PygLinear(in_channels, out_channels)
        self.bias = nn.Parameter(torch.empty(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        self.lin.reset_parameters()
        self.bias.data.zero_()

    def forward(self, x, edge_index):
        n = x.shape[0]
        src, dst = edge_index[0], edge_index[1]
        loops = src == dst
        has = torch.zeros(n, dtype=torch.bool)
        has[src[loops]] = True
        add = torch.arange(n)[~has]
        src, dst = torch.cat([src, add]), torch.cat([dst, add])
        w = torch.ones(src.numel(), dtype=x.dtype)
        deg = torch.zeros(n, dtype=x.dtype).scatter_add_(0, dst, w)
        dis = deg.pow(-0.5)
        dis.masked_fill_(dis == float("inf"), 0)
        norm = dis[src] * w * dis[dst]
        x = self.lin(x)
        out = torch.zeros_like(x).index_add_(0, dst, norm.view(-1, 1) * x[src])
        return out + self.bias


class PygGCN(nn.Module):
    """torch_geometric 2.1.0 `GCN(in_channels, hidden_channels, num_layers)` (BasicGNN) with out_channels None, dropout 0, act ReLU,
    no norm, no jk: convs = [GCNConv(in, hidden)] + [GCNConv(hidden, hidden)] * (num_layers - 1), ReLU after every conv but the
    last; dropout 0 draws nothing."""

    def __init__(self, in_channels, hidden_channels, num_layers, **kwargs):
        super().__init__()
        if kwargs:
            raise ValueError("the stub restates the defaults only")
        self.convs = nn.ModuleList([PygGCNConv(in_channels if k == 0 else hidden_channels, hidden_channels) for k in range(num_layers)])

    def forward(self, x, edge_index):
        for k, conv in enumerate(self.convs):
            x = conv(x, edge_index)
            if k < len(self.convs) - 1:
                x = torch.relu(x)
        return x


def dense_gcn_operator(adj):
    """float64 D^-1/2 P^T D^-1/2 of the dense A_hat: P = [adj > 0] with its diagonal set, D = diag(column sums of P)."""
    a = np.asarray(adj, dtype=np.float32)
    P = (a > 0).astype(np.float64)
    np.fill_diagonal(P, 1.0)
    deg = P.sum(0)
    dis = np.where(deg > 0, deg ** -0.5, 0.0)
    return dis[:, None] * P.T * dis[None, :]


def _stub_modules():
    sys.modules["dgl"] = types.ModuleType("dgl")
    tg = types.ModuleType("torch_geometric")
    tgnn = types.ModuleType("torch_geometric.nn")
    tgnn.GCN = PygGCN
    tg.nn = tgnn
    sys.modules["torch_geometric"] = tg
    sys.modules["torch_geometric.nn"] = tgnn
    torch.Tensor.cuda = lambda self, *a, **k: self                # the reference moves edge_index with .cuda()


def _checks():
    """The two facts the model relies on, checked with this torch: F.dropout(x, 0.0) draws nothing from the CPU generator, and the
    restated GCNConv draws its weight twice (the constructor's draw, then reset_parameters')."""
    torch.manual_seed(0)
    s0 = torch.get_rng_state()
    torch.nn.functional.dropout(torch.ones(5, 3), 0.0)
    assert torch.equal(s0, torch.get_rng_state()), "F.dropout(p=0) consumed the RNG"
    torch.manual_seed(0)
    conv = PygGCNConv(7, 5)
    torch.manual_seed(0)
    a = (6.0 / 12) ** 0.5
    first = torch.empty(5, 7).uniform_(-a, a)
    second = torch.empty(5, 7).uniform_(-a, a)
    assert torch.equal(conv.lin.weight.data, second) and not torch.equal(first, second)
    assert list(dict(conv.state_dict())) == ["bias", "lin.weight"]


def _pyg_vs_dense(adj, seed):
    """PygGCNConv on the reference's edge list equals the dense float64 operator (float64 throughout)."""
    from model_domaint import neighList_to_edgeList
    a = torch.as_tensor(adj, dtype=torch.float32)
    ei = torch.tensor(np.array(neighList_to_edgeList(a))).T
    torch.manual_seed(seed)
    conv = PygGCNConv(6, 4).double()
    x = torch.randn(a.shape[0], 6, dtype=torch.float64)
    with torch.no_grad():
        conv.bias.normal_()
        got = conv(x, ei).numpy()
        ref = dense_gcn_operator(adj) @ (x @ conv.lin.weight.T).numpy() + conv.bias.numpy()
    err = np.abs(got - ref).max()
    assert err < 1e-12, err
    return err


def _sparse(name, m):
    """A dense float64 matrix stored as its nonzero entries (row, col, value), row-major order."""
    r, c = np.nonzero(m)
    return {name + "_row": r.astype(np.int32), name + "_col": c.astype(np.int32), name + "_val": m[r, c]}


def _prep(rowptr, col, feat, n, rutils):
    """dominant.py:82-96 on the Amazon branch: features row-normalised, adj = normalize_adj(adj) + I dense."""
    adj_sp = synth_csr(rowptr, col, n)
    feats_dense, _ = rutils.preprocess_features(sp.lil_matrix(feat))
    adj = np.asarray((rutils.normalize_adj(adj_sp) + sp.eye(n)).todense())
    return torch.FloatTensor(np.asarray(feats_dense)[np.newaxis]), torch.FloatTensor(adj[np.newaxis])


def synth_csr(rowptr, col, n):
    from ggad_amd import synth
    return synth.csr_to_scipy(rowptr, col, n)


def _state(model, prefix, out, trained_only=False):
    """state_dict into `out`; trained_only: the autoencoder's tensors alone (dense_stru, gat_layer and disc never get a gradient,
    so Adam leaves them at their initial values)."""
    for k, v in model.state_dict().items():
        if not trained_only or k.startswith("dense_attr_"):
            out[prefix + k] = _np(v).copy()


def model_case(tag, n, n_entries, f, n_h, seed, lr, epochs=5):
    from model_domaint import Model                                 # /root/reference/model_domaint.py
    import utils as rutils                                          # /root/reference/utils.py
    rowptr, col, feat, ano = _inputs(tag, n, n_entries, f, seed)
    normal, idx_test = _split(n, ano, seed)[1:]
    features, adj = _prep(rowptr, col, feat, n, rutils)
    out = {f"{tag}.{k}": v for k, v in dict(n=n, f=f, n_h=n_h, seed=seed, lr=lr, rowptr=rowptr, col=col, ano=ano,
                                             features=_np(features[0]), idx_train=np.array(normal), idx_test=np.array(idx_test),
                                             **_sparse("gcn_op", dense_gcn_operator(_np(adj[0]))),
                                             pyg_vs_dense=_pyg_vs_dense(_np(adj[0]), seed)).items()}
    torch.manual_seed(seed)
    model = Model(f, n_h, "prelu", 1, "avg")
    _state(model, f"{tag}.init.", out)
    optimiser = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0.0)
    model.train()
    optimiser.zero_grad()
    loss, score = model(features, adj, normal, idx_test)
    loss.backward()
    out.update({f"{tag}.emb": _np(model.emb), f"{tag}.loss0": np.float64(loss.item()), f"{tag}.score0": _np(score)})
    for k, p in model.named_parameters():
        if p.grad is not None:
            out[f"{tag}.grad.{k}"] = _np(p.grad).copy()
    optimiser.step()
    _state(model, f"{tag}.step1.", out, trained_only=True)

    torch.manual_seed(seed)                                          # the script's loop (dominant.py:121-150)
    model = Model(f, n_h, "prelu", 1, "avg")
    optimiser = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0.0)
    losses, scores = [], []
    for epoch in range(epochs):
        model.train()
        optimiser.zero_grad()
        loss, score = model(features, adj, normal, idx_test)
        loss.backward()
        optimiser.step()
        losses.append(loss.item())
        scores.append(_np(score))
        if epoch % 5 == 0:
            model.eval()
    out[f"{tag}.traj_loss"] = np.array(losses, dtype=np.float64)
    out[f"{tag}.traj_score"] = np.stack(scores)
    for k, v in model.state_dict().items():
        if not k.startswith("dense_attr_"):
            assert np.array_equal(_np(v), out[f"{tag}.init.{k}"]), k
    _state(model, f"{tag}.final.", out, trained_only=True)
    print(tag, "rows", len(normal), len(idx_test), "loss", losses)
    return out


def planted_case(n=600, n_entries=5000, f=32, n_h=64, seed=2, num_epoch=50, lr=3e-3, self_sensitivity=1e-7):
    """The restated loop of dominant.py on planted anomalies: AUROC / AP of the epoch's test scores every 5 epochs."""
    from model_domaint import Model
    import utils as rutils
    from sklearn.metrics import average_precision_score, roc_auc_score
    rowptr, col, feat, ano = _inputs("a", n, n_entries, f, seed, planted=dict(scale=0.25, rewire=0.5))
    normal, idx_test = _split(n, ano, seed)[1:]
    features, adj = _prep(rowptr, col, feat, n, rutils)
    yt = ano[np.array(idx_test)]

    def train(perturb=0.0):
        torch.manual_seed(seed)
        model = Model(f, n_h, "prelu", 1, "avg")
        if perturb:
            g = torch.Generator().manual_seed(12345)
            with torch.no_grad():
                for p in model.parameters():
                    p.mul_(1 + perturb * torch.randn(p.shape, generator=g))
        optimiser = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0.0)
        epochs, aucs, aps, losses = [], [], [], []
        for epoch in range(num_epoch):
            model.train()
            optimiser.zero_grad()
            loss, score = model(features, adj, normal, idx_test)
            loss.backward()
            optimiser.step()
            losses.append(loss.item())
            if epoch % 5 == 0:
                sc = _np(score)
                epochs.append(epoch)
                aucs.append(roc_auc_score(yt, sc))
                aps.append(average_precision_score(yt, sc, average="macro", pos_label=1, sample_weight=None))
                model.eval()
        return np.array(epochs), np.array(aucs), np.array(aps), np.array(losses, dtype=np.float64)

    epochs, aucs, aps, losses = train()
    out = dict(n=n, f=f, n_h=n_h, seed=seed, lr=lr, num_epoch=num_epoch, rowptr=rowptr, col=col, ano=ano, features=_np(features[0]),
               idx_train=np.array(normal), idx_test=np.array(idx_test), eval_epochs=epochs, auc=aucs, ap=aps, losses=losses)
    _, aucs2, aps2, _ = train(perturb=self_sensitivity)
    out.update(self_sens_perturb=np.float64(self_sensitivity), self_sens_auc=np.abs(aucs2 - aucs), self_sens_ap=np.abs(aps2 - aps))
    print("planted auc", aucs, "ap", aps)
    print("self-sensitivity auc", np.abs(aucs2 - aucs).max(), "ap", np.abs(aps2 - aps).max())
    return out


def main():
    if not os.path.isdir(REF):
        sys.exit("reference tree not present; the fixtures can only be regenerated where it is")
    _stub_modules()
    _checks()
    sys.path.insert(0, REF)
    torch.set_num_threads(4)
    out = {"cases": np.array(["a", "b"])}
    out.update(model_case("a", n=301, n_entries=2400, f=64, n_h=48, seed=1, lr=1e-3))
    out.update(model_case("b", n=211, n_entries=2600, f=129, n_h=24, seed=3, lr=5e-4))
    np.savez_compressed(os.path.join(HERE, "fullgraph_dominant.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "fullgraph_dominant_planted.npz"), **planted_case())


if __name__ == "__main__":
    main()
