#!/usr/bin/env python3
"""Generate the full-graph GAAN fixtures from the *imported* reference `model_gaan.py`.

Runs only where the reference tree is present (see make_golden.py).  The reference imports `torch_geometric.nn.MLP`; it is stubbed
by `PygMLP` of make_golden_aegis.py (imported, not restated), `dgl` is stubbed empty, and everything runs on the CPU.  `gaan.py` has
no `__main__` guard and needs dgl and a dataset file, so its training loop is restated here line by line.  Inputs come from
`ggad_amd.synth`; the fixtures are data.

    python tests/golden/make_golden_gaan.py        # writes tests/golden/fullgraph_gaan{,_planted}.npz
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402
import torch  # noqa: E402

from ggad_amd import synth  # noqa: E402
from make_golden_aegis import _np, _split, _stub_modules  # noqa: E402  (PygMLP comes in through _stub_modules)


def _inputs(tag, n, n_entries, f, seed, planted=None):
    """(rowptr, col, feat, ano) of the raw adjacency.  Graph 'b': raw self loops, an isolated node (n - 1), a node whose only entry
    is its self loop (n - 2), and an asymmetric adjacency: node n - 3 keeps its in-entries but loses its out-entries (the normalised
    entries of its column are then stored zeros of normalize_adj's CSR), and a tenth of the remaining upper-triangle entries go."""
    rowptr, col = synth.make_graph(n, n_entries, seed, kind="powerlaw", max_degree=n // 4, self_loop_frac=0.1 if tag == "b" else 0.0)
    feat = synth.make_features(n, f, seed)
    ano = synth.make_labels(n, 0.1, seed)
    if planted:
        rowptr, col, feat = synth.plant_anomalies(rowptr, col, feat, ano, seed, **planted)
    if tag == "b":
        a = synth.csr_to_scipy(rowptr, col, n).tolil()
        for k in (n - 1, n - 2):
            a[k, :] = 0
            a[:, k] = 0
        a[n - 2, n - 2] = 1
        a[n - 3, :] = 0
        a = sp.csr_matrix(a)
        a.eliminate_zeros()
        coo = a.tocoo()
        rng = np.random.default_rng(seed)
        drop = (coo.row < coo.col) & (rng.random(coo.nnz) < 0.1)
        a = sp.csr_matrix((coo.data[~drop], (coo.row[~drop], coo.col[~drop])), shape=(n, n))
        a.sort_indices()
        rowptr, col = a.indptr.astype(np.int64), a.indices.astype(np.int64)
    return rowptr, col, feat, ano


def _prep(rowptr, col, feat, n, rutils):
    """gaan.py:77-95: features row-normalised (Amazon's branch), adj = normalize_adj(adj) + I dense."""
    adj_sp = synth.csr_to_scipy(rowptr, col, n)
    feats_dense, _ = rutils.preprocess_features(sp.lil_matrix(feat))
    adj = np.asarray((rutils.normalize_adj(adj_sp) + sp.eye(n)).todense())
    return torch.FloatTensor(np.asarray(feats_dense)[np.newaxis]), torch.FloatTensor(adj[np.newaxis])


class _Hooks:
    """Last noise and output of the generator, and the discriminator's two outputs (x first, then x_)."""

    def __init__(self, model):
        self.out = {}

        def gen(m, i, o):
            self.out["noise"] = i[0].detach().clone()
            self.out["x_"] = o.detach().clone()
        model.generator.register_forward_hook(gen)
        model.discriminator.register_forward_hook(lambda m, i, o: self.out.setdefault("dis", []).append(o.detach().clone()))


def _state(model, prefix, out, unused_too=False):
    for k, v in model.state_dict().items():
        if unused_too or not k.startswith("disc."):
            out[prefix + k] = _np(v).copy()


def _bn_buffers(model):
    return {k: _np(v).copy() for k, v in model.state_dict().items() if ".norms." in k and ("running" in k or "num_batches" in k)}


def model_case(tag, n, n_entries, f, n_h, seed, lr, subset, epochs=5):
    from model_gaan import Model, neighList_to_edgeList_train      # /root/reference/model_gaan.py
    import utils as rutils                                          # /root/reference/utils.py
    rowptr, col, feat, ano = _inputs(tag, n, n_entries, f, seed)
    all_idx, _, idx_test = _split(n, ano, seed)
    idx_train = all_idx[: int(0.7 * n)] if subset else all_idx          # 'b': a proper subset of the nodes as the row list
    features, adj = _prep(rowptr, col, feat, n, rutils)
    edges = np.array(neighList_to_edgeList_train(torch.squeeze(adj), idx_train))
    out = {f"{tag}.{k}": v for k, v in dict(n=n, f=f, n_h=n_h, seed=seed, lr=lr, rowptr=rowptr, col=col, ano=ano,
                                             features=_np(features[0]), idx_train=np.array(idx_train), idx_test=np.array(idx_test),
                                             edges=edges.astype(np.int64)).items()}

    # (1) one epoch from the initial state: forward values, every gradient after both backward calls, the state after both steps
    torch.manual_seed(seed)
    model = Model(f, n_h, "prelu", 1, "avg")
    _state(model, f"{tag}.init.", out, unused_too=True)
    hooks = _Hooks(model)
    optimiser = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0.0)
    optimiser_gen = torch.optim.Adam(model.generator.parameters(), lr=lr)
    model.train()
    optimiser.zero_grad()
    optimiser_gen.zero_grad()
    loss, loss_g, score = model(features, adj, idx_train, idx_test)
    # the two loss parts, recomputed from the model's own dense matrices exactly as loss_func_ed builds them
    a = torch.sigmoid(model.emb @ model.emb.T)
    a_ = torch.sigmoid(hooks.out["dis"][1] @ hooks.out["dis"][1].T)
    loss_r = torch.nn.functional.binary_cross_entropy(a[edges[:, 0], edges[:, 1]], torch.ones(len(edges)))
    loss_f = torch.nn.functional.binary_cross_entropy(a_[edges[:, 0], edges[:, 1]], torch.zeros(len(edges)))
    loss.backward()
    loss_g.backward()
    out.update({f"{tag}.noise0": _np(hooks.out["noise"]), f"{tag}.x_": _np(hooks.out["x_"]), f"{tag}.emb": _np(hooks.out["dis"][0]),
                f"{tag}.z_": _np(hooks.out["dis"][1]), f"{tag}.m": np.int64(len(edges)), f"{tag}.loss0": np.float64(loss.item()),
                f"{tag}.loss_r0": np.float64(loss_r.item()), f"{tag}.loss_f0": np.float64(loss_f.item()),
                f"{tag}.loss_g0": np.float64(loss_g.item()), f"{tag}.score0": _np(score)})
    for k, p in model.named_parameters():
        if p.grad is not None:
            out[f"{tag}.grad.{k}"] = _np(p.grad).copy()
    optimiser.step()
    optimiser_gen.step()
    _state(model, f"{tag}.step1.", out)

    # (2) the script's loop (gaan.py:119-140) for `epochs` epochs
    torch.manual_seed(seed)
    model = Model(f, n_h, "prelu", 1, "avg")
    optimiser = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0.0)
    optimiser_gen = torch.optim.Adam(model.generator.parameters(), lr=lr)
    losses, losses_g, scores, bufs = [], [], [], {}
    for epoch in range(epochs):
        model.train()
        optimiser.zero_grad()
        optimiser_gen.zero_grad()
        loss, loss_g, score = model(features, adj, idx_train, idx_test)
        loss.backward()
        loss_g.backward()
        optimiser.step()
        optimiser_gen.step()
        losses.append(loss.item())
        losses_g.append(loss_g.item())
        scores.append(_np(score))
        for k, v in _bn_buffers(model).items():
            bufs.setdefault(k, []).append(v)
        if epoch % 5 == 0:
            model.eval()
    out[f"{tag}.traj_loss"] = np.array(losses, dtype=np.float64)
    out[f"{tag}.traj_loss_g"] = np.array(losses_g, dtype=np.float64)
    out[f"{tag}.traj_score"] = np.stack(scores)
    for k, v in bufs.items():
        out[f"{tag}.traj_buf.{k}"] = np.stack(v)
    _state(model, f"{tag}.final.", out)
    print(tag, "m", len(edges), "loss", losses, "loss_g", losses_g)
    return out


def planted_case(n=600, n_entries=5000, f=32, n_h=64, seed=2, num_epoch=40, lr=1e-3, self_sensitivity=1e-7):
    """The restated loop of gaan.py on planted anomalies: AUROC / AP of the epoch's test scores every 5 epochs."""
    from model_gaan import Model
    import utils as rutils
    from sklearn.metrics import average_precision_score, roc_auc_score
    rowptr, col, feat, ano = _inputs("a", n, n_entries, f, seed, planted=dict(scale=0.25, rewire=0.5))
    all_idx, _, idx_test = _split(n, ano, seed)
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
        optimiser_gen = torch.optim.Adam(model.generator.parameters(), lr=lr)
        epochs, aucs, aps, losses = [], [], [], []
        for epoch in range(num_epoch):
            model.train()
            optimiser.zero_grad()
            optimiser_gen.zero_grad()
            loss, loss_g, score = model(features, adj, all_idx, idx_test)
            loss.backward()
            loss_g.backward()
            optimiser.step()
            optimiser_gen.step()
            losses.append([loss.item(), loss_g.item()])
            if epoch % 5 == 0:
                sc = _np(score)
                epochs.append(epoch)
                aucs.append(roc_auc_score(yt, sc))
                aps.append(average_precision_score(yt, sc, average="macro", pos_label=1, sample_weight=None))
                model.eval()
        return np.array(epochs), np.array(aucs), np.array(aps), np.array(losses, dtype=np.float64)

    epochs, aucs, aps, losses = train()
    out = dict(n=n, f=f, n_h=n_h, seed=seed, lr=lr, num_epoch=num_epoch, rowptr=rowptr, col=col, ano=ano, features=_np(features[0]),
               all_idx=np.array(all_idx), idx_test=np.array(idx_test), eval_epochs=epochs, auc=aucs, ap=aps, losses=losses)
    _, aucs2, aps2, losses2 = train(perturb=self_sensitivity)
    out.update(self_sens_perturb=np.float64(self_sensitivity), self_sens_auc=np.abs(aucs2 - aucs), self_sens_ap=np.abs(aps2 - aps),
               self_sens_loss=np.abs(losses2 - losses).max(axis=1))
    print("planted auc", aucs, "ap", aps)
    print("self-sensitivity auc", np.abs(aucs2 - aucs).max(), "ap", np.abs(aps2 - aps).max())
    return out


def main():
    if not os.path.isdir(REF):
        sys.exit("reference tree not present; the fixtures can only be regenerated where it is")
    _stub_modules()
    sys.path.insert(0, REF)
    torch.set_num_threads(4)
    out = {"cases": np.array(["a", "b"])}
    out.update(model_case("a", n=301, n_entries=2400, f=10, n_h=32, seed=1, lr=1e-3, subset=False))
    out.update(model_case("b", n=211, n_entries=2600, f=93, n_h=24, seed=3, lr=5e-4, subset=True))
    np.savez_compressed(os.path.join(HERE, "fullgraph_gaan.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "fullgraph_gaan_planted.npz"), **planted_case())


if __name__ == "__main__":
    main()
