#!/usr/bin/env python3
"""Generate the full-graph AEGIS fixtures from the *imported* reference `model_AEGIS.py`.

Runs only where the reference tree is present (see make_golden.py).  The reference imports `torch_geometric.nn.MLP`; it is stubbed
by `PygMLP` below, a pure-torch restatement that makes the same draws and carries the same names as `ggad_amd.graphsage_aegis.MLP`
(the stack of torch_geometric 2.1's MLP for the arguments the reference passes).  `dgl` is stubbed empty and `.cuda()` is made an
identity, so everything runs on the CPU.  `aegis.py` has no `__main__` guard and needs dgl and a dataset file, so its training loop is
restated here line by line.  Inputs come from `ggad_amd.synth`; the fixtures are data.

    python tests/golden/make_golden_aegis.py        # writes tests/golden/fullgraph_aegis{,_planted}.npz
"""
from __future__ import annotations

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
import torch.nn.functional as F  # noqa: E402

from ggad_amd import synth  # noqa: E402


class _Norm(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.module = nn.BatchNorm1d(c)

    def forward(self, x):
        return self.module(x)


class PygMLP(nn.Module):
    """torch_geometric.nn.MLP (2.1) for in/hidden/out_channels, num_layers, dropout = 0 and a callable act, every other argument at
    its default (batch_norm, act_first = False, plain_last = True, bias): [Linear -> BatchNorm1d -> act] x (L - 1) -> Linear.  The
    Linear layers draw as torch.nn.Linear does (kaiming-uniform, a = sqrt(5), bias U(+-1/sqrt(fan_in))), one layer after the other."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers, dropout=0.0, act=F.relu, **kwargs):
        super().__init__()
        chans = [in_channels] + [hidden_channels] * (num_layers - 1) + [out_channels]
        self.lins = nn.ModuleList([nn.Linear(a, b) for a, b in zip(chans[:-1], chans[1:])])
        self.norms = nn.ModuleList([_Norm(c) for c in chans[1:-1]])
        self.dropout = float(dropout)
        self.act = act

    def forward(self, x):
        for lin, norm in zip(self.lins[:-1], self.norms):
            x = self.act(norm(lin(x)))
            x = F.dropout(x, p=self.dropout, training=self.training)
        return self.lins[-1](x)


def _stub_modules():
    sys.modules["dgl"] = types.ModuleType("dgl")
    tg = types.ModuleType("torch_geometric")
    tgnn = types.ModuleType("torch_geometric.nn")
    tgnn.MLP = PygMLP
    tg.nn = tgnn
    sys.modules["torch_geometric"] = tg
    sys.modules["torch_geometric.nn"] = tgnn
    torch.Tensor.cuda = lambda self, *a, **k: self                # the reference moves noise and labels with .cuda()


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _inputs(n, n_entries, f, seed, self_loop_frac, isolated, planted=None):
    rowptr, col = synth.make_graph(n, n_entries, seed, kind="powerlaw", max_degree=n // 4, self_loop_frac=self_loop_frac)
    feat = synth.make_features(n, f, seed)
    ano = synth.make_labels(n, 0.1, seed)
    if planted:
        rowptr, col, feat = synth.plant_anomalies(rowptr, col, feat, ano, seed, **planted)
    if isolated:
        # the last node loses all its entries; the one before keeps only a raw self loop
        import scipy.sparse as sp
        a = synth.csr_to_scipy(rowptr, col, n).tolil()
        a[n - 1, :] = 0
        a[:, n - 1] = 0
        a[n - 2, :] = 0
        a[:, n - 2] = 0
        a[n - 2, n - 2] = 1
        a = sp.csr_matrix(a)
        a.eliminate_zeros()
        rowptr, col = a.indptr.astype(np.int64), a.indices.astype(np.int64)
    return rowptr, col, feat, ano


def _split(n, ano, seed):
    """all_idx (the shuffled permutation load_mat returns), normal_label_idx and idx_test as `utils.load_mat` draws them."""
    random.seed(seed)
    all_idx = list(range(n))
    random.shuffle(all_idx)
    idx_train, idx_test = all_idx[:int(n * 0.3)], all_idx[int(n * 0.3) + int(n * 0.1):]
    normal = [i for i in idx_train if ano[i] == 0]
    normal = normal[:int(len(normal) * 0.8)]
    return all_idx, normal, idx_test


def _prep(rowptr, col, feat, n, rutils):
    import scipy.sparse as sp
    adj_sp = synth.csr_to_scipy(rowptr, col, n)
    feats_dense, _ = rutils.preprocess_features(sp.lil_matrix(feat))                # aegis.py:77-78
    adj = rutils.normalize_adj(adj_sp)                                               # :86
    raw = np.asarray((adj_sp + sp.eye(n)).todense())                                 # :89
    adj = np.asarray((adj + sp.eye(n)).todense())                                    # :90
    return (torch.FloatTensor(np.asarray(feats_dense)[np.newaxis]), torch.FloatTensor(adj[np.newaxis]),
            torch.FloatTensor(raw[np.newaxis]))


def _affinity(emb_all, raw_adj, n):
    """aegis.py:126-146 as written."""
    emb_inf = torch.pow(torch.norm(emb_all, dim=-1, keepdim=True), -1)
    emb_inf[torch.isinf(emb_inf)] = 0.
    emb_norm = emb_all * emb_inf
    sim = torch.mm(emb_norm, emb_norm.T)
    raw = torch.squeeze(raw_adj)
    s1 = sim[:n, :n] * raw
    s2 = sim[n:, n:] * raw
    r_inv = torch.pow(torch.sum(raw, 0), -1)
    r_inv[torch.isinf(r_inv)] = 0.
    return torch.sum(s1, 0) * r_inv, torch.sum(s2, 0) * r_inv


def draw_arrays(affinity1, affinity2, all_idx, ano_label):
    """The three arrays aegis.py:155-166 hands to draw_pdf_methods (the anomalous set is np.array(all_idx)[argwhere(ano == 1)]: a
    reference quirk, kept)."""
    real_abn = np.array(all_idx)[np.argwhere(ano_label == 1).squeeze()].tolist()
    real_nrm = np.array(all_idx)[np.argwhere(ano_label == 0).squeeze()].tolist()
    ra, _ = torch.sort(torch.as_tensor(np.asarray(affinity1))[real_abn])
    return np.asarray(affinity1)[real_nrm], np.asarray(affinity2)[:500], _np(ra[:50])


class _Hooks:
    """Last outputs of the generator, gcn_enc2 (called on x_gen, then on x) and gcn_dec2."""

    def __init__(self, model):
        self.out = {}
        model.generator.register_forward_hook(lambda m, i, o: self.out.__setitem__("x_gen", o.detach().clone()))
        model.gcn_enc2.register_forward_hook(lambda m, i, o: self.out.setdefault("enc2", []).append(o.detach().clone()))
        model.gcn_dec2.register_forward_hook(lambda m, i, o: self.out.__setitem__("z_dec", o.detach().clone()))


def _state(model, prefix, out, unused_too=False):
    """state_dict under `prefix`; the unused disc / discriminator (which never change) only with unused_too."""
    for k, v in model.state_dict().items():
        if unused_too or not k.startswith(("disc.", "discriminator.")):
            out[prefix + k] = _np(v).copy()


def model_case(tag, n, n_entries, f, n_h, seed, lr, self_loop_frac, isolated, main_epochs=5, recon_epochs=10):
    from model_AEGIS import Model             # /root/reference/model_AEGIS.py
    import utils as rutils                    # /root/reference/utils.py
    rowptr, col, feat, ano = _inputs(n, n_entries, f, seed, self_loop_frac, isolated)
    all_idx, normal_idx, idx_test = _split(n, ano, seed)
    features, adj, raw_adj = _prep(rowptr, col, feat, n, rutils)
    out = {f"{tag}.{k}": v for k, v in dict(n=n, f=f, n_h=n_h, seed=seed, lr=lr, rowptr=rowptr, col=col, ano=ano,
                                             features=_np(features[0]), all_idx=np.array(all_idx), idx_test=np.array(idx_test),
                                             normal_idx=np.array(normal_idx)).items()}

    # (1) one main-loop epoch from the initial state: forward values, every gradient, the state after both optimisers
    torch.manual_seed(seed)
    model = Model(f, n_h, "prelu", 1, "avg")
    _state(model, f"{tag}.init.", out, unused_too=True)
    hooks = _Hooks(model)
    optimiser = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0.0)
    optimiser_gen = torch.optim.Adam(model.generator.parameters(), lr=lr)
    model.train()
    optimiser.zero_grad()
    optimiser_gen.zero_grad()
    loss_dis, loss_g, loss_ae, score, emb_all = model(features, adj, all_idx, idx_test)
    loss_g.backward(retain_graph=True)
    loss_dis.backward(retain_graph=True)
    out.update({f"{tag}.x_gen": _np(hooks.out["x_gen"]), f"{tag}.z_gen": _np(hooks.out["enc2"][0]), f"{tag}.z": _np(hooks.out["enc2"][1]),
                f"{tag}.z_dec": _np(hooks.out["z_dec"]), f"{tag}.loss_ae0": np.float64(loss_ae.item()),
                f"{tag}.loss_g0": np.float64(loss_g.item()), f"{tag}.score0": _np(score)})
    for k, p in model.named_parameters():
        if p.grad is not None:
            out[f"{tag}.grad.{k}"] = _np(p.grad).copy()
    optimiser.step()
    optimiser_gen.step()
    _state(model, f"{tag}.step1.", out)
    a1, a2 = _affinity(emb_all.detach(), raw_adj, n)
    out[f"{tag}.affinity1_0"], out[f"{tag}.affinity2_0"] = _np(a1), _np(a2)
    for i, arr in enumerate(draw_arrays(_np(a1), _np(a2), all_idx, ano)):
        out[f"{tag}.draw{i}_0"] = arr

    # (2) the script's schedule (aegis.py:116-172): recon_epochs pre-training epochs with accumulating gradients, then main epochs
    torch.manual_seed(seed)
    model = Model(f, n_h, "prelu", 1, "avg")
    optimiser_ae = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0.0)
    optimiser = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0.0)
    optimiser_gen = torch.optim.Adam(model.generator.parameters(), lr=lr)
    pre = []
    for epoch in range(recon_epochs):
        loss_dis, loss_g, loss_ae, score, emb_all = model(features, adj, normal_idx, idx_test)
        loss_ae.backward()
        optimiser_ae.step()
        pre.append(loss_ae.item())
    out[f"{tag}.pre_losses"] = np.array(pre, dtype=np.float64)
    for k, p in model.named_parameters():
        if p.grad is not None:
            out[f"{tag}.pre_grad.{k}"] = _np(p.grad).copy()
    l_ae, l_g, scores = [], [], []
    for epoch in range(main_epochs):
        model.train()
        optimiser.zero_grad()
        optimiser_gen.zero_grad()
        loss_dis, loss_g, loss_ae, score, emb_all = model(features, adj, all_idx, idx_test)
        loss_g.backward(retain_graph=True)
        loss_dis.backward(retain_graph=True)
        optimiser.step()
        optimiser_gen.step()
        l_ae.append(loss_dis.item())
        l_g.append(loss_g.item())
        scores.append(_np(score)[:, 0])
        if epoch % 5 == 0:
            model.eval()
    out[f"{tag}.main_loss_ae"] = np.array(l_ae, dtype=np.float64)
    out[f"{tag}.main_loss_g"] = np.array(l_g, dtype=np.float64)
    out[f"{tag}.main_scores"] = np.stack(scores)
    _state(model, f"{tag}.final.", out)
    print(tag, "pre", pre[0], "->", pre[-1], "main ae", l_ae, "g", l_g)
    return out


def planted_case(n=600, n_entries=5000, f=32, n_h=64, seed=2, num_epoch=40, recon_epochs=10, lr=1e-3, self_sensitivity=1e-7):
    """The restated loop of aegis.py on planted anomalies: AUROC / AP of the epoch's test scores every 5 main epochs."""
    from model_AEGIS import Model
    import utils as rutils
    from sklearn.metrics import average_precision_score, roc_auc_score
    rowptr, col, feat, ano = _inputs(n, n_entries, f, seed, 0.0, False, planted=dict(scale=0.25, rewire=0.5))
    all_idx, normal_idx, idx_test = _split(n, ano, seed)
    features, adj, _ = _prep(rowptr, col, feat, n, rutils)
    yt = ano[np.array(idx_test)]

    def train(perturb=0.0):
        torch.manual_seed(seed)
        model = Model(f, n_h, "prelu", 1, "avg")
        if perturb:
            g = torch.Generator().manual_seed(12345)
            with torch.no_grad():
                for p in model.parameters():
                    p.mul_(1 + perturb * torch.randn(p.shape, generator=g))
        optimiser_ae = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0.0)
        optimiser = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=0.0)
        optimiser_gen = torch.optim.Adam(model.generator.parameters(), lr=lr)
        for epoch in range(recon_epochs):
            loss_dis, loss_g, loss_ae, score, emb_all = model(features, adj, normal_idx, idx_test)
            loss_ae.backward()
            optimiser_ae.step()
        epochs, aucs, aps, losses = [], [], [], []
        for epoch in range(num_epoch):
            model.train()
            optimiser.zero_grad()
            optimiser_gen.zero_grad()
            loss_dis, loss_g, loss_ae, score, emb_all = model(features, adj, all_idx, idx_test)
            loss_g.backward(retain_graph=True)
            loss_dis.backward(retain_graph=True)
            optimiser.step()
            optimiser_gen.step()
            losses.append([loss_dis.item(), loss_g.item()])
            if epoch % 5 == 0:
                sc = _np(score)[:, 0]
                epochs.append(epoch)
                aucs.append(roc_auc_score(yt, sc))
                aps.append(average_precision_score(yt, sc, average="macro", pos_label=1, sample_weight=None))
                model.eval()
        return np.array(epochs), np.array(aucs), np.array(aps), np.array(losses, dtype=np.float64)

    epochs, aucs, aps, losses = train()
    out = dict(n=n, f=f, n_h=n_h, seed=seed, lr=lr, num_epoch=num_epoch, recon_epochs=recon_epochs, rowptr=rowptr, col=col,
               feat_raw=feat, ano=ano, features=_np(features[0]), all_idx=np.array(all_idx), idx_test=np.array(idx_test),
               normal_idx=np.array(normal_idx), eval_epochs=epochs, auc=aucs, ap=aps, losses=losses)
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
    out.update(model_case("a", n=301, n_entries=2400, f=10, n_h=32, seed=1, lr=1e-3, self_loop_frac=0.0, isolated=False))
    out.update(model_case("b", n=211, n_entries=2600, f=93, n_h=24, seed=3, lr=5e-4, self_loop_frac=0.1, isolated=True))
    np.savez_compressed(os.path.join(HERE, "fullgraph_aegis.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "fullgraph_aegis_planted.npz"), **planted_case())


if __name__ == "__main__":
    main()
