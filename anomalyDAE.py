#!/usr/bin/env python3
"""Full-graph AnomalyDAE comparison run on one MI355X:  python anomalyDAE.py --dataset reddit [--synthetic]

Same command line, per-dataset defaults (lr 1e-3 Amazon / reddit, 5e-4 t_finance, 3e-3 photo / elliptic; epochs reddit 500 /
t_finance 1500 / Amazon 800 / photo 500 / elliptic 500), seeding and prints as the reference's `anomalyDAE.py`: the training
loss every 2 epochs, AUROC / AP on idx_test every 5.  As there, the test scores printed at epoch e come from that epoch's
training forward (the weights before the step): they are scored from the forward's z and x_hat.  The dense branches, the GAT
layer, the fused reconstruction loss, the backward and Adam run in the kernels of libggad_hip.so on the CSR adjacency;
`--synthetic` / `--device` / `--quiet` / `--no_graph` as in `run.py` (the epoch is captured as a hipGraph at epoch 2 and
replayed unless `--no_graph`).
"""
import argparse
import os
import random
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ggad_amd.fullgraph import FlatAdam, FullGraphAdj  # noqa: E402
from ggad_amd.metrics import average_precision, roc_auc  # noqa: E402
from ggad_amd.model_anomalydae import Model, recon_score  # noqa: E402
from ggad_amd.utils import normalize_adj, preprocess_features  # noqa: E402
from run import load  # noqa: E402

LR = {"Amazon": 1e-3, "t_finance": 5e-4, "reddit": 1e-3, "photo": 3e-3, "elliptic": 3e-3}
EPOCHS = {"reddit": 500, "t_finance": 1500, "Amazon": 800, "photo": 500, "elliptic": 500}


def parse(argv=None):
    p = argparse.ArgumentParser(description="")
    p.add_argument("--dataset", type=str, default="t_finance")
    p.add_argument("--lr", type=float)
    p.add_argument("--weight_decay", type=float, default=0.0)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--embedding_dim", type=int, default=300)
    p.add_argument("--num_epoch", type=int)
    p.add_argument("--drop_prob", type=float, default=0.0)
    p.add_argument("--batch_size", type=int, default=300)
    p.add_argument("--subgraph_size", type=int, default=4)
    p.add_argument("--readout", type=str, default="avg")
    p.add_argument("--auc_test_rounds", type=int, default=256)
    p.add_argument("--negsamp_ratio", type=int, default=1)
    p.add_argument("--synthetic", action="store_true", help="generate a graph of the dataset's size instead of loading ./dataset/*.mat")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--no_graph", action="store_true", help="do not replay a captured hipGraph of the training epoch")
    a = p.parse_args(argv)
    if a.lr is None:
        a.lr = LR.get(a.dataset)
    if a.num_epoch is None:
        a.num_epoch = EPOCHS.get(a.dataset)
    if a.lr is None or a.num_epoch is None:
        p.error("no default lr / num_epoch for dataset {!r}: pass --lr and --num_epoch".format(a.dataset))
    return a


def setup(args, dev):
    """Graph, features, model and optimiser as anomalyDAE.py:66-110 builds them (CSR adjacency in HBM)."""
    adj, features, ano_label, idx_test, normal_label_idx, _ = load(args)
    if args.dataset in ["Amazon", "tf_finace", "reddit", "elliptic"]:                 # anomalyDAE.py:80 (same typo as run.py)
        features = preprocess_features(features)
    else:
        features = np.asarray(features.todense())
    nb_nodes, ft_size = features.shape
    full = FullGraphAdj(normalize_adj(adj) + sp.eye(nb_nodes), adj + sp.eye(nb_nodes), dev)     # :92-93
    feats = torch.FloatTensor(np.asarray(features, dtype=np.float32)[np.newaxis]).to(dev)
    model = Model(ft_size, args.embedding_dim, "prelu", args.negsamp_ratio, args.readout).to(dev)
    optimiser = FlatAdam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    return full, feats, model, optimiser, np.asarray(ano_label), np.asarray(idx_test, dtype=np.int64), np.asarray(normal_label_idx, dtype=np.int64)


def make_epoch(model, optimiser, feats, full, normal_idx):
    def train_epoch():
        optimiser.zero_grad()
        loss, z, xhat = model.train_forward(feats, full, normal_idx)      # anomalyDAE.py:136-137
        loss.backward()
        optimiser.step()
        return loss.detach(), z.detach(), xhat.detach()
    return train_epoch


def main():
    args = parse()
    print("Dataset: ", args.dataset)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed_all(args.seed)
    random.seed(args.seed)
    if not torch.cuda.is_available():
        sys.exit("anomalyDAE.py needs an MI355X: there is no CPU fallback")
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)      # the C-ABI launches on the CURRENT device's stream: it must be the one the tensors live on
    full, feats, model, optimiser, ano_label, idx_test, normal_idx = setup(args, dev)
    y_test_dev = torch.as_tensor(ano_label[idx_test].astype(np.int64), device=dev)
    x = feats[0]
    train_epoch = make_epoch(model, optimiser, feats, full, normal_idx)
    total_time, epoch_times = 0.0, []
    graph, static = None, None
    for epoch in range(args.num_epoch):
        start_time = time.time()
        model.train()
        if not args.no_graph and graph is None and epoch == 2:
            optimiser.zero_grad()
            import gc
            gc.collect()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static = train_epoch()
            print("training epoch captured as a hipGraph", flush=True)
        if graph is not None:
            graph.replay()
            loss, z, xhat = static
        else:
            loss, z, xhat = train_epoch()
        if epoch % 2 == 0:
            print("Epoch:", "%04d" % epoch, "train_loss=", "{:.5f}".format(loss.item()))
        if epoch % 5 == 0:
            model.eval()
            score = recon_score(z, xhat, x, full, idx_test)       # the test rows of this epoch's training forward (:138-145)
            print("Testing {} AUC:{:.4f}".format(args.dataset, roc_auc(score, y_test_dev)))
            print("Testing AP:", average_precision(score, y_test_dev))
            print("Total time is", total_time)
        torch.cuda.synchronize()
        epoch_times.append(time.time() - start_time)
        total_time += epoch_times[-1]
    med = float(np.median(epoch_times))
    n = full.n
    print("median epoch {:.3f} ms -> {:.1f} nodes/s (first epoch {:.1f} ms incl. one-off structure building / module load)".format(
        med * 1e3, n / med, epoch_times[0] * 1e3))


if __name__ == "__main__":
    main()
