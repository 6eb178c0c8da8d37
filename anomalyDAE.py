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
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ggad_amd.fullgraph import FlatAdam  # noqa: E402
from ggad_amd.fullgraph_script import (CapturedEpoch, init_process, load_graph, make_parser, parse_with_defaults, prepare,  # noqa: E402
                                       print_captured, print_eval, print_median)
from ggad_amd.model_anomalydae import Model, recon_score  # noqa: E402

LR = {"Amazon": 1e-3, "t_finance": 5e-4, "reddit": 1e-3, "photo": 3e-3, "elliptic": 3e-3}
EPOCHS = {"reddit": 500, "t_finance": 1500, "Amazon": 800, "photo": 500, "elliptic": 500}


def parse(argv=None):
    return parse_with_defaults(make_parser("t_finance"), argv, LR, EPOCHS)


def setup(args, dev):
    """Graph, features, model and optimiser as anomalyDAE.py:66-110 builds them (CSR adjacency in HBM)."""
    g = load_graph(args)
    full, feats, ft_size = prepare(args, g.adj, g.feat, dev)
    model = Model(ft_size, args.embedding_dim, "prelu", args.negsamp_ratio, args.readout).to(dev)
    optimiser = FlatAdam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    return full, feats, model, optimiser, np.asarray(g.ano_label), np.asarray(g.idx_test, dtype=np.int64), np.asarray(g.normal_idx, dtype=np.int64)


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
    dev = init_process(args, "anomalyDAE.py")
    full, feats, model, optimiser, ano_label, idx_test, normal_idx = setup(args, dev)
    y_test_dev = torch.as_tensor(ano_label[idx_test].astype(np.int64), device=dev)
    x = feats[0]
    cap = CapturedEpoch(make_epoch(model, optimiser, feats, full, normal_idx), enabled=not args.no_graph,
                        before_capture=optimiser.zero_grad, after_capture=print_captured)
    total_time, epoch_times = 0.0, []
    for epoch in range(args.num_epoch):
        start_time = time.time()
        model.train()
        loss, z, xhat = cap.step(epoch)
        if epoch % 2 == 0:
            print("Epoch:", "%04d" % epoch, "train_loss=", "{:.5f}".format(loss.item()))
        if epoch % 5 == 0:
            model.eval()
            score = recon_score(z, xhat, x, full, idx_test)       # the test rows of this epoch's training forward (:138-145)
            print_eval(args.dataset, score, y_test_dev)
            print("Total time is", total_time)
        torch.cuda.synchronize()
        epoch_times.append(time.time() - start_time)
        total_time += epoch_times[-1]
    print_median(epoch_times, full.n, "one-off structure building / module load")


if __name__ == "__main__":
    main()
