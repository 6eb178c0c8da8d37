#!/usr/bin/env python3
"""Full-graph DOMINANT comparison run on one MI355X:  python dominant.py --dataset t_finance [--synthetic]

Same command line, per-dataset defaults (lr 1e-3 Amazon / reddit, 5e-4 t_finance, 3e-3 photo / elliptic; epochs reddit 500 /
t_finance 1500 / Amazon 800 / photo 500 / elliptic 500; elsewhere --lr and --num_epoch are required), seeding and prints as the
reference's `dominant.py`:

- every epoch: zero_grad, the forward on normal_label_idx / idx_test, loss.backward(), the Adam step (all parameters, --lr,
  --weight_decay; dense_stru and gat_layer never get a gradient, so Adam never moves them);
- every 2 epochs: train_loss; every 5 epochs: AUROC / AP of the epoch's test scores (from the training forward, before the step);
  every epoch: the total time so far (not with --quiet).
Features are row-normalised for Amazon / reddit / elliptic only (the reference's list names 'tf_finace', never T-Finance).  The epoch
is captured as a hipGraph at epoch 2, after the eager epochs have built the GCN embedding cache and the row structures, and replayed
(unless --no_graph).  DOMINANT draws nothing per epoch.  `--synthetic` / `--device` / `--quiet` / `--no_graph` as in `gaan.py`.
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
from ggad_amd.model_dominant import Model  # noqa: E402

LR = {"Amazon": 1e-3, "t_finance": 5e-4, "reddit": 1e-3, "photo": 3e-3, "elliptic": 3e-3}
EPOCHS = {"reddit": 500, "t_finance": 1500, "Amazon": 800, "photo": 500, "elliptic": 500}


def parse(argv=None):
    return parse_with_defaults(make_parser("t_finance"), argv, LR, EPOCHS)


def setup(args, dev):
    """Graph, features, model and optimiser as dominant.py:81-110 builds them (CSR adjacency in HBM)."""
    g = load_graph(args)
    full, feats, ft_size = prepare(args, g.adj, g.feat, dev)
    model = Model(ft_size, args.embedding_dim, "prelu", args.negsamp_ratio, args.readout).to(dev)
    optimiser = FlatAdam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    return full, feats, model, optimiser, np.asarray(g.ano_label), list(g.normal_idx), np.asarray(g.idx_test, dtype=np.int64)


def make_epoch(model, optimiser, feats, full, normal_idx, idx_test):
    def epoch_fn():
        optimiser.zero_grad()
        loss, score = model(feats, full, normal_idx, idx_test)
        loss.backward()
        optimiser.step()
        return loss.detach(), score.detach()
    return epoch_fn


def main():
    args = parse()
    print("Dataset: ", args.dataset)
    dev = init_process(args, "dominant.py")
    full, feats, model, optimiser, ano_label, normal_idx, idx_test = setup(args, dev)
    y_test_dev = torch.as_tensor(ano_label[idx_test].astype(np.int64), device=dev)
    cap = CapturedEpoch(make_epoch(model, optimiser, feats, full, normal_idx, idx_test), enabled=not args.no_graph,
                        before_capture=optimiser.zero_grad, after_capture=print_captured)
    total_time, epoch_times = 0.0, []
    for epoch in range(args.num_epoch):
        start_time = time.time()
        model.train()
        loss, score = cap.step(epoch)
        if epoch % 2 == 0:
            print("Epoch:", "%04d" % epoch, "train_loss=", "{:.5f}".format(loss.item()))
        if epoch % 5 == 0:
            model.eval()
            print_eval(args.dataset, score.view(-1), y_test_dev)
        torch.cuda.synchronize()
        epoch_times.append(time.time() - start_time)
        total_time += epoch_times[-1]
        if not args.quiet:
            print("Total time is", total_time)
    print_median(epoch_times, full.n, "the GCN branch / one-off structure building")


if __name__ == "__main__":
    main()
