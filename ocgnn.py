#!/usr/bin/env python3
"""Full-graph OCGNN comparison run on one MI355X:  python ocgnn.py --dataset reddit [--synthetic]

Same command line, per-dataset defaults (lr 5e-4 for t_finance, else 1e-3; epochs reddit 500 / t_finance 1500 / Amazon 800 /
elliptic 500 / photo 600), seeding, prints and evaluation cadence (AUROC / AP on idx_test every 5 epochs) as the reference's
`ocgnn.py`; the two GCN layers, the one-class loss, the backward and Adam run in the kernels of libggad_hip.so on the CSR
adjacency.  `--synthetic` / `--device` / `--quiet` / `--no_graph` as in `run.py`.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ggad_amd.fullgraph import FlatAdam  # noqa: E402
from ggad_amd.fullgraph_script import (CapturedEpoch, init_process, load_graph, make_parser, parse_with_defaults, prepare,  # noqa: E402
                                       print_eval, print_median)
from ggad_amd.model_ocgnn import Model, ocgnn_loss  # noqa: E402

LR = {"t_finance": 5e-4}
EPOCHS = {"reddit": 500, "t_finance": 1500, "Amazon": 800, "elliptic": 500, "photo": 600}


def parse(argv=None):
    return parse_with_defaults(make_parser("t_finance"), argv, LR, EPOCHS, fallback=(1e-3, 500))


def main():
    args = parse()
    print("Dataset: ", args.dataset)
    dev = init_process(args, "ocgnn.py")
    g = load_graph(args)
    full, feats, ft_size = prepare(args, g.adj, g.feat, dev)
    model = Model(ft_size, args.embedding_dim, "prelu", args.negsamp_ratio, args.readout).to(dev)
    optimiser = FlatAdam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    idx_test = np.asarray(g.idx_test, dtype=np.int64)
    normal_dev = torch.as_tensor(np.asarray(g.normal_idx, dtype=np.int64), device=dev)
    idx_test_dev = torch.as_tensor(idx_test, device=dev)
    y_test_dev = torch.as_tensor(np.asarray(g.ano_label)[idx_test].astype(np.int64), device=dev)
    total_time, epoch_times = 0.0, []

    def train_epoch():
        optimiser.zero_grad()
        emb = model(feats, full)
        loss, _ = ocgnn_loss(emb[0], normal_dev)                # torch.squeeze(emb)[normal_label_idx]   ocgnn.py:180-184
        loss.backward()
        optimiser.step()
        return loss.detach()

    # a host-bound epoch is captured (see run.py)
    cap = CapturedEpoch(train_epoch, enabled=not args.no_graph, before_capture=optimiser.zero_grad,
                        gate=lambda: epoch_times[1] < float(os.environ.get("GGAD_CAPTURE_BELOW_S", "20e-3")))
    for epoch in range(args.num_epoch):
        start_time = time.time()
        model.train()
        loss = cap.step(epoch)
        torch.cuda.synchronize()
        if epoch % 5 == 0:
            print("Epoch:", "%04d" % epoch, "train_loss=", "{:.5f}".format(loss.item()))
            model.eval()
            with torch.no_grad():
                _, score = ocgnn_loss(model(feats, full)[0])
            print_eval(args.dataset, score[idx_test_dev], y_test_dev)
            print("Total time is", total_time)
        epoch_times.append(time.time() - start_time)         # like the reference, the window includes the evaluation (ocgnn.py:210-211)
        total_time += epoch_times[-1]
    print_median(epoch_times, full.n, "one-off plan building / module load")


if __name__ == "__main__":
    main()
