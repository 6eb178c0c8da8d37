#!/usr/bin/env python3
"""Full-graph GAAN comparison run on one MI355X:  python gaan.py --dataset Amazon [--synthetic]

Same command line, per-dataset defaults (lr 1e-3 Amazon / reddit / photo, 5e-4 t_finance, 5e-3 elliptic; epochs Amazon 800 /
t_finance 1500 / reddit 500 / photo 300 / elliptic 600; elsewhere --lr and --num_epoch are required), seeding and prints as the
reference's `gaan.py`:

- every epoch on all_idx: zero_grad of `optimiser` (all parameters, --lr, --weight_decay) and `optimiser_gen` (the generator, --lr,
  no weight decay), loss and loss_g backpropagated, `optimiser` then `optimiser_gen` stepped -- the generator gets two Adam
  updates from one gradient.  Every parameter with a gradient gets a fresh one each epoch, so FlatAdam.zero_grad (None) gives the
  updates of the reference's zeroing zero_grad;
- every 5 epochs: train_loss, AUROC / AP of the epoch's test scores (from the training forward, before the step) and the total
  time of the epochs before this one.
The epoch is captured as a hipGraph at epoch 2 and replayed (unless --no_graph), both optimisers inside it.  The forward's noise is
drawn from the CPU generator every epoch in the reference's order and copied into the buffer the captured epoch reads.
`--device_noise` (opt-in): the same stream continues on the device (ggad_amd.rng) and the draw opens the captured epoch; the host does
nothing between replays.  `--synthetic` / `--device` / `--quiet` / `--no_graph` as in `aegis.py`.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ggad_amd.fullgraph import FlatAdam  # noqa: E402
from ggad_amd.fullgraph_script import (DEVICE_NOISE_HELP, CapturedEpoch, NoiseFeed, init_process, load_graph, make_parser,  # noqa: E402
                                       parse_with_defaults, prepare, print_captured, print_eval, print_median)
from ggad_amd.model_gaan import Model  # noqa: E402

LR = {"Amazon": 1e-3, "t_finance": 5e-4, "reddit": 1e-3, "photo": 1e-3, "elliptic": 5e-3}
EPOCHS = {"reddit": 500, "t_finance": 1500, "Amazon": 800, "photo": 300, "elliptic": 600}


def parse(argv=None):
    return parse_with_defaults(make_parser("Amazon", device_noise_help=DEVICE_NOISE_HELP), argv, LR, EPOCHS)


def setup(args, dev):
    """Graph, features, model and the two optimisers as gaan.py:74-105 builds them (CSR adjacency in HBM)."""
    g = load_graph(args)
    full, feats, ft_size = prepare(args, g.adj, g.feat, dev)
    model = Model(ft_size, args.embedding_dim, "prelu", args.negsamp_ratio, args.readout).to(dev)
    optimiser = FlatAdam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    optimiser_gen = FlatAdam(model.generator.parameters(), lr=args.lr)
    return full, feats, model, optimiser, optimiser_gen, np.asarray(g.ano_label), list(g.all_idx), np.asarray(g.idx_test, dtype=np.int64)


def make_epoch(model, optimiser, optimiser_gen, feats, full, all_idx, idx_test):
    def epoch_fn():
        optimiser.zero_grad()
        optimiser_gen.zero_grad()
        loss, loss_g, score = model(feats, full, all_idx, idx_test)
        torch.autograd.backward([loss, loss_g])                   # loss.backward(); loss_g.backward()
        optimiser.step()
        optimiser_gen.step()
        return loss.detach(), score.detach()
    return epoch_fn


def main():
    args = parse()
    print("Dataset: ", args.dataset)
    dev = init_process(args, "gaan.py")
    full, feats, model, optimiser, optimiser_gen, ano_label, all_idx, idx_test = setup(args, dev)
    y_test_dev = torch.as_tensor(ano_label[idx_test].astype(np.int64), device=dev)
    n = full.n
    # the forward's noise (model_gaan.py:311): one (n, noise_dim) draw per epoch, in the reference's order
    noise = NoiseFeed(model, make_epoch(model, optimiser, optimiser_gen, feats, full, all_idx, idx_test), (n, model.noise_dim), dev,
                      args.device_noise)

    def before_capture():
        noise.before_capture()
        model.emb = None
        optimiser.zero_grad()
        optimiser_gen.zero_grad()

    def after_capture():
        noise.after_capture()
        print_captured()

    cap = CapturedEpoch(noise.epoch_fn, enabled=not args.no_graph, before_capture=before_capture, after_capture=after_capture)
    total_time, epoch_times = 0.0, []
    try:
        for epoch in range(args.num_epoch):
            start_time = time.time()
            model.train()
            loss, score = cap.step(epoch, noise.before_replay)
            if epoch % 5 == 0:
                print("Epoch:", "%04d" % epoch, "train_loss=", "{:.5f}".format(loss.item()))
                model.eval()
                print_eval(args.dataset, score.view(-1), y_test_dev)
                if not args.quiet:
                    print("Total time is", total_time)
            torch.cuda.synchronize()
            epoch_times.append(time.time() - start_time)
            total_time += epoch_times[-1]
    finally:
        noise.close()
    print_median(epoch_times, n, "one-off structure building / module load")


if __name__ == "__main__":
    main()
