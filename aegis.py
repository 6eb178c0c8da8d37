#!/usr/bin/env python3
"""Full-graph AEGIS comparison run on one MI355X:  python aegis.py --dataset reddit [--synthetic]

Same command line, per-dataset defaults (lr 1e-3 Amazon / reddit, 5e-4 t_finance; epochs reddit 500 / t_finance 1500 / Amazon 800;
elsewhere --lr and --num_epoch are required), seeding and prints as the reference's `aegis.py`:

- pre-training, `recon_num_epoch` epochs on normal_label_idx: loss_ae backward and a step of `optimiser_ae` (all parameters, lr
  1e-3) with NO zero_grad, so the gradients accumulate across these epochs, as there; one `ae_loss` line per epoch;
- main loop on all_idx (the shuffled permutation of the split): zero_grad of `optimiser` (all parameters, --lr) and `optimiser_gen`
  (the generator, --lr, no weight decay), loss_g and loss_ae backpropagated, `optimiser` then `optimiser_gen` stepped -- the
  generator gets two Adam updates from one gradient.  The reference pins torch 1.11, whose zero_grad zeroes gradients instead of
  dropping them; here every parameter with a gradient gets a fresh one each main epoch, so FlatAdam.zero_grad (None) gives the
  same updates;
- every 5 main epochs: train_loss (the reference prints loss_ae under that name), AUROC / AP of the epoch's test scores (from the
  training forward, before the step) and the total time.
Pre-training runs eager; the main epoch is captured as a hipGraph at main epoch 2 and replayed (unless --no_graph).  The forward's
noise is drawn from the CPU generator every epoch in the reference's order and copied into the buffer the captured epoch reads.
`--affinity_dir DIR`: at the epochs the reference plots (every 20), the three arrays it hands to draw_pdf_methods go to
DIR/aegis_<dataset>_affinity_<epoch>.npz (normal, generated, anomalous); the 'anomalous' nodes are np.array(all_idx)[ano_label == 1]
as the reference writes it -- with all_idx shuffled these are not the anomalies (a reference quirk, kept).  Plotting is out of scope.
`--device_noise` (opt-in): from the main loop on, the same stream continues on the device (ggad_amd.rng) and the draw opens the captured
epoch.  `--synthetic` / `--device` / `--quiet` / `--no_graph` as in `anomalyDAE.py`.
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
from ggad_amd.model_aegis import Model  # noqa: E402

LR = {"Amazon": 1e-3, "t_finance": 5e-4, "reddit": 1e-3}
EPOCHS = {"reddit": 500, "t_finance": 1500, "Amazon": 800}


def parse(argv=None):
    p = make_parser("reddit", no_graph_help="do not replay a captured hipGraph of the main training epoch",
                    device_noise_help=DEVICE_NOISE_HELP)
    p.add_argument("--recon_num_epoch", type=int, default=10)
    p.add_argument("--affinity_dir", type=str, default=None, help="write the arrays the reference plots every 20 epochs here")
    return parse_with_defaults(p, argv, LR, EPOCHS)


def setup(args, dev):
    """Graph, features, model and the three optimisers as aegis.py:71-100 builds them (CSR adjacency in HBM)."""
    g = load_graph(args)
    full, feats, ft_size = prepare(args, g.adj, g.feat, dev)
    model = Model(ft_size, args.embedding_dim, "prelu", args.negsamp_ratio, args.readout).to(dev)
    optimiser_ae = FlatAdam(model.parameters(), lr=1e-3, weight_decay=args.weight_decay)
    optimiser = FlatAdam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    optimiser_gen = FlatAdam(model.generator.parameters(), lr=args.lr)
    return (full, feats, model, optimiser_ae, optimiser, optimiser_gen, np.asarray(g.ano_label), list(g.all_idx),
            np.asarray(g.idx_test, dtype=np.int64), list(g.normal_idx))


def draw_arrays(affinity1, affinity2, all_idx, ano_label):
    """The three arrays aegis.py:155-166 hands to draw_pdf_methods."""
    real_abn = np.array(all_idx)[np.argwhere(ano_label == 1).squeeze()].tolist()
    real_nrm = np.array(all_idx)[np.argwhere(ano_label == 0).squeeze()].tolist()
    return affinity1[real_nrm], affinity2[:500], np.sort(affinity1[real_abn], kind="stable")[:50]


def make_main_epoch(model, optimiser, optimiser_gen, feats, full, all_idx, idx_test):
    def main_epoch():
        optimiser.zero_grad()
        optimiser_gen.zero_grad()
        loss_ae, loss_g, score, z, z_gen, _ = model.train_forward(feats, full, all_idx, idx_test)
        torch.autograd.backward([loss_g, loss_ae])                 # loss_g.backward(); loss_dis.backward() (loss_dis is loss_ae)
        optimiser.step()
        optimiser_gen.step()
        return loss_ae.detach(), score.detach(), z.detach(), z_gen.detach()
    return main_epoch


def main():
    args = parse()
    print("Dataset: ", args.dataset)
    dev = init_process(args, "aegis.py")
    full, feats, model, optimiser_ae, optimiser, optimiser_gen, ano_label, all_idx, idx_test, normal_idx = setup(args, dev)
    y_test_dev = torch.as_tensor(ano_label[idx_test].astype(np.int64), device=dev)
    n = full.n
    for epoch in range(args.recon_num_epoch):                        # aegis.py:118-124
        loss_ae = model.train_forward(feats, full, normal_idx, idx_test)[0]
        loss_ae.backward()
        optimiser_ae.step()
        loss_ae = loss_ae.detach()          # (nothing of an eager autograd graph may survive into the capture)
        print("Epoch:", "%04d" % epoch, "ae_loss=", "{:.5f}".format(loss_ae.item()))
    if args.affinity_dir:
        os.makedirs(args.affinity_dir, exist_ok=True)
    # the forward's noise (model_AEGIS.py:226): one (n, noise_dim) draw per main epoch, in the reference's order
    noise = NoiseFeed(model, make_main_epoch(model, optimiser, optimiser_gen, feats, full, all_idx, idx_test), (n, model.noise_dim), dev,
                      args.device_noise)

    def before_capture():
        noise.before_capture()
        optimiser_ae.zero_grad()
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
            loss_ae, score, z, z_gen = cap.step(epoch, noise.before_replay)
            if epoch % 20 == 0 and args.affinity_dir:                   # aegis.py:148-166 (the arrays; no plot)
                a1 = Model.affinity(z, full).cpu().numpy()
                a2 = Model.affinity(z_gen, full).cpu().numpy()
                nrm, gen, abn = draw_arrays(a1, a2, all_idx, ano_label)
                np.savez(os.path.join(args.affinity_dir, "aegis_{}_affinity_{}.npz".format(args.dataset, epoch)), normal=nrm, generated=gen,
                         anomalous=abn)
            if epoch % 5 == 0:
                print("Epoch:", "%04d" % epoch, "train_loss=", "{:.5f}".format(loss_ae.item()))
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
