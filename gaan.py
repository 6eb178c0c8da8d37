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
import argparse
import os
import random
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ggad_amd import synth  # noqa: E402
from ggad_amd.fullgraph import FlatAdam, FullGraphAdj  # noqa: E402
from ggad_amd.metrics import average_precision, roc_auc  # noqa: E402
from ggad_amd.model_gaan import Model  # noqa: E402
from ggad_amd.utils import load_mat, normalize_adj, preprocess_features, split_nodes  # noqa: E402
from run import SIZES  # noqa: E402

LR = {"Amazon": 1e-3, "t_finance": 5e-4, "reddit": 1e-3, "photo": 1e-3, "elliptic": 5e-3}
EPOCHS = {"reddit": 500, "t_finance": 1500, "Amazon": 800, "photo": 300, "elliptic": 600}


def parse(argv=None):
    p = argparse.ArgumentParser(description="")
    p.add_argument("--dataset", type=str, default="Amazon")
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
    p.add_argument("--device_noise", action="store_true", help="draw the per-epoch noise on the device from torch's own CPU stream "
                   "(ggad_amd.rng): the draw is the first node of the captured epoch; values agree with the host's to float32 rounding")
    a = p.parse_args(argv)
    if a.lr is None:
        a.lr = LR.get(a.dataset)
    if a.num_epoch is None:
        a.num_epoch = EPOCHS.get(a.dataset)
    if a.lr is None or a.num_epoch is None:
        p.error("no default lr / num_epoch for dataset {!r}: pass --lr and --num_epoch".format(a.dataset))
    return a


def load(args):
    """(adj, features, ano_label, all_idx, idx_test) as the reference's load_mat returns them."""
    if args.synthetic or not os.path.exists("./dataset/{}.mat".format(args.dataset)):
        if not args.synthetic:
            print("./dataset/{}.mat not found: using a synthetic graph of the same size".format(args.dataset))
        n, ne, f, rate = SIZES[args.dataset]
        rowptr, col = synth.make_graph(n, ne, args.seed, kind="powerlaw", max_degree=max(64, n // 8), exact=True)
        adj = synth.csr_to_scipy(rowptr, col, n)
        feat = sp.lil_matrix(synth.make_features(n, f, args.seed))
        ano = synth.make_labels(n, rate, args.seed)
        all_idx, _, _, idx_test, _, _ = split_nodes(ano, args.dataset, verbose=not args.quiet)
        return adj, feat, ano, all_idx, idx_test
    adj, feat, _, all_idx, _, _, idx_test, ano, _, _, _, _ = load_mat(args.dataset)
    return adj, feat, ano, all_idx, idx_test


def setup(args, dev):
    """Graph, features, model and the two optimisers as gaan.py:74-105 builds them (CSR adjacency in HBM)."""
    adj, features, ano_label, all_idx, idx_test = load(args)
    if args.dataset in ["Amazon", "tf_finace", "reddit", "elliptic"]:                 # gaan.py:77 (typo kept: never T-Finance)
        features = preprocess_features(features)
    else:
        features = np.asarray(features.todense())
    nb_nodes, ft_size = features.shape
    full = FullGraphAdj(normalize_adj(adj) + sp.eye(nb_nodes), adj + sp.eye(nb_nodes), dev)     # :89-91
    feats = torch.FloatTensor(np.asarray(features, dtype=np.float32)[np.newaxis]).to(dev)
    model = Model(ft_size, args.embedding_dim, "prelu", args.negsamp_ratio, args.readout).to(dev)
    optimiser = FlatAdam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    optimiser_gen = FlatAdam(model.generator.parameters(), lr=args.lr)
    return full, feats, model, optimiser, optimiser_gen, np.asarray(ano_label), list(all_idx), np.asarray(idx_test, dtype=np.int64)


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
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    random.seed(args.seed)
    if not torch.cuda.is_available():
        sys.exit("gaan.py needs an MI355X: there is no CPU fallback")
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)      # the C-ABI launches on the CURRENT device's stream: it must be the one the tensors live on
    full, feats, model, optimiser, optimiser_gen, ano_label, all_idx, idx_test = setup(args, dev)
    y_test_dev = torch.as_tensor(ano_label[idx_test].astype(np.int64), device=dev)
    n = full.n
    epoch_fn = make_epoch(model, optimiser, optimiser_gen, feats, full, all_idx, idx_test)
    total_time, epoch_times = 0.0, []
    graph, static, noise_buf = None, None, None
    # --device_noise: the CPU generator continues on the device from here on; the draw opens every epoch (and the captured one), and
    # the host generator gets the advanced state back when the loop ends
    mt = None
    if args.device_noise:
        from ggad_amd.rng import DeviceMT
        mt = DeviceMT.from_host(dev)
        noise_buf = torch.zeros(n, model.noise_dim, device=dev)
        model.noise_override = noise_buf
        host_epoch = epoch_fn

        def epoch_fn():
            mt.randn_(noise_buf)                                # this epoch's draw (model_gaan.py:311), in the reference's order
            return host_epoch()
    try:
        for epoch in range(args.num_epoch):
            start_time = time.time()
            model.train()
            if not args.no_graph and graph is None and epoch == 2:
                if mt is None:
                    noise_buf = torch.zeros(n, model.noise_dim, device=dev)
                    model.noise_override = noise_buf
                # nothing of the eager epochs' autograd graphs may survive into the capture
                loss = score = None
                model.emb = None
                optimiser.zero_grad()
                optimiser_gen.zero_grad()
                import gc
                gc.collect()
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    static = epoch_fn()
                if mt is None:
                    model.noise_override = None
                print("training epoch captured as a hipGraph", flush=True)
            if graph is not None:
                if mt is None:
                    noise_buf.copy_(torch.randn(n, model.noise_dim))       # this epoch's draw (model_gaan.py:311), in the reference's order
                graph.replay()
                loss, score = static
            else:
                loss, score = epoch_fn()
            if epoch % 5 == 0:
                print("Epoch:", "%04d" % epoch, "train_loss=", "{:.5f}".format(loss.item()))
                model.eval()
                sc = score.view(-1)
                print("Testing {} AUC:{:.4f}".format(args.dataset, roc_auc(sc, y_test_dev)))
                print("Testing AP:", average_precision(sc, y_test_dev))
                if not args.quiet:
                    print("Total time is", total_time)
            torch.cuda.synchronize()
            epoch_times.append(time.time() - start_time)
            total_time += epoch_times[-1]
    finally:
        if mt is not None:
            model.noise_override = None
            mt.to_host()
    if epoch_times:
        med = float(np.median(epoch_times))
        print("median epoch {:.3f} ms -> {:.1f} nodes/s (first epoch {:.1f} ms incl. one-off structure building / module load)".format(
            med * 1e3, n / med, epoch_times[0] * 1e3))


if __name__ == "__main__":
    main()
