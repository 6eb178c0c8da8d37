"""What the mini-batch handlers (`model_handler.py`, `model_handler_dominate.py`, `model_handler_anomalydae.py`,
`model_handler_aegis.py`) share: the loader and split of their constructors, the adjacency coercion, the best-checkpoint rule, the
report of a test sweep, and the epoch loop of the labelled-batch models (`model: 'SAGE'` on the set, step and epoch paths,
`model: 'PCGNN'`).  The loop of the reconstruction models lives in `model_handler_dominate.ModelHandler.train`, the GGAD loop
(blocks of epochs through `trainer.run_steps`) in `model_handler.ModelHandler.train`.
"""
from __future__ import annotations

import datetime
import os
import time

import numpy as np
import torch

from .dgraph import load_dgraphfin, normalize_features, split_dgraphfin
from .graph import DeviceGraph


def load_and_split(args, extra=(), **split_kw):
    """The body of a handler's constructor (`src/model_handler.py:23-247`): load (or take config key `data`), split, normalise, the
    reference's five prints (wording and typos are its own).  `split_kw`: the handler's fractions for `split_dgraphfin`; `extra`: keys
    of the split to carry into the dataset besides the common ones.  Returns (args, dataset)."""
    data = getattr(args, "data", None)
    if data is not None:
        homo, feat_data, labels = data
        labels = np.array(labels)
    elif args.data_name == "dgraphfin":
        homo, feat_data, labels = load_dgraphfin("../data/dgraphfin.npz", args.data_dir + "dgraphfin_adj_list")
    else:
        raise ValueError("only data_name 'dgraphfin' (or an explicit `data` entry) is supported")
    sp = split_dgraphfin(labels, args.seed, getattr(args, "test_ratio", 0.67), **split_kw)     # model_handler.py:29-30,150-178
    labels = sp["labels"]
    print(f"Run on {args.data_name}, postive/total num: {np.sum(labels)}/{len(labels)}, train num {len(sp['y_train'])}," +
          f"valid num {len(sp['y_valid'])}, valid positive num {np.sum(sp['y_valid'])} , test num {len(sp['y_test'])}, "
          f"test positive num {np.sum(sp['y_test'])}")
    print(f"Classification threshold: {args.thres}")
    print(f"Feature dimension: {feat_data.shape[1]}")
    feat_data = normalize_features(feat_data)                                                  # model_handler.py:225
    print(f"Model: {args.model}, multi-relation aggregator: {args.multi_relation}, emb_size: {args.emb_size}.")
    dataset = {"feat_data": feat_data, "labels": labels, "adj_lists": homo, "homo": homo}
    for k in ("idx_train", "idx_valid", "idx_test", "y_train", "y_valid", "y_test", "idx_labeled") + tuple(extra):
        dataset[k] = sp[k]
    return args, dataset


def device_graph(adj_lists, n, dev, cache=None, source_path=None) -> DeviceGraph:
    """The adjacency a handler was given as a `DeviceGraph`: one as it is, a (rowptr, col) pair uploaded, the reference's dict of sets
    converted (through the binary CSR cache `cache`, where one is named)."""
    if isinstance(adj_lists, DeviceGraph):
        return adj_lists
    if isinstance(adj_lists, tuple):
        return DeviceGraph(adj_lists[0], adj_lists[1], dev)
    return DeviceGraph.from_adj_lists_cached(adj_lists, n, dev, cache, source_path=source_path)


class BestCheckpoint:
    """The reference's checkpoint rule (`src/model_handler.py:302-306,393-409`): a validation AUC above the best so far (from 0) is
    saved under `save_dir + timestamp`; `restore` loads the last one saved.  `write=False` (every rank but the first) follows the
    rule without touching the disk or printing."""

    def __init__(self, save_dir, data_name, model_name, write=True):
        timestamp = datetime.datetime.fromtimestamp(int(time.time())).strftime("%Y-%m-%d %H-%M-%S")
        self.dir_saver = save_dir + timestamp
        self.path_saver = os.path.join(self.dir_saver, "{}_{}.pkl".format(data_name, model_name))
        self.write = write
        self.f1_mac_best, self.auc_best, self.ep_best = 0, 0, -1

    def offer(self, epoch, f1_mac, auc, model):
        if auc > self.auc_best:
            self.f1_mac_best, self.auc_best, self.ep_best = f1_mac, auc, epoch
            if self.write:
                if not os.path.exists(self.dir_saver):
                    os.makedirs(self.dir_saver)
                print("  Saving model ...")
                torch.save(model.state_dict(), self.path_saver)

    def restore(self, model):
        if self.ep_best >= 0 and self.write:
            print("Restore model from epoch {}".format(self.ep_best))
            print("Model path: {}".format(self.path_saver))
            model.load_state_dict(torch.load(self.path_saver))


def sweep_report(probs, labels, thres):
    """The closing lines of `test_sage` (`src/utils.py:237-247`) for the scores of a sweep; returns its 5-tuple."""
    from .metrics import binary_report
    r = binary_report(probs, torch.as_tensor(np.asarray(labels), device=probs.device), thres)
    print(f"   GNN F1-binary-1: {r['f1_1']:.4f}\tF1-binary-0: {r['f1_0']:.4f}" +
          f"\tF1-macro: {r['f1_macro']:.4f}\tG-Mean: {r['gmean']:.4f}\tAUC: {r['auc']:.4f}")
    print("Testing AP:", r["ap"])
    return r["f1_macro"], r["f1_1"], r["f1_0"], r["auc"], r["gmean"]


def train_labelled(args, dataset, model, train, pool, *, shuffle, join, step, report, sweep, log, epoch_fn=None):
    """The loop of `src/model_handler.py:310-414` for a model trained on labelled batches: per epoch one shuffle of `train` (`:314`),
    per batch a shuffle of the pseudo-anomaly `pool` and then the slice + the pool's first `n_pseudo` (`:341-347`); validation every
    `valid_epochs` on the TEST split (`:260-261`), the best checkpoint restored before the test sweep.

    `train` / `pool`: python lists shuffled by `random.shuffle` and joined by `+`, or int64 arrays shuffled by a `PyCompatRandom`
    and joined by `np.concatenate` -- the same draws either way.  `step(batch_nodes, batch_labels)` makes one optimiser step and
    returns its loss tensor(s); the batch's clock stops before they are read, and the floats go to `log` (a tuple per batch when
    there are several).  `epoch_fn(epoch)`, when given, replaces the shuffles and the batch loop of an epoch and returns its
    losses.  `report(epoch, means, epoch_time)` prints the epoch's line, `sweep(cases, labels, model, batch_size, thres)` scores."""
    num_batches = int(getattr(args, "num_batches", 150))               # :317
    n_pseudo = int(getattr(args, "n_pseudo", 50))
    bs, labels = args.batch_size, dataset["labels"]
    idx_valid, y_valid, idx_test, y_test = dataset["idx_test"], dataset["y_test"], dataset["idx_test"], dataset["y_test"]   # :260-261
    best = BestCheckpoint(args.save_dir, args.data_name, args.model)
    def record(sums, vals):
        log.append(vals[0] if len(vals) == 1 else tuple(vals))
        return [s + v for s, v in zip(sums, vals)] if sums else vals

    for epoch in range(args.num_epochs):
        sums, epoch_time = None, 0.0
        if epoch_fn is not None:
            t0 = time.time()
            epoch_losses = epoch_fn(epoch)
            epoch_time = time.time() - t0
            for l in epoch_losses:
                sums = record(sums, [float(l)])
        else:
            shuffle(train)                                             # :314
            for batch in range(num_batches):
                t0 = time.time()
                i0, i1 = batch * bs, min((batch + 1) * bs, len(train))
                shuffle(pool)                                          # :341
                batch_nodes = join(train[i0:i1], pool[:n_pseudo])      # :342,347
                out = step(batch_nodes, labels[np.asarray(batch_nodes)])
                epoch_time += time.time() - t0
                sums = record(sums, [float(v.item()) for v in out])
        report(epoch, [s / num_batches for s in sums], epoch_time)
        if epoch % args.valid_epochs == 0:
            print("Valid at epoch {}".format(epoch))
            f1_mac_val, _, _, auc_val, _ = sweep(idx_valid, y_valid, model, bs, args.thres)
            best.offer(epoch, f1_mac_val, auc_val, model)
    best.restore(model)
    return sweep(idx_test, y_test, model, bs, args.thres)
