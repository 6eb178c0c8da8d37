"""`ModelHandler` -- drop-in for the reference's DGraph driver (`src/model_handler.py`).

    ModelHandler(config).train() -> (f1_macro, f1_binary_1, f1_binary_0, auc, gmean)

Same config keys (`src/dgraph.yml`), same split, same batch schedule for equal seeds, same prints,
same checkpoint format (state_dict keys of `GCN`).  What differs is where the work runs: the batch
sub-graphs, the aggregation, the model step and Adam are HIP kernels on the MI355X; the python
`random` stream is continued by the native sampler; validation scores thousands of reference batches
per launch.  ``model: 'GCN'`` is the GGAD model.  ``model: 'SAGE'`` (the vanilla GraphSAGE baseline of
`src/graphsage.py:19-154`) cannot run through the reference's own loop -- `GraphSage.loss` returns one value where the loop
unpacks four (`:358-362`), and `test_sage` calls `to_prob(nodes, None)` where `GraphSage.to_prob` takes one argument
 -- here it is REPAIRED with exactly those two changes (`_train_sage`).

Extra, optional config keys:  ``device`` (cuda index), ``num_batches`` (default 150, the reference's
hard override `:317`), ``data`` = (adj_lists | DeviceGraph | (rowptr, col), feat_data, labels) to bypass
the file loader, ``log_every``, ``n_pseudo`` (pseudo-anomalies per batch, default 50: the reference's `:342-347`).  Under `torch.distributed` (backend nccl = RCCL) batches are dealt
round-robin over the ranks and gradients are all-reduced once per step.

``top_k: K`` / ``top_k_out`` (`model: 'GCN'`, one GPU): the K highest scores of the closing test sweep are ranked on the device in a
fixed order (`metrics.top_k`, csrc/topk.hip), kept in `self.ranked`, reported in one line and written to an `.npz`;
`ModelHandler(config).score(checkpoint)` does the sweep, the report and the ranking from a saved checkpoint without training.
``top_k_wide: true`` (with ``top_k`` > 0): the list is ranked by csrc/topk.hip, K up to 4,194,304 instead of 16,384.
``rank_wide: true`` (with ``eval_cache: true``): a validation / test list with more than 8,192 positives is reported from the
counting kernels of csrc/rank_metrics.hip instead of `binary_report`'s two device sorts.
``thres_select: CRIT`` (`model: 'GCN'`; f1, f1_macro, gmean, precision:X, fpr:X): after the best checkpoint is restored the validation
list is scored once more, the alert threshold that is best under CRIT is chosen on the device (`metrics.operating_point`), printed as
one `[threshold]` line, kept in `self.operating_point`, used by the closing test sweep instead of ``thres`` and written by rank 0 to
`<checkpoint>.thres.json`; `score(checkpoint)` with the key on reads that file.  The validation list is the reference's -- the test
split (`src/model_handler.py:260-261`) --, so the threshold, like the checkpoint, is chosen on the list it is then reported on.
``auc_ci: LEVEL`` (`model: 'GCN'`; 0 = off): after the closing test sweep, and in `score(checkpoint)`, the test AUROC is printed with
DeLong's standard error and the normal interval at LEVEL as one `[auc_ci]` line (`metrics.auc_ci`, csrc/rank_metrics.hip: exact
integer numerators), kept in `self.auc_interval`; `score(checkpoint, compare=other)` scores the same list under a second checkpoint and
prints DeLong's paired test of the two AUROCs as one `[compare]` line (`metrics.compare_auc`), kept in `self.auc_comparison`.
``ap_ci: LEVEL`` with ``boot_reps`` / ``boot_seed`` (`model: 'GCN'`; 0 = off): at the same two places, behind the `[auc_ci]` line, the
test average precision and AUROC are printed with the percentile intervals of a stratified bootstrap as one `[ap_ci]` line
(`metrics.ap_ci`, csrc/rank_metrics.hip: one workgroup per replicate), kept in `self.ap_interval`; the sweep's device scores are reused.
``compare_ap: LEVEL`` (`model: 'GCN'`; 0 = off; ``boot_reps`` / ``boot_seed`` as for ``ap_ci``): `score(checkpoint, compare=other)`
prints, behind the `[compare]` line, the paired stratified bootstrap of the two checkpoints' average precisions as one `[compare_ap]`
line (`metrics.compare_ap`: interval, standard error and p-value of the difference), kept in `self.ap_comparison`.
``explain: M`` / ``explain_out`` (with ``top_k`` > 0): every node of the ranked list is explained on the device (`explain.explain`,
csrc/explain.hip): its logit split exactly per feature and per neighbour, the M signed-greatest neighbour contributions listed; kept in
`self.explained`, reported in one `[explain]` line and written to an `.npz`; after `train()` and by `score(checkpoint)` alike.

The loader and split, the adjacency coercion, the checkpoint rule and the epoch loop of the labelled-batch models (`_train_sage`,
`_train_sage_device`, `_train_pcgnn` build model, optimiser and containers and hand them to it) live in `handler_loop.py`; the GGAD
loop (blocks of epochs through `trainer.run_steps`) is in `train` below.
"""
from __future__ import annotations

import argparse
import operator
import os
import random
import time

import numpy as np
import torch
import torch.nn as nn

from .graph import DeviceGraph
from .graphsage import GCN, Encoder, FeatureTable, GCNAggregator, GCNEncoder, GraphSage, MeanAggregator
from .handler_loop import BestCheckpoint, device_graph, load_and_split, sweep_report, train_labelled
from .metrics import write_ranked  # noqa: F401  (it lives beside `top_k`; re-exported: callers import it from here)
from .sage_utils import score_nodes, test_sage
from .sampler import PyCompatRandom
from .trainer import BatchSchedule, DGraphTrainer


def _autograd_step(gnn_model, optimizer):
    """The optimiser step of the labelled-batch models for `train_labelled`: `loss` returns one tensor (GraphSage: the first repair of
    the module docstring) or (loss, loss_constraint) (`:352-353`); the first is back-propagated."""
    def step(batch_nodes, batch_label):
        optimizer.zero_grad()
        out = gnn_model.loss(batch_nodes, batch_label)
        out = (out,) if isinstance(out, torch.Tensor) else tuple(out)
        out[0].backward()
        optimizer.step()
        return out
    return step


def _report_sage(epoch, means, epoch_time):
    print(f"Epoch: {epoch}, loss: {means[0]}, time: {epoch_time}s")


class ModelHandler(object):

    def __init__(self, config):
        args = argparse.Namespace(**config)
        if bool(getattr(args, "pcgnn_fused", False)) and not bool(getattr(args, "pcgnn_device", False)):
            raise ValueError("config key `pcgnn_fused` needs `pcgnn_device: true`: the fused head runs behind the relation kernels of "
                             "the device path")
        if bool(getattr(args, "sage_epoch", False)) and not bool(getattr(args, "sage_device", False)):
            raise ValueError("config key `sage_epoch` needs `sage_device: true`: the epoch path replays the kernels of the device path")
        if bool(getattr(args, "eval_cache", False)):
            if getattr(args, "model", None) != "GCN":
                raise ValueError("config key `eval_cache` needs `model: 'GCN'`: the resident sweep caches the inference rows of the GGAD "
                                 "encoder (the sweeps of the other models are not cached)")
            if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
                raise ValueError("config key `eval_cache` runs on one GPU: the resident sweep is not sharded over the ranks of a "
                                 "torch.distributed world yet")
        if bool(getattr(args, "rank_wide", False)) and not bool(getattr(args, "eval_cache", False)):
            raise ValueError("config key `rank_wide` needs `eval_cache: true`: it chooses the metric kernels of the resident sweep "
                             "(without the sweep the metrics come from `binary_report`)")
        top_k, top_k_out = getattr(args, "top_k", 0) or 0, str(getattr(args, "top_k_out", "") or "")
        top_k_wide = bool(getattr(args, "top_k_wide", False))
        if top_k_wide and not top_k:
            raise ValueError("config key `top_k_wide` needs `top_k: K` with K > 0: it chooses the kernels that rank the K highest scores "
                             "(there is no ranking while `top_k` is 0)")
        if top_k or top_k_out:
            if getattr(args, "model", None) != "GCN":
                raise ValueError("config keys `top_k` / `top_k_out` need `model: 'GCN'`: the ranked list is made from the scores of the "
                                 "GGAD test sweep (the other models' sweeps are not ranked)")
            if not top_k:
                raise ValueError("config key `top_k_out` needs `top_k: K` with K > 0: there is no ranking to write while `top_k` is 0")
            from .metrics import check_k
            check_k(top_k, "config key `top_k`", wide=top_k_wide)
            if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
                raise ValueError("config keys `top_k` / `top_k_out` run on one GPU: the ranking is not made under a torch.distributed "
                                 "world of several ranks yet")
        explain_m, explain_out = getattr(args, "explain", 0) or 0, str(getattr(args, "explain_out", "") or "")
        if explain_m or explain_out:
            if not top_k:
                raise ValueError("config keys `explain` / `explain_out` need `top_k: K` with K > 0: `explain` explains the nodes of the "
                                 "ranked list (there is no list while `top_k` is 0)")
            if not explain_m:
                raise ValueError("config key `explain_out` needs `explain: M` with M > 0: there is no explanation to write while "
                                 "`explain` is 0")
            from .explain import check_m
            check_m(explain_m, "config key `explain`")
        self.ranked = None
        self.explained = None
        self.operating_point = None
        self.thres_select = None                                 # config key `thres_select`: (name, param) of the criterion, else None
        if str(getattr(args, "thres_select", "") or ""):
            if getattr(args, "model", None) != "GCN":
                raise ValueError("config key `thres_select` needs `model: 'GCN'`: the threshold is chosen from the scores of the GGAD "
                                 "validation sweep")
            from .metrics import parse_criterion
            self.thres_select = parse_criterion(args.thres_select)
        self.auc_interval = self.auc_comparison = None
        self.auc_level = float(getattr(args, "auc_ci", 0) or 0)  # config key `auc_ci`: the level of the interval, 0 = off
        if self.auc_level:
            if getattr(args, "model", None) != "GCN":
                raise ValueError("config key `auc_ci` needs `model: 'GCN'`: the interval is made from the scores of the GGAD test sweep")
            if not 0.0 < self.auc_level < 1.0:
                raise ValueError(f"config key `auc_ci`: {args.auc_ci!r} is not a confidence level inside (0, 1) (0 = off)")
        self.ap_interval = None
        self.ap_level = float(getattr(args, "ap_ci", 0) or 0)    # config key `ap_ci`: the level of the bootstrap interval, 0 = off
        self.boot_reps, self.boot_seed = getattr(args, "boot_reps", 1000), getattr(args, "boot_seed", 0)
        if self.ap_level:
            if getattr(args, "model", None) != "GCN":
                raise ValueError("config key `ap_ci` needs `model: 'GCN'`: the interval is made from the scores of the GGAD test sweep")
            if not 0.0 < self.ap_level < 1.0:
                raise ValueError(f"config key `ap_ci`: {args.ap_ci!r} is not a confidence level inside (0, 1) (0 = off)")
        self.ap_comparison = None
        self.compare_ap_level = float(getattr(args, "compare_ap", 0) or 0)      # config key `compare_ap`: the level, 0 = off
        if self.compare_ap_level:
            if getattr(args, "model", None) != "GCN":
                raise ValueError("config key `compare_ap` needs `model: 'GCN'`: the test is made from the scores of the GGAD test sweep")
            if not 0.0 < self.compare_ap_level < 1.0:
                raise ValueError(f"config key `compare_ap`: {args.compare_ap!r} is not a confidence level inside (0, 1) (0 = off)")
        self.args, self.dataset = load_and_split(args, extra=("idx_anomaly",))

    @staticmethod
    def thres_path(checkpoint):
        """The side file of config key `thres_select`, next to the checkpoint: settings only (the `.pkl` stays a plain state dict)."""
        return str(checkpoint) + ".thres.json"

    def _choose_threshold(self, gnn_model, ids, labels, sweep, dist, verbose):
        """Config key `thres_select`: one more sweep over the validation list under the weights `gnn_model` holds, the operating point
        of its scores (`metrics.operating_point`: one call, one read-back), one `[threshold]` line; kept in `self.operating_point`.
        Under a torch.distributed world every rank calls it on the all-reduced scores."""
        from .metrics import operating_point
        name, param = self.thres_select
        if sweep is not None:
            op = sweep.operating_point(name, param, thres=self.args.thres)
        else:
            scores = score_nodes(gnn_model, ids, self.args.batch_size, device=True, dist=dist)
            lab = np.asarray(labels).reshape(-1).astype(np.uint8)
            op = operating_point(scores, torch.from_numpy(lab).to(scores.device), name, param, thres=self.args.thres,
                                 pos_cap=max(1, int(np.count_nonzero(lab == 1))))
        self.operating_point = op
        if verbose:
            print(f"[threshold] {self.args.thres_select}: threshold {op.thres!r}\tvalue {op.value!r}\tTP: {op.tp}\tFP: {op.fp}\tFN: {op.fn}"
                  f"\tTN: {op.tn}" + ("" if op.feasible else "\t(no candidate meets the constraint: no node alerts)"))
        return op

    def _write_threshold(self, checkpoint, op, epoch):
        import json
        import struct
        doc = {"criterion": op.criterion, "param": op.param, "thres": op.thres,
               "thres_bits": struct.unpack("<I", struct.pack("<f", op.thres))[0], "value": op.value,
               "tp": op.tp, "fp": op.fp, "fn": op.fn, "tn": op.tn, "epoch": int(epoch)}
        with open(self.thres_path(checkpoint), "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")

    def _read_threshold(self, checkpoint):
        """The threshold of the side file, from its bit pattern: exactly the float32 that was chosen."""
        import json
        import struct
        path = self.thres_path(checkpoint)
        if not os.path.exists(path):
            raise ValueError(f"config key `thres_select`: {path} not found (it is written next to the checkpoint by a training run "
                             "with the key on)")
        with open(path) as fh:
            doc = json.load(fh)
        return float(struct.unpack("<f", struct.pack("<I", int(doc["thres_bits"])))[0]), doc

    def _auc_ci(self, scores, labels, sweep, verbose=True):
        """Config key `auc_ci`: the interval of `scores` (the device scores of a sweep, already made) on `labels`, one `[auc_ci]` line;
        kept in `self.auc_interval`."""
        from .metrics import auc_ci, format_auc_ci
        if sweep is not None:
            ci = sweep.auc_ci(self.auc_level, scores=scores)
        else:
            lab = np.asarray(labels).reshape(-1).astype(np.uint8)
            ci = auc_ci(scores, torch.from_numpy(lab).to(scores.device), self.auc_level, pos_cap=max(1, int(np.count_nonzero(lab == 1))))
        self.auc_interval = ci
        if verbose:
            print(format_auc_ci(ci))
        return ci

    def _ap_ci(self, scores, labels, sweep, verbose=True):
        """Config key `ap_ci`: the bootstrap interval of `scores` (the device scores of a sweep, already made) on `labels`, one
        `[ap_ci]` line; kept in `self.ap_interval`."""
        from .metrics import ap_ci, format_ap_ci
        if sweep is not None:
            ci = sweep.ap_ci(self.ap_level, self.boot_reps, self.boot_seed, scores=scores)
        else:
            lab = np.asarray(labels).reshape(-1).astype(np.uint8)
            ci = ap_ci(scores, torch.from_numpy(lab).to(scores.device), self.ap_level, self.boot_reps, self.boot_seed,
                       pos_cap=max(1, int(np.count_nonzero(lab == 1))))
        self.ap_interval = ci
        if verbose:
            print(format_ap_ci(ci))
        return ci

    def _compare(self, scores, other, gnn_model, engine, ids, labels, sweep):
        """`score(compare=other)`: the same list scored under the weights of `other` -- by the same sweep, whose cached rows do not
        depend on the weights -- and DeLong's paired test of the two AUROCs, one `[compare]` line; kept in `self.auc_comparison`."""
        from .metrics import compare_ap, compare_auc, format_compare, format_compare_ap
        gnn_model.load_state_dict(torch.load(other))
        engine.sync_params()
        boot = (self.compare_ap_level, self.boot_reps, self.boot_seed)
        if sweep is not None:
            scores_b = sweep.scores()
            c = sweep.compare(scores_b, scores=scores)
            ca = sweep.compare_ap(scores_b, scores, *boot) if self.compare_ap_level else None
        else:
            lab = np.asarray(labels).reshape(-1).astype(np.uint8)
            scores_b = score_nodes(gnn_model, ids, self.args.batch_size, device=True)
            y, cap = torch.from_numpy(lab).to(scores.device), max(1, int(np.count_nonzero(lab == 1)))
            c = compare_auc(scores, scores_b, y, pos_cap=cap)
            ca = compare_ap(scores, scores_b, y, *boot, pos_cap=cap) if self.compare_ap_level else None
        self.auc_comparison, self.ap_comparison = c, ca
        print(format_compare(c))
        if ca is not None:                           # config key `compare_ap`: the paired bootstrap of the two APs, behind `[compare]`
            print(format_compare_ap(ca))
        return c

    def _build_gcn(self):
        """The GGAD model as `src/model_handler.py:263-296` builds it, shared by `train` and `score`: device, graph (through the
        binary CSR cache of the real data set), `FeatureTable`, aggregator, encoder, `GCN`, and the engine's optimiser settings.
        Draws from torch's RNG exactly what the reference does.  Returns (dev, graph, features, gnn_model, engine)."""
        args = self.args
        dev = torch.device("cuda", int(getattr(args, "device", torch.cuda.current_device())))
        torch.cuda.set_device(dev)
        feat_data, adj_lists = self.dataset["feat_data"], self.dataset["adj_lists"]
        n, f = feat_data.shape
        # same RNG consumption as the reference: nn.Embedding's default init draws N x F normals (:263)
        nn.Embedding(n, f)
        # the reference's pickled dict of sets: converted once, then served from a binary CSR cache beside it
        # (keyed by size + mtime of the pickle; written under a per-process temporary name: ranks may convert concurrently)
        cache = src = None
        if getattr(args, "data_name", "") == "dgraphfin" and getattr(args, "data", None) is None:
            src = args.data_dir + "dgraphfin_adj_list"
            cache = os.path.join(args.data_dir, "dgraphfin_adj_list.csr.npz")
        graph = device_graph(adj_lists, n, dev, cache, source_path=src)
        features = FeatureTable(torch.FloatTensor(np.asarray(feat_data, dtype=np.float32)))
        agg_gcn = GCNAggregator(features, cuda=True)
        enc_gcn = GCNEncoder(features, f, args.emb_size, graph, agg_gcn, gcn=True, cuda=True)
        gnn_model = GCN(2, enc_gcn)
        engine = enc_gcn.engine
        engine.lr, engine.wd = float(args.lr), float(args.weight_decay)
        engine.sync_params()
        return dev, graph, features, gnn_model, engine

    def _rank(self, scores, ids, labels, sweep, k, verbose=True, model=None):
        """Config key `top_k` / `score(k=)`: the `Ranked` head of `scores` (the device scores of a sweep over `ids`, already made: nothing
        is scored again), kept in `self.ranked`; one printed line; the `.npz` of config key `top_k_out`.  Config key `top_k_wide`: ranked
        by `ggad_topk_wide_f32` (K above 16,384).  Config key `explain: M` (`model`: the `GCN` whose sweep made `scores`): every ranked
        node is explained under the weights that scored it (`explain.explain`, csrc/explain.hip), kept in `self.explained`; one
        `[explain]` line; the `.npz` of config key `explain_out`."""
        from .metrics import precision_recall_at, top_k
        wide = bool(getattr(self.args, "top_k_wide", False))
        if sweep is not None:
            ranked = sweep.top_k(k, scores=scores, wide=wide)
        else:
            lab = None if labels is None else torch.from_numpy(np.asarray(labels).reshape(-1).astype(np.uint8)).to(scores.device)
            ranked = top_k(scores, k, lab, torch.from_numpy(np.asarray(ids, dtype=np.int64).reshape(-1)).to(scores.device), wide=wide)
        self.ranked = ranked
        if verbose:
            if ranked.cum_pos is not None and ranked.m:
                prec, rec = precision_recall_at(ranked, ranked.m)
                print(f"Top-{ranked.m}: precision@K {prec:.4f}\trecall@K {rec:.4f}\thits {int(ranked.cum_pos[-1])} of {ranked.n_pos}"
                      f"\ttied left out {ranked.tied_left_out}")
            else:
                print(f"Top-{ranked.m}: no labels\ttied left out {ranked.tied_left_out}")
            out = str(getattr(self.args, "top_k_out", "") or "")
            if out:
                write_ranked(out, ranked, labels)
        explain_m = int(getattr(self.args, "explain", 0) or 0)
        if explain_m:
            from .explain import explain, write_explained
            if sweep is not None:
                ex = sweep.explain(ranked, explain_m)
            else:
                ex = explain(model, np.asarray(ids, dtype=np.int64).reshape(-1), self.args.batch_size, ranked, explain_m)
            self.explained = ex
            if verbose:
                print(f"[explain] rows explained {ex.rows}\tneighbours listed {ex.m}\tmax |z - sum_j t_j| {ex.completeness():.3e}"
                      f"\trows on the workspace branch {ex.rows_workspace}")
                out = str(getattr(self.args, "explain_out", "") or "")
                if out:
                    write_explained(out, ranked, ex)
        return ranked

    def score(self, checkpoint, ids=None, labels=None, k=None, compare=None):
        """Scores from a saved checkpoint, without training: the model is built as `train` builds it, the state dict of `checkpoint`
        (a `.pkl` of `BestCheckpoint`) is loaded and the engine synchronised exactly as the restore at the end of `train` does, and
        `ids` are swept in `test_sage`'s slices of `batch_size` (whose per-slice normalisation matters).  Default: the test split with
        its labels, which follows from the config alone (`split_dgraphfin` reseeds itself from `seed`).  With labels `test_sage`'s report
        is printed and its 5-tuple kept in `self.metrics`; with `k` (default: config key `top_k`) > 0 the scores are ranked (`_rank`).
        Honours `eval_cache`.  With labels, config key `auc_ci` prints the `[auc_ci]` line and `compare` (a second checkpoint) the
        `[compare]` line (and, with config key `compare_ap`, the `[compare_ap]` line behind it); the model then holds the second checkpoint's
        weights.  Returns (device float32 scores, `Ranked` or None)."""
        args = self.args
        if args.model != "GCN":
            raise NotImplementedError("ModelHandler.score serves model 'GCN' (GGAD)")
        if not torch.cuda.is_available():
            raise RuntimeError("ModelHandler.score needs an MI355X: the GGAD hot path has no CPU fallback")
        k = int(getattr(args, "top_k", 0) or 0) if k is None else int(k)
        if k:
            from .metrics import check_k
            check_k(k, "ModelHandler.score", wide=bool(getattr(args, "top_k_wide", False)))
        if compare is not None and ids is not None and labels is None:
            raise ValueError("ModelHandler.score: `compare` tests two AUROCs against each other: it needs labels")
        thres = args.thres
        if self.thres_select is not None:                        # config key `thres_select`: report at the threshold chosen in training
            thres, self.thres_doc = self._read_threshold(checkpoint)
        _, _, _, gnn_model, engine = self._build_gcn()
        self.model = gnn_model
        gnn_model.load_state_dict(torch.load(checkpoint))
        engine.sync_params()
        if ids is None:
            ids, labels = self.dataset["idx_test"], self.dataset["y_test"]
        sweep = None
        if bool(getattr(args, "eval_cache", False)):
            from .eval_cache import ResidentSweep
            sweep = ResidentSweep(gnn_model, ids, labels, args.batch_size, rank_wide=bool(getattr(args, "rank_wide", False)))
        self.eval_sweeps = (sweep, sweep)
        self.metrics, self.sweep_ap = None, []
        if labels is not None:
            keep = []
            self.metrics = test_sage(ids, labels, gnn_model, args.batch_size, thres, resident=sweep, keep=keep)
            self.sweep_ap.append(getattr(test_sage, "last_ap", None))
            scores = keep[0]
        else:
            scores = sweep.scores() if sweep is not None else score_nodes(gnn_model, ids, args.batch_size, device=True)
        self.test_scores = scores
        self.ranked = self._rank(scores, ids, labels, sweep, k, model=gnn_model) if k else None
        if self.auc_level and labels is not None:
            self._auc_ci(scores, labels, sweep)
        if self.ap_level and labels is not None:
            self._ap_ci(scores, labels, sweep)
        if compare is not None:
            self._compare(scores, compare, gnn_model, engine, ids, labels, sweep)
        return scores, self.ranked

    def train(self):
        args = self.args
        if args.model == "SAGE":
            return self._train_sage()
        if args.model == "PCGNN":
            return self._train_pcgnn()
        if args.model != "GCN":
            raise NotImplementedError("models 'GCN' (GGAD), 'SAGE' and 'PCGNN' are trainable")
        if not torch.cuda.is_available():
            raise RuntimeError("ModelHandler.train needs an MI355X: the GGAD hot path has no CPU fallback")
        dist = torch.distributed if (torch.distributed.is_available() and torch.distributed.is_initialized()) else None
        world = dist.get_world_size() if dist else 1
        rank = dist.get_rank() if dist else 0
        idx_train = self.dataset["idx_train"]
        idx_valid, y_valid, idx_test, y_test = (self.dataset["idx_test"], self.dataset["y_test"],
                                                self.dataset["idx_test"], self.dataset["y_test"])   # :260-261
        _, graph, features, gnn_model, engine = self._build_gcn()

        best = BestCheckpoint(args.save_dir, args.data_name, args.model, write=rank == 0)   # every rank follows the rule, rank 0 saves

        num_batches = int(getattr(args, "num_batches", 150))                            # :317
        rng = PyCompatRandom.from_python_state(random.getstate())
        # data parallel: `dp_sampler: independent` (the default when world > 1) gives every rank a batch stream of its own
        # (seed * 1000003 + rank + 1).  The bit-exact sampler is ONE serial Mersenne-Twister stream (~31 us per batch on the host):
        # dealt to W ranks (`dp_sampler: shared`, rank r takes batches r, r + W, ...) every rank must generate all W batches of a
        # step, which caps an end-to-end run at ~6.4 M nodes/s for ANY W -- below one GPU's steady state.  The trajectory is not the
        # reference's at W > 1 in either mode (global batch W x 150), so nothing is lost; `shared` stays as the opt-in for checks
        # against the W-batch gradient-averaging oracle (tests/test_distributed_cpu.py).  W = 1: the reference's own stream.
        own_stream = world > 1 and str(getattr(args, "dp_sampler", "independent")) != "shared"
        if own_stream:
            rng = PyCompatRandom(int(getattr(args, "seed", 0)) * 1000003 + rank + 1)
        sched = BatchSchedule(idx_train, self.dataset["idx_anomaly"], self.dataset["labels"], args.batch_size, rng,
                              n_pseudo=int(getattr(args, "n_pseudo", 50)), batches_per_epoch=num_batches)      # (50: the reference's, :342-347)
        allreduce = None
        if world > 1:
            def allreduce(t):
                dist.all_reduce(t, op=dist.ReduceOp.SUM)
        exchange = None
        want_oneshot = os.environ.get("GGAD_EXCHANGE", "oneshot") == "oneshot"
        if world > 1:                                   # rank 0's choice holds for everybody (the hand-shake below is collective)
            flag = torch.tensor([int(want_oneshot)], dtype=torch.int32,
                                device=features.weight.device if dist.get_backend() == "nccl" else "cpu")
            dist.broadcast(flag, src=0)
            want_oneshot = bool(flag.item())
        if world > 1 and want_oneshot and engine.D <= int(engine.lib.ggad_max_embed_dim()):     # (emb_size > 64: the all-reduce path)
            # one-shot peer-write exchange inside the gradient / Adam launch; every rank agrees on whether
            # it is usable, else all of them keep the all-reduce
            from .exchange import OneShotExchange
            n_par = int(engine.n_train)
            try:
                exchange = OneShotExchange(rank, world, n_par, features.weight.device)
            except Exception:
                exchange = None
            good = exchange.connect(dist) if exchange is not None else OneShotExchange.decline(dist, features.weight.device)
            if not good:
                exchange = None
        steps_per_epoch = max(1, num_batches // world)
        trainer = DGraphTrainer(graph, features.weight.data, args.emb_size, sched, chunk_batches=steps_per_epoch, rank=rank,
                                world_size=world, allreduce=allreduce, engine=engine, exchange=exchange, own_stream=own_stream)
        self.trainer, self.model = trainer, gnn_model
        self.sweep_ap = []                                      # AP of every sweep, validation sweeps then the test sweep (the reference prints it)
        self.epoch_losses, self.valid_history = [], []          # {total, cls, margin, rec} of every batch; (epoch, five metrics) of every sweep
        # config key `eval_cache`: one resident sweep per distinct id list (validation and test are the same list, :260-261): the plans
        # are built once, a sweep is one score launch over the cached rows and the counting kernels of csrc/rank_metrics.hip
        sweep_valid = sweep_test = None
        if bool(getattr(args, "eval_cache", False)):
            from .eval_cache import ResidentSweep
            wide = bool(getattr(args, "rank_wide", False))       # config key `rank_wide`: lists above 8,192 positives keep the counting route
            sweep_valid = ResidentSweep(gnn_model, idx_valid, y_valid, args.batch_size, rank_wide=wide)
            sweep_test = sweep_valid if (idx_test is idx_valid and y_test is y_valid) else \
                ResidentSweep(gnn_model, idx_test, y_test, args.batch_size, rank_wide=wide)
        self.eval_sweeps = (sweep_valid, sweep_test)
        trainer.start_stream(steps_per_epoch * args.num_epochs)        # sampler thread alive across the validation pauses
        total_time = 0.0
        epoch = 0
        while epoch < args.num_epochs:
            # run up to (and including) the next validation epoch in one call: the sampler thread then prefetches
            # the following epochs' batch schedules while the GPU trains (reference validates when epoch % valid_epochs == 0)
            last = epoch
            while last % args.valid_epochs != 0 and last + 1 < args.num_epochs:
                last += 1
            n_ep = last - epoch + 1
            t0 = time.time()
            trainer.run_steps(steps_per_epoch * n_ep)
            torch.cuda.synchronize()
            trainer.check_exchange(dist if world > 1 else None)
            block_time = time.time() - t0
            lall = engine.losses(steps_per_epoch * n_ep).astype(np.float64)
            for j in range(n_ep):
                l = lall[j * steps_per_epoch:(j + 1) * steps_per_epoch]
                self.last_epoch_losses = l
                self.epoch_losses.append(l)
                if rank == 0:
                    print(f"Epoch: {epoch + j}, loss: {l[:, 0].mean()}, marigin_loss: {l[:, 2].mean()}, time: {block_time / n_ep}s")
                    print("loss_cls", l[:, 1].mean())
                    print("total_time is", total_time)
                    print("loss_constraint", l[:, 2].mean())
            epoch = last
            if epoch % args.valid_epochs == 0:
                # the validation sweep is sharded over the ranks (contiguous ranges of the reference's batches, one
                # all-reduce of the scores); every rank sees the same metrics, rank 0 prints and saves
                if rank == 0:
                    print("Valid at epoch {}".format(epoch))
                f1_mac_val, f1_1_val, f1_0_val, auc_val, gmean_val = test_sage(idx_valid, y_valid, gnn_model, args.batch_size,
                                                                               args.thres, dist=dist, verbose=rank == 0,
                                                                               resident=sweep_valid)
                self.valid_history.append((epoch, (f1_mac_val, f1_1_val, f1_0_val, auc_val, gmean_val)))
                self.sweep_ap.append(getattr(test_sage, "last_ap", None))
                best.offer(epoch, f1_mac_val, auc_val, gnn_model)
            if dist:
                dist.barrier()
            total_time += time.time() - t0
            epoch += 1
        random.setstate(rng.to_python_state())       # hand the stream back to python `random`
        self.end_state = {k: v.detach().clone() for k, v in gnn_model.state_dict().items() if "features" not in k}   # before the restore
        if best.ep_best >= 0:
            best.restore(gnn_model)
            if dist and world > 1:
                dist.broadcast(engine.params, src=0)          # every rank tests the restored weights
            engine.sync_params()
        top_k = int(getattr(args, "top_k", 0) or 0)
        keep = [] if top_k or self.auc_level or self.ap_level else None    # config keys `top_k`, `auc_ci`, `ap_ci`: the sweep's device scores are kept, not made twice
        thres = args.thres
        if self.thres_select is not None:            # config key `thres_select`: the closing sweep reports at the chosen threshold
            op = self._choose_threshold(gnn_model, idx_valid, y_valid, sweep_valid, dist, verbose=rank == 0)
            thres = op.thres
            if rank == 0 and best.ep_best >= 0:
                self._write_threshold(best.path_saver, op, best.ep_best)
        res = test_sage(idx_test, y_test, gnn_model, args.batch_size, thres, dist=dist, verbose=rank == 0, resident=sweep_test,
                        keep=keep)
        self.sweep_ap.append(getattr(test_sage, "last_ap", None))
        if top_k:
            self.test_scores = keep[0]
            self._rank(keep[0], idx_test, y_test, sweep_test, top_k, verbose=rank == 0, model=gnn_model)
        if self.auc_level:
            self._auc_ci(keep[0], y_test, sweep_test, verbose=rank == 0)
        if self.ap_level:
            self._ap_ci(keep[0], y_test, sweep_test, verbose=rank == 0)
        return res


    # ---------------------------------------------------------------------------------------------------------------- SAGE
    def _cuda_device(self):
        if not torch.cuda.is_available():
            raise RuntimeError("ModelHandler.train needs an MI355X: there is no CPU fallback")
        dev = torch.device("cuda", int(getattr(self.args, "device", torch.cuda.current_device())))
        torch.cuda.set_device(dev)
        return dev

    def _train_sage(self):
        """`model: 'SAGE'`: MeanAggregator -> Encoder(gcn=False) -> GraphSage(2, enc) as `src/model_handler.py:278-293` builds
        them, trained by the loop of `:310-370` with the two repairs named in the module docstring.  Host side as in the reference
        (python `random` shuffles and neighbour sampling, python sets); the arithmetic -- segment mean of sampled neighbour
        rows, the two projections and their gradients, Adam -- runs in libggad_hip.so."""
        from .fullgraph import FlatAdam
        args = self.args
        dev = self._cuda_device()
        feat_data, adj_lists = self.dataset["feat_data"], self.dataset["adj_lists"]
        n, f = feat_data.shape
        nn.Embedding(n, f)                                            # RNG consumption of :263
        if isinstance(adj_lists, tuple):
            adj_lists = DeviceGraph(adj_lists[0], adj_lists[1], dev)
        features = FeatureTable(torch.FloatTensor(np.asarray(feat_data, dtype=np.float32)))
        agg_sage = MeanAggregator(features, cuda=True)
        if bool(getattr(args, "sage_device", False)):
            return self._train_sage_device(dev, adj_lists, features, agg_sage)
        enc_sage = Encoder(features, f, args.emb_size, adj_lists, agg_sage, gcn=False, cuda=True)
        enc_sage.num_samples = 5                                       # :291 (a new attribute: the encoder keeps num_sample = 10)
        gnn_model = GraphSage(2, enc_sage).to(dev)
        features.to(dev)
        optimizer = FlatAdam([p for p in gnn_model.parameters() if p.requires_grad], lr=args.lr, weight_decay=args.weight_decay)
        self.model = gnn_model
        self.sage_losses = []
        return train_labelled(args, self.dataset, gnn_model, list(self.dataset["idx_train"]), list(self.dataset["idx_anomaly"]),
                              shuffle=random.shuffle, join=operator.add, step=_autograd_step(gnn_model, optimizer),
                              report=_report_sage, sweep=self._test_graphsage, log=self.sage_losses)

    def _train_sage_device(self, dev, adj_lists, features, agg_sage):
        """`_train_sage` with config key `sage_device: true` (sage_device.py): the adjacency is a `DeviceGraph` (a (rowptr, col)
        pair as it is, a dict of sets through `DeviceGraph.from_adj_lists`), ONE native generator continues python's `random`
        stream for the epoch shuffle, the pool shuffle and the neighbour samples, and a step is one sampler call, one upload and the
        fused kernels of csrc/sage.hip; a validation sweep is one sampler call and one forward launch.  Same loop, same prints,
        same checkpoints.  The draws equal the set path's bit for bit for CSR input and for dicts whose sets were filled in
        ascending id order; the stream is handed back to `random` before this returns.

        Config key `sage_epoch: true` (needs `sage_device`; sage_epoch.py): an epoch is one native sampler call, one upload and one
        replayed graph of three launches per step, Adam inside the last; `self.sage_epoch` is the runner.  Same draws, losses,
        weights, optimiser state, prints and checkpoints as the step path, bit for bit."""
        from .fullgraph import FlatAdam
        from .sage_device import SageDevice
        args = self.args
        n, f = self.dataset["feat_data"].shape
        adj_lists = device_graph(adj_lists, n, dev)
        idx_sweep = list(self.dataset["idx_test"])          # validation runs on the test split (:260-261)
        rng = PyCompatRandom.from_python_state(random.getstate())
        try:
            sage = SageDevice(adj_lists, features, f, args.emb_size, 10, rng=rng)      # the encoder's default num_sample (:291 sets
            enc_sage = Encoder(features, f, args.emb_size, adj_lists, agg_sage, gcn=False, cuda=True, sage_device=sage)   # another name)
            enc_sage.num_samples = 5
            gnn_model = GraphSage(2, enc_sage).to(dev)
            features.to(dev)
            optimizer = FlatAdam([p for p in gnn_model.parameters() if p.requires_grad], lr=args.lr, weight_decay=args.weight_decay)
            self.model = gnn_model
            idx_train = np.array(list(self.dataset["idx_train"]), dtype=np.int64)
            idx_anomaly = np.array(list(self.dataset["idx_anomaly"]), dtype=np.int64)
            self.sage_losses = []
            self.sage_epoch = epoch_fn = None
            if bool(getattr(args, "sage_epoch", False)):
                from .sage_epoch import SageEpoch
                self.sage_epoch = SageEpoch(sage, enc_sage.weight, gnn_model.weight, optimizer, idx_train, idx_anomaly,
                                            self.dataset["labels"], args.batch_size, int(getattr(args, "n_pseudo", 50)),
                                            int(getattr(args, "num_batches", 150)))

                def epoch_fn(epoch):
                    # what the stream is asked for after this epoch is drawn while the device trains it: the validation sweep, the
                    # next epoch, or -- after the last epoch -- the test sweep (a restored checkpoint changes no draw)
                    if epoch % args.valid_epochs != 0 and epoch + 1 < args.num_epochs:
                        return self.sage_epoch.run_epoch("epoch")
                    return self.sage_epoch.run_epoch(lambda: sage.presample(idx_sweep))
            return train_labelled(args, self.dataset, gnn_model, idx_train, idx_anomaly, shuffle=rng.shuffle,
                                  join=lambda a, b: np.concatenate([a, b]), step=_autograd_step(gnn_model, optimizer),
                                  report=_report_sage, sweep=self._test_graphsage, log=self.sage_losses, epoch_fn=epoch_fn)
        finally:
            random.setstate(rng.to_python_state())       # hand the stream back to python `random`

    def _train_pcgnn(self):
        """`model: 'PCGNN'`: IntraAgg x 3 -> InterAgg -> PCALayer(2, inter1, alpha) as `src/model_handler.py:269-277,287-288` builds
        them, trained by the loop of `:310-370` and validated / tested through the `test_pcgnn` call sites of `:392,411`.  The reference
        cannot run this branch: its handler hands the homogeneous adjacency to `InterAgg`, which indexes three relations
        (`src/layers.py:43-45`), and `test_pcgnn` is not defined anywhere.  Two repairs, nothing else:
        (1) `adj_lists` must be a list of THREE relation adjacencies -- config key `relations` (dicts of sets / (rowptr, col) pairs),
        or `data = ([r1, r2, r3], feat, labels)`; (2) `test_pcgnn` = `test_sage`'s protocol on `PCALayer.to_prob(nodes, labels,
        train_flag=False)[0][:, 1]` (the class-1 GNN score).  No vectors of the reference exist for this loop (it never ran): the
        modules are pinned (tests/golden/minibatch_pcgnn.npz), the loop is checked for self-consistency (tests/test_dropin_gpu.py).
        Config key `pcgnn_device` (default False): the relations become `DeviceGraph`s and `InterAgg` runs from the CSR in HBM
        (pcgnn_device.py); without it nothing here changes.  Config key `pcgnn_fused` (default False, needs `pcgnn_device`): the head
        behind the relations and `PCALayer.loss` / `to_prob` run in csrc/pcgnn_head.hip (`PcgnnHeadFn`)."""
        from .fullgraph import FlatAdam
        from .layers import InterAgg, IntraAgg, PCALayer
        from . import synth
        args = self.args
        dev = self._cuda_device()
        feat_data = self.dataset["feat_data"]
        relations = getattr(args, "relations", None)
        if relations is None and isinstance(self.dataset["adj_lists"], (list, tuple)) and len(self.dataset["adj_lists"]) == 3 \
                and not isinstance(self.dataset["adj_lists"][0], np.ndarray):
            relations = self.dataset["adj_lists"]
        if relations is None or len(relations) != 3:
            raise ValueError("model 'PCGNN' needs three relation graphs: config key `relations` = [r1, r2, r3] "
                             "(dict of neighbour sets, or (rowptr, col)); the reference's branch never ran (its handler passes one)")
        if bool(getattr(args, "pcgnn_device", False)):
            # relations stay CSR in HBM (pcgnn_device.py): no dict of sets is built; `InterAgg` checks every relation once
            adjs = [device_graph(r, feat_data.shape[0], dev) for r in relations]
        else:
            adjs = [synth.csr_to_adj_lists(r[0], r[1]) if isinstance(r, tuple) else r for r in relations]
        idx_train = list(self.dataset["idx_train"])
        n, f = feat_data.shape
        nn.Embedding(n, f)                                            # RNG consumption of :263
        features = FeatureTable(torch.FloatTensor(np.asarray(feat_data, dtype=np.float32)))
        train_pos = [i for i in idx_train if self.dataset["labels"][i] == 1]          # pos_neg_split(idx_train, y_train)[0]
        rho, alpha = float(getattr(args, "rho", 0.5)), float(getattr(args, "alpha", 2))
        intras = [IntraAgg(features, f, args.emb_size, train_pos, rho, cuda=True) for _ in range(3)]         # :270-275
        inter1 = InterAgg(features, f, args.emb_size, train_pos, adjs, intras, inter=args.multi_relation, cuda=True,      # :276-277
                          fused=bool(getattr(args, "pcgnn_fused", False)))
        gnn_model = PCALayer(2, inter1, alpha).to(dev)                 # :288
        features.to(dev)
        optimizer = FlatAdam([p for p in gnn_model.parameters() if p.requires_grad], lr=args.lr, weight_decay=args.weight_decay)
        self.model = gnn_model
        self.pcgnn_losses = []

        def report(epoch, means, epoch_time):
            print(f"Epoch: {epoch}, loss: {means[0]}, loss_constraint: {means[1]}, time: {epoch_time}s")
        return train_labelled(args, self.dataset, gnn_model, idx_train, list(self.dataset["idx_anomaly"]), shuffle=random.shuffle,
                              join=operator.add, step=_autograd_step(gnn_model, optimizer), report=report, sweep=self._test_pcgnn,
                              log=self.pcgnn_losses)

    @staticmethod
    def _test_pcgnn(test_cases, labels, model, batch_size, thres=0.5):
        """What the undefined `test_pcgnn` of `src/model_handler.py:392,411` has to be for that call to work: `test_sage`'s protocol
        (`src/utils.py:207-247`) on the class-1 GNN score of `PCALayer.to_prob(nodes, labels, train_flag=False)`."""
        test_cases = list(test_cases)
        labels = np.asarray(labels)
        probs = []
        with torch.no_grad():
            for it in range(int(len(test_cases) / batch_size) + 1):
                lo, hi = it * batch_size, min((it + 1) * batch_size, len(test_cases))
                if hi <= lo:
                    continue
                chunk = test_cases[lo:hi]
                dev = next(model.parameters()).device
                gnn_prob, _ = model.to_prob(chunk, torch.as_tensor(labels[lo:hi], device=dev).long(), train_flag=False)
                probs.append(gnn_prob[:, 1])
        return sweep_report(torch.cat(probs), labels, thres)

    @staticmethod
    def _test_graphsage(test_cases, labels, model, batch_size, thres=0.5):
        """`test_sage` (`src/utils.py:207-247`) for the two-class GraphSage head: `to_prob(nodes)` (repair 2: one argument), the
        score of a node = its class-1 probability."""
        test_cases = list(test_cases)
        probs = []
        with torch.no_grad():
            if getattr(model.enc, "device_path", None) is not None:
                # the device path scores a sweep in one sampler call and one forward launch: the stream, and so every sample, depends on
                # the order of the rows only
                probs.append(model.to_prob(test_cases)[:, 1])
            else:
                for it in range(int(len(test_cases) / batch_size) + 1):
                    chunk = test_cases[it * batch_size:min((it + 1) * batch_size, len(test_cases))]
                    if not chunk:
                        continue
                    probs.append(model.to_prob(chunk)[:, 1])
        return sweep_report(torch.cat(probs), labels, thres)
