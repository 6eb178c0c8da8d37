"""What the full-graph entry scripts (`run.py`, `ocgnn.py`, `anomalyDAE.py`, `aegis.py`, `gaan.py`, `dominant.py`, `tam.py`) share:
the command line the reference's scripts have in common, the loader (a `.mat` file or a synthetic graph of the published size),
feature / adjacency preparation, process setup, the capture of the training epoch as a hipGraph (`capture` / `CapturedEpoch`, which the
mini-batch loop of `model_handler_dominate.py` uses too), the per-epoch noise feed of `gaan.py` / `aegis.py`, and the closing prints.  What differs between the scripts -- their defaults, print cadence and timed window
-- stays in the scripts.
"""
from __future__ import annotations

import argparse
import gc
import os
import random
import sys
from typing import NamedTuple

import numpy as np
import scipy.sparse as sp
import torch

from . import synth
from .fullgraph import FullGraphAdj
from .metrics import average_precision, roc_auc
from .utils import load_mat, normalize_adj, preprocess_features, split_nodes

# published sizes (reference README.md:53-58): nodes, directed entries, features, anomaly rate
SIZES = {"reddit": (10984, 168016, 64, 0.033), "Amazon": (11944, 4398392, 25, 0.069), "photo": (7535, 119043, 745, 0.092),
         "t_finance": (39357, 21222543, 10, 0.046), "elliptic": (46564, 73248, 93, 0.098)}
NO_GRAPH_HELP = "do not replay a captured hipGraph of the training epoch"
DEVICE_NOISE_HELP = ("draw the per-epoch noise on the device from torch's own CPU stream (ggad_amd.rng): the draw is the first node "
                     "of the captured epoch; values agree with the host's to float32 rounding")


# ------------------------------------------------------------------------------------------------ command line
def make_parser(dataset, no_graph_help=NO_GRAPH_HELP, device_noise_help=None, sampling=True):
    """The options the reference's full-graph scripts share, plus `--synthetic` / `--device` / `--quiet` / `--no_graph` and -- where
    `device_noise_help` is given -- `--device_noise`.  `sampling`: `--batch_size` / `--subgraph_size`, which the reference's baselines
    carry and its `run.py` does not.  A script adds its own options to the returned parser."""
    p = argparse.ArgumentParser(description="")
    p.add_argument("--dataset", type=str, default=dataset)
    p.add_argument("--lr", type=float)
    p.add_argument("--weight_decay", type=float, default=0.0)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--embedding_dim", type=int, default=300)
    p.add_argument("--num_epoch", type=int)
    p.add_argument("--drop_prob", type=float, default=0.0)
    if sampling:
        p.add_argument("--batch_size", type=int, default=300)
        p.add_argument("--subgraph_size", type=int, default=4)
    p.add_argument("--readout", type=str, default="avg")
    p.add_argument("--auc_test_rounds", type=int, default=256)
    p.add_argument("--negsamp_ratio", type=int, default=1)
    p.add_argument("--synthetic", action="store_true", help="generate a graph of the dataset's size instead of loading ./dataset/*.mat")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--no_graph", action="store_true", help=no_graph_help)
    if device_noise_help is not None:
        p.add_argument("--device_noise", action="store_true", help=device_noise_help)
    return p


def parse_with_defaults(p, argv, lr, epochs, fallback=None):
    """Parse, then let the script's per-dataset `lr` / `epochs` dictionaries fill what the command line left open.  A dataset outside
    them is an error (the reference's scripts leave the value None there), unless `fallback` = (lr, num_epoch) says what it gets."""
    a = p.parse_args(argv)
    fb_lr, fb_epochs = fallback or (None, None)
    if a.lr is None:
        a.lr = lr.get(a.dataset, fb_lr)
    if a.num_epoch is None:
        a.num_epoch = epochs.get(a.dataset, fb_epochs)
    if a.lr is None or a.num_epoch is None:
        p.error("no default lr / num_epoch for dataset {!r}: pass --lr and --num_epoch".format(a.dataset))
    return a


def add_select_options(p):
    """`--select` / `--save` / `--score` / `--top_k` / `--top_k_out` / `--top_k_wide`: keep the epoch with the best validation metric (ggad_amd.select),
    write a checkpoint, score a graph from one and rank its test nodes.  All off by default, and an option that is not given leaves NO
    attribute behind (`argparse.SUPPRESS`): the namespace of a command line without them is the one the script had before they existed
    (tests/test_fullgraph_script_cpu.py pins it), and a caller's hand-made namespace needs none of them.  Read them with
    `select_options`; `check_select_options` after parsing."""
    off = argparse.SUPPRESS
    p.add_argument("--select", choices=["auroc", "ap"], default=off,
                   help="validate every epoch on idx_val inside the (captured) epoch and keep the weights of the epoch with the best "
                        "AUROC / AP on the device; the training trajectory is unchanged")
    p.add_argument("--save", type=str, default=off, metavar="PATH",
                   help="write the weights to PATH (torch.save): the best epoch's with --select, else the last epoch's")
    p.add_argument("--score", type=str, default=off, metavar="CKPT",
                   help="no training: load the weights of CKPT (written by --save), score the graph and report on idx_test")
    p.add_argument("--top_k", type=int, default=off, help="with --score: rank the K highest-scoring test nodes (precision / recall @ K)")
    p.add_argument("--top_k_out", type=str, default=off, metavar="F.npz", help="with --score --top_k K: write the ranked list to F.npz")
    p.add_argument("--top_k_wide", action="store_true", default=off,
                   help="with --score --top_k K: rank through csrc/topk.hip, K above 16384 up to 4194304 (a whole test split)")
    return p


def select_options(a):
    """(select, save, score, top_k, top_k_out) of a namespace, with what "not given" means: None, None, None, 0, ""."""
    return (getattr(a, "select", None), getattr(a, "save", None), getattr(a, "score", None), int(getattr(a, "top_k", 0) or 0),
            str(getattr(a, "top_k_out", "") or ""))


def top_k_wide_option(a):
    """`--top_k_wide` of a namespace (False when not given); apart from `select_options`, whose five values callers unpack."""
    return bool(getattr(a, "top_k_wide", False))


def check_select_options(p, a):
    select, save, score, top_k, top_k_out = select_options(a)
    if top_k_wide_option(a) and not top_k:
        p.error("--top_k_wide chooses the kernels of --top_k K: it needs --top_k K with K > 0")
    if score and select:
        p.error("--score does no training: it cannot be combined with --select")
    if score and save:
        p.error("--score does no training: there is nothing for --save to write")
    if (top_k or top_k_out) and not score:
        p.error("--top_k / --top_k_out rank the scores of --score CKPT")
    if top_k < 0 or (top_k_out and not top_k):
        p.error("--top_k_out needs --top_k K with K > 0")
    return a


def add_threshold_options(p):
    """`--threshold CRIT` (run.py only): after training, choose the alert threshold on idx_val on the device (`metrics.operating_point`)
    and report idx_test at it.  Off by default and, like the options of `add_select_options`, absent from the namespace when not
    given.  Read it with `threshold_option`; `check_threshold_options` after parsing."""
    p.add_argument("--threshold", type=str, default=argparse.SUPPRESS, metavar="CRIT",
                   help="choose the alert threshold on idx_val after training: f1, f1_macro, gmean, precision:X (the greatest recall at a "
                        "precision of at least X) or fpr:X (at a false-positive rate of at most X); --save keeps it, --score reports at it")
    return p


def threshold_option(a):
    """`--threshold` of a namespace: the criterion's text, or None when not given."""
    return getattr(a, "threshold", None) or None


def check_threshold_options(p, a):
    crit = threshold_option(a)
    if crit is None:
        return a
    if select_options(a)[2]:
        p.error("--score reports at the threshold its checkpoint carries: --threshold chooses one at training time")
    from .metrics import parse_criterion
    try:
        parse_criterion(crit)
    except ValueError as exc:
        p.error("--threshold: {}".format(exc))
    return a


def choose_threshold(crit, scores, idx_val, ano_label, dev):
    """`--threshold CRIT` after training: the operating point of the (N,) device `scores` on `idx_val`, printed as one `[threshold]`
    line; returns the `metrics.OperatingPoint`."""
    from .metrics import operating_point, parse_criterion
    name, param = parse_criterion(crit)
    idx = np.asarray(idx_val, dtype=np.int64)
    y8 = np.asarray(ano_label).reshape(-1)[idx].astype(np.uint8)
    val = scores.detach().float().index_select(0, torch.as_tensor(idx, device=dev))
    op = operating_point(val, torch.from_numpy(y8).to(dev), name, param, pos_cap=max(1, int(np.count_nonzero(y8 == 1))))
    print("[threshold] {} on {} validation nodes: threshold {!r} value {!r} tp {} fp {} fn {} tn {} ({} candidates{})".format(
        crit, idx.size, op.thres, op.value, op.tp, op.fp, op.fn, op.tn, op.n_candidates,
        "" if op.feasible else "; none meets the constraint: no node alerts"))
    return op


def print_threshold_test(test_scores, y_dev, thres, alerts=False):
    """One `[threshold] test` line: the confusion counts, F1-macro and G-mean of `score >= thres` on the test nodes (`alerts`: and how
    many of them alert); returns the dict of `metrics._confusion_scores`."""
    from .metrics import _confusion_scores
    pred, pos = test_scores >= thres, y_dev == 1
    c = _confusion_scores(int((pred & pos).sum()), int((pred & ~pos).sum()), int((~pred & pos).sum()), int((~pred & ~pos).sum()))
    print("[threshold] test at {!r}: tp {} fp {} fn {} tn {} F1-macro {!r} G-mean {!r}".format(
        float(thres), c["tp"], c["fp"], c["fn"], c["tn"], c["f1_macro"], c["gmean"]))
    if alerts:
        print("alerts: {} of {} test nodes".format(c["tp"] + c["fp"], test_scores.numel()))
    return c


def add_compare_options(p):
    """`--auc_ci [LEVEL]` / `--compare CKPT_B` / `--compare_ap [LEVEL]` (run.py only): the test AUROC with DeLong's standard error and
    interval (`metrics.auc_ci`), DeLong's paired test of two checkpoints' AUROCs on idx_test (`metrics.compare_auc`) and, with it,
    the paired bootstrap of their average precisions (`metrics.compare_ap`; `--boot_reps` / `--boot_seed` of `add_bootstrap_options`).
    Off by default and, like the options of `add_select_options`, absent from the namespace when not given.  Read them with
    `compare_options` and `compare_ap_option`; `check_compare_options` after parsing."""
    p.add_argument("--auc_ci", type=float, nargs="?", const=0.95, default=argparse.SUPPRESS, metavar="LEVEL",
                   help="after training, or with --score: the AUROC on idx_test with DeLong's standard error and the normal interval at "
                        "LEVEL (default 0.95), from exact counts on the device")
    p.add_argument("--compare", type=str, default=argparse.SUPPRESS, metavar="CKPT_B",
                   help="with --score CKPT: score idx_test under CKPT_B too and test the two AUROCs against each other (DeLong's paired "
                        "z and two-sided p)")
    p.add_argument("--compare_ap", type=float, nargs="?", const=0.95, default=argparse.SUPPRESS, metavar="LEVEL",
                   help="with --score CKPT --compare CKPT_B: test the two average precisions against each other too, by a paired "
                        "stratified bootstrap made on the device (interval of the difference at LEVEL, default 0.95, and two-sided p)")
    return p


def compare_options(a):
    """(auc_ci level or None, compare path or None) of a namespace."""
    return getattr(a, "auc_ci", None) or None, getattr(a, "compare", None) or None


def compare_ap_option(a):
    """The level of `--compare_ap`, or None."""
    return getattr(a, "compare_ap", None) or None


def check_compare_options(p, a):
    level, other = compare_options(a)
    if hasattr(a, "compare_ap") and not 0.0 < float(a.compare_ap) < 1.0:
        p.error("--compare_ap LEVEL: a confidence level inside (0, 1), as in --compare_ap 0.9")
    if hasattr(a, "compare_ap") and not other:
        p.error("--compare_ap tests the average precisions of --score CKPT and --compare CKPT_B: it needs --compare")
    if hasattr(a, "auc_ci") and not 0.0 < float(a.auc_ci) < 1.0:
        p.error("--auc_ci LEVEL: a confidence level inside (0, 1), as in --auc_ci 0.9")
    if other and not select_options(a)[2]:
        p.error("--compare CKPT_B compares with the checkpoint of --score CKPT: it needs --score")
    return a


def _test_lists(scores, idx_test, ano_label, dev):
    """(float32 scores, uint8 labels, count of positives) of idx_test on the device, as the DeLong calls take them."""
    idx = np.asarray(idx_test, dtype=np.int64)
    y8 = np.asarray(ano_label).reshape(-1)[idx].astype(np.uint8)
    return (scores.detach().float().index_select(0, torch.as_tensor(idx, device=dev)).contiguous(), torch.from_numpy(y8).to(dev),
            max(1, int(np.count_nonzero(y8 == 1))))


def print_auc_ci(level, scores, idx_test, ano_label, dev):
    """`--auc_ci LEVEL`: one `[auc_ci]` line for the (N,) device `scores` on idx_test; returns the `metrics.AucInterval`."""
    from .metrics import auc_ci, format_auc_ci
    s, y, cap = _test_lists(scores, idx_test, ano_label, dev)
    ci = auc_ci(s, y, level, pos_cap=cap)
    print(format_auc_ci(ci))
    return ci


def add_bootstrap_options(p):
    """`--ap_ci [LEVEL]`, `--boot_reps B`, `--boot_seed S` (run.py only): the test average precision and AUROC with the percentile
    intervals of a stratified bootstrap (`metrics.ap_ci`); B and S also serve `--compare_ap`.  Off by default and absent from the
    namespace when not given.  Read them with `bootstrap_options`; `check_bootstrap_options` after parsing."""
    p.add_argument("--ap_ci", type=float, nargs="?", const=0.95, default=argparse.SUPPRESS, metavar="LEVEL",
                   help="after training, or with --score: average precision and AUROC on idx_test with the percentile intervals of a "
                        "stratified bootstrap at LEVEL (default 0.95), every replicate made on the device")
    p.add_argument("--boot_reps", type=int, default=argparse.SUPPRESS, metavar="B", help="with --ap_ci or --compare_ap: replicates (default 1000)")
    p.add_argument("--boot_seed", type=int, default=argparse.SUPPRESS, metavar="S", help="with --ap_ci or --compare_ap: the Philox seed (default 0)")
    return p


def bootstrap_options(a):
    """(ap_ci level or None, replicates, seed) of a namespace."""
    return getattr(a, "ap_ci", None) or None, getattr(a, "boot_reps", 1000), getattr(a, "boot_seed", 0)


def check_bootstrap_options(p, a):
    if hasattr(a, "ap_ci") and not 0.0 < float(a.ap_ci) < 1.0:
        p.error("--ap_ci LEVEL: a confidence level inside (0, 1), as in --ap_ci 0.9")
    if (hasattr(a, "boot_reps") or hasattr(a, "boot_seed")) and not (hasattr(a, "ap_ci") or hasattr(a, "compare_ap")):
        p.error("--boot_reps and --boot_seed set the bootstrap of --ap_ci and --compare_ap: they need one of them")
    if hasattr(a, "boot_reps") and a.boot_reps < 1:
        p.error("--boot_reps B: at least one replicate")
    if hasattr(a, "boot_seed") and not 0 <= a.boot_seed < 1 << 64:
        p.error("--boot_seed S: an unsigned 64-bit integer")
    return a


def print_ap_ci(options, scores, idx_test, ano_label, dev):
    """`--ap_ci LEVEL`: one `[ap_ci]` line for the (N,) device `scores` on idx_test, `options` the triple of `bootstrap_options`;
    returns the `metrics.BootstrapInterval`."""
    from .metrics import ap_ci, format_ap_ci
    level, reps, seed = options
    s, y, cap = _test_lists(scores, idx_test, ano_label, dev)
    ci = ap_ci(s, y, level, reps, seed, pos_cap=cap)
    print(format_ap_ci(ci))
    return ci


def print_compare(scores_a, scores_b, idx_test, ano_label, dev):
    """`--compare`: one `[compare]` line for two (N,) device score tensors on idx_test; returns the `metrics.AucComparison`."""
    from .metrics import compare_auc, format_compare
    a, y, cap = _test_lists(scores_a, idx_test, ano_label, dev)
    b = _test_lists(scores_b, idx_test, ano_label, dev)[0]
    c = compare_auc(a, b, y, pos_cap=cap)
    print(format_compare(c))
    return c


def print_compare_ap(options, scores_a, scores_b, idx_test, ano_label, dev):
    """`--compare_ap LEVEL`: one `[compare_ap]` line for two (N,) device score tensors on idx_test, `options` = (level, replicates,
    seed); returns the `metrics.ApComparison`."""
    from .metrics import compare_ap, format_compare_ap
    level, reps, seed = options
    a, y, cap = _test_lists(scores_a, idx_test, ano_label, dev)
    b = _test_lists(scores_b, idx_test, ano_label, dev)[0]
    c = compare_ap(a, b, y, level, reps, seed, pos_cap=cap)
    print(format_compare_ap(c))
    return c


# ------------------------------------------------------------------------------------------------ checkpoints
def save_checkpoint(path, state_dict, args, n_in, nodes, epoch, value=None, threshold=None):
    """`torch.save({"state_dict", "meta"})`: the model's own state_dict (host copies; for `run.py` the reference's key names, so the
    reference's `Model` loads it) and what a later `--score` checks or reports.  `epoch`: the epoch the weights are from; `value`: the
    validation metric `--select` chose them by (None without).  `threshold`: the `metrics.OperatingPoint` of `--threshold`; only then
    does `meta` hold `thres` (a float that is exactly a float32), `thres_select` (the criterion as given) and `thres_value`."""
    meta = {"dataset": args.dataset, "n_in": int(n_in), "embedding_dim": int(args.embedding_dim), "nodes": int(nodes), "seed": int(args.seed),
            "epoch": int(epoch), "select": getattr(args, "select", None), "value": None if value is None else float(value)}
    if threshold is not None:
        meta.update(thres=float(threshold.thres), thres_select=str(threshold_option(args)), thres_value=float(threshold.value))
    torch.save({"state_dict": type(state_dict)((k, v.detach().cpu().clone()) for k, v in state_dict.items()), "meta": meta}, path)
    return meta


def load_checkpoint(path, n_in, embedding_dim):
    """The dict `save_checkpoint` wrote (tensors on the host).  Weights made for another `n_in` or `embedding_dim`: `ValueError` naming
    both values of each."""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(ck, dict) or "state_dict" not in ck or "meta" not in ck:
        raise ValueError("{}: not a checkpoint written by --save (no 'state_dict' / 'meta')".format(path))
    meta = ck["meta"]
    if int(meta["n_in"]) != int(n_in) or int(meta["embedding_dim"]) != int(embedding_dim):
        raise ValueError("{}: the checkpoint was written for n_in = {}, embedding_dim = {}; this graph and command line give n_in = {}, "
                         "embedding_dim = {}".format(path, meta["n_in"], meta["embedding_dim"], int(n_in), int(embedding_dim)))
    return ck


def score_from_checkpoint(args, model, score_fn, n_in, idx_test, ano_label, dev):
    """`--score CKPT [--top_k K] [--top_k_out F.npz] [--top_k_wide]`: load CKPT into `model` (strict), `score_fn()` -> the (N,) float32 device scores
    of all nodes (no training, no noise draw), the reference's two evaluation lines on `idx_test`, and -- with `--top_k` -- the K
    highest-scoring test nodes through `metrics.top_k`: precision / recall @ K printed, the list written by `write_ranked`.  Returns
    (scores, auc, ap, ranked or None)."""
    from .metrics import check_k, precision_recall_at, top_k, write_ranked
    _, _, path, k, k_out = select_options(args)
    wide = top_k_wide_option(args)
    if k:
        check_k(k, "--top_k", wide=wide)                                        # before anything is loaded or scored
    ck = load_checkpoint(path, n_in, args.embedding_dim)
    model.load_state_dict(ck["state_dict"], strict=True)
    model.eval()
    meta = ck["meta"]
    print("scoring with {} (dataset {}, epoch {}, select {}, value {})".format(path, meta["dataset"], meta["epoch"], meta["select"],
                                                                               meta["value"]))
    scores = score_fn()
    idx = np.asarray(idx_test, dtype=np.int64)
    idx_dev = torch.as_tensor(idx, device=dev)
    y = np.asarray(ano_label).reshape(-1)[idx]
    test_scores = scores.index_select(0, idx_dev)
    y_dev = torch.as_tensor(y.astype(np.int64), device=dev)
    auc, ap = print_eval(args.dataset, test_scores, y_dev)
    if meta.get("thres") is not None:                                           # a checkpoint of --threshold: the alert rule it carries
        print_threshold_test(test_scores, y_dev, meta["thres"], alerts=True)
    ranked = None
    if k:
        y8 = y.astype(np.uint8)
        ranked = top_k(test_scores, k, torch.from_numpy(y8).to(dev), idx_dev, wide=wide)
        prec, rec = precision_recall_at(ranked, ranked.m)
        print("top {} of {} test nodes: precision@{} {:.4f} recall@{} {:.4f} ({} positives among the test nodes, {} tied with the last "
              "rank left out)".format(ranked.m, idx.size, ranked.m, prec, ranked.m, rec, ranked.n_pos, ranked.tied_left_out))
        if k_out:
            write_ranked(k_out, ranked, y8)
            print("ranked list written to", k_out)
    return scores, auc, ap, ranked


# ------------------------------------------------------------------------------------------------ data
class Graph(NamedTuple):
    """What the reference's `load_mat` returns, less what no script reads."""
    adj: object
    feat: object
    ano_label: object
    all_idx: list
    idx_train: list
    idx_val: list
    idx_test: list
    normal_idx: list
    abn_idx: list


def synthetic_graph(dataset, seed):
    """(adj, feat, ano_label) of a power-law graph with the dataset's published size, from the seed alone."""
    n, ne, f, rate = SIZES[dataset]
    rowptr, col = synth.make_graph(n, ne, seed, kind="powerlaw", max_degree=max(64, n // 8), exact=True)
    adj = synth.csr_to_scipy(rowptr, col, n)
    feat = sp.lil_matrix(synth.make_features(n, f, seed))
    return adj, feat, synth.make_labels(n, rate, seed)


def load_graph(args) -> Graph:
    """`./dataset/<dataset>.mat`, or (`--synthetic`, or no such file) a synthetic graph of the same size; the split draws from
    python's `random` stream as the reference's `load_mat` does."""
    if args.synthetic or not os.path.exists("./dataset/{}.mat".format(args.dataset)):
        if not args.synthetic:
            print("./dataset/{}.mat not found: using a synthetic graph of the same size".format(args.dataset))
        adj, feat, ano = synthetic_graph(args.dataset, args.seed)
        return Graph(adj, feat, ano, *split_nodes(ano, args.dataset, verbose=not args.quiet))
    adj, feat, _, all_idx, idx_train, idx_val, idx_test, ano, _, _, normal_idx, abn_idx = load_mat(args.dataset)
    return Graph(adj, feat, ano, all_idx, idx_train, idx_val, idx_test, normal_idx, abn_idx)


def prepare(args, adj, feat, dev):
    """(full, feats, ft_size): the CSR adjacency pair in HBM (normalize_adj(A) + I and A + I, run.py:98-101) and the (1, N, F)
    feature tensor, row-normalised for the datasets the reference's scripts list."""
    # run.py:87, and the same list in ocgnn.py:124, anomalyDAE.py:80, aegis.py:77, gaan.py:77, dominant.py:84 (typo kept: never T-Finance)
    if args.dataset in ["Amazon", "tf_finace", "reddit", "elliptic"]:
        features = preprocess_features(feat)
    else:
        features = np.asarray(feat.todense())
    nb_nodes, ft_size = features.shape
    full = FullGraphAdj(normalize_adj(adj) + sp.eye(nb_nodes), adj + sp.eye(nb_nodes), dev)
    feats = torch.FloatTensor(np.asarray(features, dtype=np.float32)[np.newaxis]).to(dev)
    return full, feats, ft_size


def init_process(args, script_name, why="there is no CPU fallback", host_threads=8):
    """Seed numpy, torch (`torch.manual_seed` seeds every CUDA generator too) and `random`, insist on a GPU, make `--device` current;
    returns the device."""
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    random.seed(args.seed)
    if not torch.cuda.is_available():
        sys.exit("{} needs an MI355X: {}".format(script_name, why))
    if host_threads:
        # the host-side tensor work left is tiny (a noise draw per epoch at most): torch's default of one intra-op thread per core
        # (128 on the MI355X box) turns it into a 1-90 ms lottery on a loaded host
        torch.set_num_threads(min(host_threads, os.cpu_count() or 1))
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)      # the C-ABI launches on the CURRENT device's stream: it must be the one the tensors live on
    return dev


# ------------------------------------------------------------------------------------------------ the captured epoch
def capture(epoch_fn, before=None):
    """Capture one call of `epoch_fn` into a hipGraph: (graph, what `epoch_fn` returned -- the static outputs every replay refills).
    The capture itself executes nothing.  Nothing of earlier eager epochs' autograd graphs may survive into it (their AccumulateGrad
    nodes are bound to the default stream): `epoch_fn` returns detached tensors, `before` is where the caller zeroes its optimisers'
    gradients and drops whatever else holds a `grad_fn`, and the collection here frees what only a reference cycle kept alive."""
    if before is not None:
        before()
    gc.collect()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = epoch_fn()
    return graph, static


class CapturedEpoch:
    """A training loop's epoch: eager (allocations, plan caches, Adam state) until epoch `at`, captured there -- if `enabled` and
    `gate()` holds -- and replayed from that epoch on.  The mini-batch handlers pass `step` a `key` (the addresses of the epoch's
    plan buffers, which the captured launches hold): from epoch `at` on a key other than the one captured under is captured again."""

    def __init__(self, epoch_fn, *, enabled=True, at=2, before_capture=None, after_capture=None, gate=None):
        self.epoch_fn, self.enabled, self.at = epoch_fn, enabled, at
        self.before_capture, self.after_capture, self.gate = before_capture, after_capture, gate
        self.graph = self.static = self.key = None

    @property
    def captured(self) -> bool:
        return self.graph is not None

    def step(self, epoch, before_replay=None, key=None):
        """Run epoch `epoch`; returns what `epoch_fn` returns (once captured: the static outputs).  `before_replay` runs ahead of every
        replay, the capturing epoch's included: the place to refill a buffer the captured epoch reads.  Without a `key` the one
        capture is due at epoch `at`; with one, from `at` on whenever there is no graph or it was captured under another key."""
        due = self.graph is None and epoch == self.at if key is None else epoch >= self.at and (self.graph is None or key != self.key)
        if self.enabled and due and (self.gate is None or self.gate()):
            self.graph, self.static = capture(self.epoch_fn, self.before_capture)
            self.key = key
            if self.after_capture is not None:
                self.after_capture()
        if self.graph is None or key != self.key:
            return self.epoch_fn()
        if before_replay is not None:
            before_replay()
        self.graph.replay()
        return self.static


class NoiseFeed:
    """The `shape` standard-normal draw that the forward of `gaan.py` / `aegis.py` makes every epoch, for a captured epoch.  On the
    host (the default): eager epochs draw inside the model; the captured epoch reads `model.noise_override`, a buffer installed for
    the capture, which `before_replay` refills from the CPU generator in the reference's order.  `device_noise`: the CPU generator
    continues on the device (ggad_amd.rng) from here on, `epoch_fn` opens with the draw, and `close` hands the advanced state back."""

    def __init__(self, model, epoch_fn, shape, dev, device_noise):
        self.model, self.epoch_fn, self.shape, self.dev = model, epoch_fn, shape, dev
        self.mt = self.buf = None
        if device_noise:
            from .rng import DeviceMT
            self.mt = mt = DeviceMT.from_host(dev)
            self.buf = buf = model.noise_override = torch.zeros(*shape, device=dev)

            def with_draw():
                mt.randn_(buf)
                return epoch_fn()
            self.epoch_fn = with_draw

    def before_capture(self):
        if self.mt is None:
            self.buf = self.model.noise_override = torch.zeros(*self.shape, device=self.dev)

    def after_capture(self):
        if self.mt is None:
            self.model.noise_override = None

    def before_replay(self):
        if self.mt is None:
            self.buf.copy_(torch.randn(*self.shape))

    def close(self):
        if self.mt is not None:
            self.model.noise_override = None
            self.mt.to_host()


# ------------------------------------------------------------------------------------------------ prints
def print_captured():
    print("training epoch captured as a hipGraph", flush=True)


def print_eval(dataset, scores, y, prefix=""):
    """The reference's two evaluation lines (= sklearn's roc_auc_score / average_precision_score); returns (auc, ap).  `prefix`: put
    in front of both, for evaluations the reference does not make (so that they cannot be mistaken for its lines)."""
    auc = roc_auc(scores, y)
    print("{}Testing {} AUC:{:.4f}".format(prefix, dataset, auc))
    ap = average_precision(scores, y)
    print("{}Testing AP:".format(prefix), ap)
    return auc, ap


def print_median(epoch_times, n, note):
    if epoch_times:
        med = float(np.median(epoch_times))
        print("median epoch {:.3f} ms -> {:.1f} nodes/s (first epoch {:.1f} ms incl. {})".format(
            med * 1e3, n / med, epoch_times[0] * 1e3, note))
