#!/usr/bin/env python3
"""Entry point of the DGraph mini-batch GGAD run:  cd src && python main.py [--config dgraph.yml] [--multi_run]

Mirrors the reference's `src/main.py` CLI (`--config`, `--multi_run`, YAML keys of dgraph.yml) on top of the
MI355X-native `ggad_amd.model_handler.ModelHandler`.  For N GPUs launch it with
`python -m torch.distributed.run --nproc-per-node N main.py ...`: batches are then sharded over the ranks."""
import argparse
import itertools
import os
import sys
import time

import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ggad_amd.model_handler import ModelHandler  # noqa: E402


def set_random_seed(seed):
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)


def print_config(config):
    bar = "**************** MODEL CONFIGURATION ****************"
    print(bar)
    for key in sorted(config):
        if key == "data":              # in-memory dataset handed over by --synthetic: not a setting
            continue
        print("{}{} -->   {}".format(key, " " * (24 - len(key)), config[key]))
    print(bar)


def expand_grid(config):
    """Every list-valued key is a swept hyper-parameter; yields one flat config per combination."""
    swept = [k for k, v in config.items() if isinstance(v, list)]
    fixed = {k: v for k, v in config.items() if k not in swept}
    for combo in itertools.product(*(config[k] for k in swept)):
        cfg = dict(fixed)
        cfg.update(dict(zip(swept, combo)))
        yield swept, cfg


HANDLER = ModelHandler


def use_handler(name):
    """The reference switches models by editing its import of `ModelHandler` (`src/main.py:11`); here it is a flag."""
    global HANDLER
    if name == "dominant":
        from ggad_amd.model_handler_dominate import ModelHandler as H
    elif name == "anomalydae":
        from ggad_amd.model_handler_anomalydae import ModelHandler as H
    elif name == "aegis":
        from ggad_amd.model_handler_aegis import ModelHandler as H
    else:
        H = ModelHandler
    HANDLER = H


SCORE = None          # --score CKPT: score from this checkpoint instead of training
SCORE_IDS = None      # --score_ids FILE.npy: the int64 ids --score sweeps and ranks (no labels) instead of the test split
COMPARE = None        # --compare CKPT_B: with --score, DeLong's paired test of the two checkpoints' test AUROCs


def run_once(config):
    set_random_seed(config["seed"])
    if SCORE is not None:
        handler = HANDLER(config)
        if SCORE_IDS is not None:
            handler.score(SCORE, ids=np.asarray(np.load(SCORE_IDS), dtype=np.int64).reshape(-1))
        elif COMPARE is not None:
            handler.score(SCORE, compare=COMPARE)
        else:
            handler.score(SCORE)
        return handler.metrics
    return HANDLER(config).train()


def main(config):
    print_config(config)
    res = run_once(config)
    if res is None:            # the comparison models' handlers only print (src/model_handler_dominate.py:171)
        return
    f1_mac, f1_1, f1_0, auc, gmean = res
    print("F1-Macro: {}".format(f1_mac))
    print("AUC: {}".format(auc))
    print("G-Mean: {}".format(gmean))


def multi_run_main(config):
    print_config(config)
    results = []
    for i, (swept, cfg) in enumerate(expand_grid(config)):
        print("Running {}:\n".format(i))
        for k in swept:
            cfg["save_dir"] += "{}_{}_".format(k, cfg[k])
        print(cfg["save_dir"])
        st = time.time()
        results.append(run_once(cfg))
        print("Running {} done, elapsed time {}s".format(i, time.time() - st))
    arr = np.array(results, dtype=np.float64)
    names = ["F1-Macro", "F1-binary-1", "F1-binary-0", "AUC", "G-Mean"]
    for j in (0, 3, 4):
        print("{}: {}".format(names[j], arr[:, j].tolist()))
    for j, name in enumerate(names):
        std = arr[:, j].std(ddof=1) if len(arr) > 1 else float("nan")
        print("{}: {}+{}".format(name, arr[:, j].mean(), std))


def init_distributed():
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        torch.distributed.init_process_group("nccl")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, default="dgraph.yml", help="")
    ap.add_argument("--multi_run", action="store_true", help="flag: multi run")
    ap.add_argument("--synthetic", action="store_true",
                    help="no ../data/dgraphfin.npz here: train on a synthetic graph of DGraph-Fin's size (power-law degrees, "
                         "U[0,1) features, 0.42 %% anomalies) built from the config's seed")
    ap.add_argument("--synthetic_entries", type=int, default=73105508, help="directed entries of the synthetic graph "
                    "(73.1 M = BASELINE's figure; 8600000 = the public dataset's average degree 2.3)")
    ap.add_argument("--num_epochs", type=int, default=None, help="override the config's num_epochs")
    ap.add_argument("--handler", choices=["ggad", "dominant", "anomalydae", "aegis"], default="ggad",
                    help="which ModelHandler drives the run: GGAD (default) or one of the mini-batch comparison models")
    ap.add_argument("--score", type=str, default=None, metavar="CKPT",
                    help="--handler ggad only: no training; load this checkpoint (the .pkl a run saved), sweep the test split of the "
                         "config's seed, print its report and, with top_k > 0, the ranked list")
    ap.add_argument("--top_k", type=int, default=None, help="override the config's top_k (rank the K highest test scores; 0 = off)")
    ap.add_argument("--top_k_out", type=str, default=None, help="override the config's top_k_out (.npz of the ranked list)")
    ap.add_argument("--explain", type=int, default=None, metavar="M",
                    help="override the config's explain (with top_k: explain every ranked node exactly, per feature and per neighbour, "
                         "listing the M signed-greatest neighbour contributions; 0 = off)")
    ap.add_argument("--explain_out", type=str, default=None, metavar="F", help="override the config's explain_out (.npz of the explanation)")
    ap.add_argument("--rank_wide", action="store_true", default=None,
                    help="override the config's rank_wide (with eval_cache: exact rank metrics in HIP above 8,192 positives)")
    ap.add_argument("--top_k_wide", action="store_true", default=None,
                    help="override the config's top_k_wide (with top_k: rank through csrc/topk.hip, K above 16384 up to 4194304)")
    ap.add_argument("--thres_select", type=str, default=None, metavar="CRIT",
                    help="override the config's thres_select (choose the alert threshold on the device: f1, f1_macro, gmean, "
                         "precision:X, fpr:X)")
    ap.add_argument("--score_ids", type=str, default=None, metavar="FILE.npy",
                    help="with --score: sweep and rank this int64 id list (np.save) instead of the test split; no labels, so no report: "
                         "with top_k it is the ranked list of these ids (every node of the graph, for instance)")
    ap.add_argument("--auc_ci", type=float, nargs="?", const=0.95, default=None, metavar="LEVEL",
                    help="override the config's auc_ci (--handler ggad: after the closing test sweep, and with --score, print the test "
                         "AUROC with DeLong's standard error and the normal interval at LEVEL, default 0.95; 0 = off)")
    ap.add_argument("--ap_ci", type=float, nargs="?", const=0.95, default=None, metavar="LEVEL",
                    help="override the config's ap_ci (--handler ggad: after the closing test sweep, and with --score, print the test "
                         "average precision and AUROC with the percentile intervals of a stratified bootstrap at LEVEL, default 0.95; "
                         "0 = off)")
    ap.add_argument("--boot_reps", type=int, default=None, metavar="B", help="override the config's boot_reps (replicates of --ap_ci and --compare_ap)")
    ap.add_argument("--boot_seed", type=int, default=None, metavar="S", help="override the config's boot_seed (Philox seed of --ap_ci and --compare_ap)")
    ap.add_argument("--compare", type=str, default=None, metavar="CKPT_B",
                    help="with --score CKPT: score the test split under CKPT_B too and print DeLong's paired test of the two AUROCs")
    ap.add_argument("--compare_ap", type=float, nargs="?", const=0.95, default=None, metavar="LEVEL",
                    help="override the config's compare_ap (with --score CKPT --compare CKPT_B: behind the [compare] line, print the paired "
                         "stratified bootstrap of the two average precisions, the interval of the difference at LEVEL, default 0.95; "
                         "0 = off)")
    a = ap.parse_args()
    if a.compare is not None and a.score is None:
        ap.error("--compare CKPT_B compares with the checkpoint of --score CKPT: it needs --score")
    if a.compare is not None and a.score_ids is not None:
        ap.error("--compare tests two AUROCs against each other: the ids of --score_ids carry no labels")
    if a.compare_ap is not None and a.compare is None:
        ap.error("--compare_ap tests the average precisions of --score CKPT and --compare CKPT_B: it needs --compare")
    if a.compare_ap is not None and not 0.0 <= a.compare_ap < 1.0:
        ap.error("--compare_ap LEVEL: a confidence level inside (0, 1), as in --compare_ap 0.9 (0 = off)")
    if a.auc_ci and a.handler != "ggad":
        ap.error("--auc_ci serves --handler ggad only")
    if a.auc_ci is not None and not 0.0 <= a.auc_ci < 1.0:
        ap.error("--auc_ci LEVEL: a confidence level inside (0, 1), as in --auc_ci 0.9 (0 = off)")
    if a.ap_ci and a.handler != "ggad":
        ap.error("--ap_ci serves --handler ggad only")
    if a.ap_ci is not None and not 0.0 <= a.ap_ci < 1.0:
        ap.error("--ap_ci LEVEL: a confidence level inside (0, 1), as in --ap_ci 0.9 (0 = off)")
    if a.boot_reps is not None and a.boot_reps < 1:
        ap.error("--boot_reps B: at least one replicate")
    if a.boot_seed is not None and not 0 <= a.boot_seed < 1 << 64:
        ap.error("--boot_seed S: an unsigned 64-bit integer")
    if a.score_ids is not None and a.score is None:
        ap.error("--score_ids names the ids --score CKPT sweeps: it needs --score")
    if a.score is not None and a.handler != "ggad":
        ap.error("--score serves --handler ggad only")
    if a.score is not None and a.multi_run:
        ap.error("--score scores one checkpoint: it does not go with --multi_run")
    with open(a.config, "r") as fh:
        cfg = yaml.load(fh, Loader=yaml.FullLoader)
    if a.num_epochs is not None:
        cfg["num_epochs"] = a.num_epochs
    if a.top_k is not None:
        cfg["top_k"] = a.top_k
    if a.top_k_out is not None:
        cfg["top_k_out"] = a.top_k_out
    if a.explain is not None:
        cfg["explain"] = a.explain
    if a.explain_out is not None:
        cfg["explain_out"] = a.explain_out
    if a.rank_wide is not None:
        cfg["rank_wide"] = a.rank_wide
    if a.top_k_wide is not None:
        cfg["top_k_wide"] = a.top_k_wide
    if a.thres_select is not None:
        cfg["thres_select"] = a.thres_select
    if a.auc_ci is not None:
        cfg["auc_ci"] = a.auc_ci
    for key in ("ap_ci", "boot_reps", "boot_seed", "compare_ap"):
        if getattr(a, key) is not None:
            cfg[key] = getattr(a, key)
    SCORE, SCORE_IDS, COMPARE = a.score, a.score_ids, a.compare
    use_handler(a.handler)
    init_distributed()
    torch.set_num_threads(min(8, os.cpu_count() or 1))        # host tensors are tiny here; 128 intra-op threads only add jitter
    if a.synthetic:
        from ggad_amd import synth
        dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
        n = 3700550
        rowptr, col = synth.make_graph_torch(n, a.synthetic_entries, cfg["seed"], dev, kind="powerlaw", max_degree=2000)
        cfg["data"] = ((rowptr, col), synth.make_features(n, 17, cfg["seed"]),
                       synth.make_labels(n, 15509.0 / 3700550.0, cfg["seed"]).astype(np.int32))
    (multi_run_main if a.multi_run else main)(cfg)
