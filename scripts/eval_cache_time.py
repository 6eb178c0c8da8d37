#!/usr/bin/env python3
"""What a validation costs with and without config key `eval_cache` (ggad_amd/eval_cache.py, csrc/rank_metrics.hip).

    python scripts/eval_cache_time.py [--nodes 3700550] [--entries 73105508] [--cases 1736598] [--reps 7] [--epochs 11]
                                      [--no-runs] [--out profiles/eval_cache_time_line.json]

On the DGraph-size synthetic graph of bench.py (power-law degrees, 17 features, emb 64), one process, a device synchronise around
every timed part, every part run `--warmup` times before it is timed, medians of `--reps` (all values are kept):

  sweep      `score_nodes(..., device=True)`: the uncached sweep (a plan per launch group of 2,048 slices of 150 ids, every time)
  resident   `ResidentSweep(...)` once (the same plans + the copies of their rows), then `scores()`: ONE score launch over the cache
  metrics    `binary_report` (two float64 device sorts, composed torch ops) against `rank_report` (four counting launches, one
             read-back) on the same scores and labels, alternating; their results are compared
  runs       wall seconds of `python main.py --synthetic --num_epochs N` with the key off and on, one process each, alternating
             `--run-reps` times (graph construction, training, the validations every 5th epoch and the final test are all inside)

Every figure stands beside the key-off figure of the same run.  Prints and writes one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ggad_amd import synth  # noqa: E402
from ggad_amd.dgraph import normalize_features  # noqa: E402
from ggad_amd.eval_cache import ResidentSweep  # noqa: E402
from ggad_amd.graph import DeviceGraph  # noqa: E402
from ggad_amd.graphsage import GCN, FeatureTable, GCNAggregator, GCNEncoder  # noqa: E402
from ggad_amd.metrics import binary_report, rank_report  # noqa: E402
from ggad_amd.sage_utils import score_nodes  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def series(fn, warmup, reps):
    for _ in range(warmup):
        timed(fn)
    return [timed(fn)[0] for _ in range(reps)]


def summary(xs):
    return dict(median_s=float(statistics.median(xs)), min_s=float(min(xs)), max_s=float(max(xs)), all_s=[float(x) for x in xs])


def whole_run(epochs, key, entries):
    """Wall seconds of one `main.py --synthetic` process with `eval_cache: key`."""
    import yaml
    with open(os.path.join(ROOT, "src", "dgraph.yml")) as fh:
        cfg = yaml.safe_load(fh)
    with tempfile.TemporaryDirectory() as tmp:
        cfg["eval_cache"] = bool(key)
        cfg["save_dir"] = os.path.join(tmp, "models") + "/"
        path = os.path.join(tmp, "cfg.yml")
        with open(path, "w") as fh:
            yaml.safe_dump(cfg, fh)
        t0 = time.perf_counter()
        p = subprocess.run([sys.executable, "main.py", "--config", path, "--synthetic", "--synthetic_entries", str(entries),
                            "--num_epochs", str(epochs)], cwd=os.path.join(ROOT, "src"), capture_output=True, text=True)
        dt = time.perf_counter() - t0
    if p.returncode != 0:
        sys.exit(f"main.py failed with code {p.returncode} (eval_cache {key}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    tail = [ln for ln in p.stdout.splitlines() if ln.startswith(("F1-Macro", "AUC", "G-Mean", "   GNN TP"))]
    return dt, tail[-4:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=3_700_550)
    ap.add_argument("--entries", type=int, default=73_105_508)
    ap.add_argument("--cases", type=int, default=1_736_598)
    ap.add_argument("--pos-rate", type=float, default=0.0042)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=11)
    ap.add_argument("--run-reps", type=int, default=1)
    ap.add_argument("--no-runs", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_cache_time.py needs an MI355X")
    dev = "cuda:0"
    rp, ci = synth.make_graph_torch(a.nodes, a.entries, 72, dev, kind="powerlaw", max_degree=2000)
    graph = DeviceGraph(rp, ci, dev)
    feat = normalize_features(synth.make_features(a.nodes, 17, 72)).astype(np.float32)
    features = FeatureTable(torch.from_numpy(feat))
    enc = GCNEncoder(features, 17, 64, graph, GCNAggregator(features, cuda=True), gcn=True, cuda=True)
    model = GCN(2, enc)
    enc.engine.sync_params()
    cases = np.random.default_rng(0).permutation(a.nodes)[:a.cases]
    y = (np.random.default_rng(1).random(len(cases)) < a.pos_rate).astype(np.int64)
    y[:2] = (0, 1)

    line = dict(what="validation of mini-batch GGAD with config key eval_cache off / on: seconds, a device synchronise around every part, "
                     "medians after warm-up; runs = wall seconds of whole main.py --synthetic processes",
                device=torch.cuda.get_device_name(0), nodes=a.nodes, entries=int(graph.nnz), cases=len(cases), positives=int(y.sum()),
                warmup=a.warmup, reps=a.reps)
    sweep_s = series(lambda: score_nodes(model, cases, 150, device=True), a.warmup, a.reps)
    want = score_nodes(model, cases, 150, device=True)
    build_s, sweep = timed(lambda: ResidentSweep(model, cases, y, 150))
    scores_s = series(sweep.scores, a.warmup, a.reps)
    got = sweep.scores()
    line["sweep"] = dict(score_nodes=summary(sweep_s), resident_build_once_s=float(build_s), resident_scores=summary(scores_s),
                         scores_bit_equal=bool(torch.equal(got, want)), cache_bytes=int(sweep.x1.numel() * 4))
    print("sweep", json.dumps(line["sweep"]), flush=True)

    yd = sweep.labels
    for _ in range(a.warmup):
        binary_report(got, yd, 0.4)
        rank_report(got, yd, 0.4)
    bin_s, rank_s = [], []
    for _ in range(a.reps):                                        # alternating
        t, b = timed(lambda: binary_report(got, yd, 0.4))
        bin_s.append(t)
        t, r = timed(lambda: rank_report(got, yd, 0.4))
        rank_s.append(t)
    from ggad_amd import _lib
    line["metrics"] = dict(binary_report=summary(bin_s), rank_report=summary(rank_s),
                           max_pos=int(_lib.load().ggad_rank_metrics_max_pos()),
                           integers_equal=all(b[k] == r[k] for k in ("tp", "fp", "fn", "tn", "f1_1", "f1_0", "f1_macro", "gmean")),
                           auc_abs_diff=abs(b["auc"] - r["auc"]), ap_abs_diff=abs(b["ap"] - r["ap"]))
    # a validation as the handler runs it: scores + report
    val_off = series(lambda: binary_report(score_nodes(model, cases, 150, device=True), yd, 0.4), 1, a.reps)
    val_on = series(lambda: sweep.report(0.4), 1, a.reps)
    line["validation"] = dict(key_off=summary(val_off), key_on=summary(val_on))
    print("metrics", json.dumps(line["metrics"]), flush=True)
    print("validation", json.dumps(line["validation"]), flush=True)
    del sweep, model, enc, graph, rp, ci, got, want
    torch.cuda.empty_cache()

    if not a.no_runs:
        off_s, on_s, same = [], [], True
        for _ in range(a.run_reps):                                # alternating, one process each
            t_off, tail_off = whole_run(a.epochs, False, a.entries)
            t_on, tail_on = whole_run(a.epochs, True, a.entries)
            off_s.append(t_off)
            on_s.append(t_on)
            same = same and tail_off[0] == tail_on[0] and tail_off[1] == tail_on[1]
        line["runs"] = dict(num_epochs=a.epochs, key_off_wall_s=off_s, key_on_wall_s=on_s, confusion_and_f1_lines_equal=bool(same))
        print("runs", json.dumps(line["runs"]), flush=True)
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
