#!/usr/bin/env python3
"""What the ranked list costs: `ggad_topk_f32` (csrc/topk.hip) against torch on the scores of the DGraph-size test sweep.

    python scripts/topk_time.py [--nodes 3700550] [--entries 73105508] [--cases 1736598] [--reps 7] [--epochs 11] [--no-runs]
                                [--profile-k K] [--out profiles/topk_time_line.json]

On the synthetic graph of bench.py (power-law degrees, 17 features, emb 64) a `ResidentSweep` over `--cases` ids gives the float32
scores; one process, a device synchronise around every timed part, every part run `--warmup` times before it is timed, the routes
alternating, medians of `--reps` (all values are kept).  For k in 100, 1,000 and 8,192:

  native        the six launches of `ggad_topk_f32` into buffers allocated beforehand (positions, scores, running positives, meta)
  top_k         `ResidentSweep.top_k(k, scores)`: the public call -- allocations, the launches and the read-back of the four meta words
  torch_topk    `torch.topk(scores, k, sorted=True)`, the labels gathered at its indices and `cumsum`: the baseline; which tied elements
                it returns and in what order is not fixed
  torch_sort    `torch.sort(scores.double(), descending=True, stable=True)` as `metrics.binary_report` sorts, cut at k, the labels
                gathered and `cumsum`: the baseline with the SAME definition (ties by position); its positions are compared to native's

  runs          wall seconds of `python main.py --synthetic --num_epochs N` without and with `--top_k 1000 --top_k_out F`, one process
                each; then `main.py --synthetic --score <the second run's .pkl> --top_k 1000 --top_k_out G`: the report lines and the two
                files are compared

`--profile-k K`: only warm up and repeat the native call at that k (for a `rocprofv3 --kernel-trace --stats` run of its own).
Prints and writes one JSON line."""
import argparse
import glob
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
from ggad_amd import _lib, synth  # noqa: E402
from ggad_amd.dgraph import normalize_features  # noqa: E402
from ggad_amd.eval_cache import ResidentSweep  # noqa: E402
from ggad_amd.graph import DeviceGraph  # noqa: E402
from ggad_amd.graphsage import GCN, FeatureTable, GCNAggregator, GCNEncoder  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(xs):
    return dict(median_s=float(statistics.median(xs)), min_s=float(min(xs)), max_s=float(max(xs)), all_s=[float(x) for x in xs])


def main_py(tmp, entries, extra):
    """One `main.py --synthetic` process; returns (wall seconds, stdout)."""
    import yaml
    with open(os.path.join(ROOT, "src", "dgraph.yml")) as fh:
        cfg = yaml.safe_load(fh)
    cfg["save_dir"] = os.path.join(tmp, "models") + "/"
    path = os.path.join(tmp, "cfg.yml")
    with open(path, "w") as fh:
        yaml.safe_dump(cfg, fh)
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, "main.py", "--config", path, "--synthetic", "--synthetic_entries", str(entries)] + extra,
                       cwd=os.path.join(ROOT, "src"), capture_output=True, text=True)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        sys.exit(f"main.py {extra} failed with code {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return dt, p.stdout


def report_tail(out):
    return [ln for ln in out.splitlines() if ln.startswith(("   GNN ", "Testing AP", "Top-", "F1-Macro", "AUC", "G-Mean"))][-7:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=3_700_550)
    ap.add_argument("--entries", type=int, default=73_105_508)
    ap.add_argument("--cases", type=int, default=1_736_598)
    ap.add_argument("--pos-rate", type=float, default=0.0042)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=11)
    ap.add_argument("--no-runs", action="store_true")
    ap.add_argument("--profile-k", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_time.py needs an MI355X")
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
    sweep = ResidentSweep(model, cases, y, 150)
    scores, labels = sweep.scores(), sweep.labels
    n = sweep.n
    lib = _lib.load()
    distinct = int(torch.unique(scores).numel())

    def native_buffers(k):
        return (torch.empty(k, dtype=torch.int32, device=dev), torch.empty(k, dtype=torch.float32, device=dev),
                torch.empty(k, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int64, device=dev),
                torch.empty(int(lib.ggad_topk_workspace_elems(n, k)), dtype=torch.int32, device=dev))

    def native(k, b):
        _lib.call("ggad_topk_f32", _lib.ptr(scores), _lib.ptr(labels), n, k, _lib.ptr(b[0]), _lib.ptr(b[1]), _lib.ptr(b[2]), _lib.ptr(b[3]),
                  _lib.ptr(b[4]))
        return b

    def torch_topk(k):
        v, i = torch.topk(scores, k, sorted=True)
        return i, v, torch.cumsum(labels[i].to(torch.int32), 0)

    def torch_sort(k):
        v, i = torch.sort(scores.double(), descending=True, stable=True)
        i = i[:k]
        return i, v[:k], torch.cumsum(labels[i].to(torch.int32), 0)

    if a.profile_k:
        b = native_buffers(a.profile_k)
        for _ in range(a.warmup + a.reps):
            timed(lambda: native(a.profile_k, b))
        print(json.dumps(dict(profiled_k=a.profile_k, calls=a.warmup + a.reps, scores=n)))
        return

    line = dict(what="top-k of the test sweep's scores: seconds, a device synchronise around every part, medians after warm-up, the routes "
                     "alternating; runs = wall seconds of whole main.py --synthetic processes",
                device=torch.cuda.get_device_name(0), nodes=a.nodes, entries=int(graph.nnz), scores=n, positives=int(y.sum()),
                distinct_scores=distinct, max_k=int(lib.ggad_topk_max_k()), warmup=a.warmup, reps=a.reps, by_k={})
    for k in (100, 1000, 8192):
        b = native_buffers(k)
        routes = dict(native=lambda: native(k, b), top_k=lambda: sweep.top_k(k, scores=scores), torch_topk=lambda: torch_topk(k),
                      torch_sort=lambda: torch_sort(k))
        for fn in routes.values():
            for _ in range(a.warmup):
                timed(fn)
        ts = {name: [] for name in routes}
        for _ in range(a.reps):                                    # alternating
            for name, fn in routes.items():
                ts[name].append(timed(fn)[0])
        pos = native(k, b)[0].long()
        it, _, ct = torch_topk(k)
        isrt, _, cs = torch_sort(k)
        entry = {name: summary(v) for name, v in ts.items()}
        entry.update(tied_left_out=int(b[3][3]), positions_equal_torch_sort=bool(torch.equal(pos, isrt)),
                     cum_pos_equal_torch_sort=bool(torch.equal(b[2], cs.to(torch.int32))),
                     positions_equal_torch_topk=bool(torch.equal(pos, it)),
                     same_set_as_torch_topk=bool(torch.equal(torch.sort(pos)[0], torch.sort(it)[0])))
        line["by_k"][str(k)] = entry
        print(k, json.dumps(entry), flush=True)
    del sweep, model, enc, graph, rp, ci, scores, labels
    torch.cuda.empty_cache()

    if not a.no_runs:
        with tempfile.TemporaryDirectory() as t0, tempfile.TemporaryDirectory() as t1:
            epochs = ["--num_epochs", str(a.epochs)]
            off_s, off_out = main_py(t0, a.entries, epochs)
            f1, f2 = os.path.join(t1, "r.npz"), os.path.join(t1, "again.npz")
            on_s, on_out = main_py(t1, a.entries, epochs + ["--top_k", "1000", "--top_k_out", f1])
            ckpt = glob.glob(os.path.join(t1, "models", "*", "*.pkl"))
            sc_s, sc_out = main_py(t1, a.entries, ["--score", ckpt[0], "--top_k", "1000", "--top_k_out", f2])
            strip = lambda o: [ln for ln in report_tail(o) if not ln.startswith("Top-")][-6:]      # noqa: E731
            line["runs"] = dict(num_epochs=a.epochs, without_top_k_wall_s=off_s, with_top_k_1000_wall_s=on_s, score_wall_s=sc_s,
                                report_lines_equal_without_and_with=strip(off_out) == strip(on_out),
                                score_report_lines_equal=report_tail(sc_out) == report_tail(on_out),
                                score_file_identical=open(f1, "rb").read() == open(f2, "rb").read(),
                                top_line=[ln for ln in on_out.splitlines() if ln.startswith("Top-")])
        print("runs", json.dumps(line["runs"]), flush=True)
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
