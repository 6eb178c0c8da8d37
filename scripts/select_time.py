#!/usr/bin/env python3
"""What `run.py --select auroc` costs per epoch.

    python scripts/select_time.py [--epochs 200] [--repeats 3] [--datasets reddit,t_finance] [--out profiles/select_time_line.json]

For every dataset: the synthetic graph of the published size is built ONCE (`run.py --synthetic`), then `run.fit` trains on it with
and without `--select auroc`, the two alternating in one process, each from the same seed.  Reported: the script's own "median epoch"
wall time (host clock around an epoch that ends in a device synchronise; with 200 epochs the median is a replayed, captured epoch).
Without the flag `fit` runs exactly the code of the commit before the flag existed.  With it every epoch ends with one more forward
(`Model.score`: two GCN layers and the scorer MLP over all N nodes), a gather of the validation rows, the four launches of
`ggad_rank_metrics_f32`, `ggad_select_decide_f64` and two `ggad_select_copy_f32` (17 parameters) -- all inside the captured epoch.

Prints and writes one JSON line."""
import argparse
import contextlib
import io
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import run  # noqa: E402
from ggad_amd.model import Model  # noqa: E402


def median_ms(args, dev, full, feats, ft_size, g, select):
    args.select = select
    torch.manual_seed(args.seed)
    model = Model(ft_size, args.embedding_dim, "prelu", args.negsamp_ratio, args.readout).to(dev)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        run.fit(args, dev, full, feats, model, g.normal_idx, g.abn_idx, g.idx_test, g.ano_label, idx_val=g.idx_val)
    text = out.getvalue()
    m = re.search(r"median epoch ([0-9.]+) ms", text)
    if m is None:
        raise RuntimeError("no median epoch in the output of fit")
    best = re.search(r"\[select\] best epoch (\d+)", text)
    return float(m.group(1)), (int(best.group(1)) if best else None)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--epochs", type=int, default=200)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--datasets", type=str, default="reddit,t_finance")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("select_time.py needs an MI355X")
    line = dict(what="run.py --synthetic: the script's own 'median epoch' wall time (captured epoch, device synchronise included) without "
                     "and with --select auroc, alternating in one process on one graph; without = the code path of the commit before "
                     "the flag, unchanged",
                device=None, epochs_per_run=a.epochs, datasets={})
    for dataset in [d for d in a.datasets.split(",") if d]:
        args = run.parse(["--dataset", dataset, "--synthetic", "--quiet", "--num_epoch", str(a.epochs)])
        dev = run.init_process(args, "select_time.py")
        line["device"] = torch.cuda.get_device_name(dev)
        with contextlib.redirect_stdout(io.StringIO()):
            g = run.load_graph(args)
        full, feats, ft_size = run.prepare(args, g.adj, g.feat, dev)
        y_val = np.asarray(g.ano_label).reshape(-1)[np.asarray(g.idx_val)]
        print(dataset, "graph ready:", feats.shape[1], "nodes,", len(g.idx_val), "validation nodes,", int((y_val == 1).sum()), "positive",
              flush=True)
        off, on, best = [], [], []
        for _ in range(a.repeats):                      # alternating, one process
            off.append(median_ms(args, dev, full, feats, ft_size, g, None)[0])
            ms, be = median_ms(args, dev, full, feats, ft_size, g, "auroc")
            on.append(ms)
            best.append(be)
            print(dataset, "without", off[-1], "ms, with --select auroc", on[-1], "ms", flush=True)
        line["datasets"][dataset] = dict(nodes=int(feats.shape[1]), embedding_dim=int(args.embedding_dim), validation_nodes=len(g.idx_val),
                                         validation_positives=int((y_val == 1).sum()), without_median_ms=off, select_auroc_median_ms=on,
                                         added_ms=float(np.median(on) - np.median(off)), best_epoch=best)
        del full, feats, g
        torch.cuda.empty_cache()
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
