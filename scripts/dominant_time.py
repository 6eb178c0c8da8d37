#!/usr/bin/env python3
"""Median replayed epoch of the full-graph DOMINANT (dominant.py) at the five published sizes (synthetic graphs, embedding_dim 300).

    python scripts/dominant_time.py [--epochs 30] [--sizes reddit,Amazon,...] [--out profiles/dominant_time_line.json]

Per size: the script's setup, the first eager epoch timed on its own (it runs the GCN branch and builds the row structures), a second
eager epoch, the capture, then `--epochs` replays, each bracketed by device events.  Where the fused autoencoder holds the size, the
same is repeated with the wide path forced (`Model.force_wide`) as the comparison.  Prints and writes one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dominant  # noqa: E402
from ggad_amd.fullgraph_script import capture  # noqa: E402
from ggad_amd.model_dominant import fused_supported  # noqa: E402


def time_path(dataset, epochs, wide):
    args = dominant.parse(["--dataset", dataset, "--synthetic", "--quiet", "--num_epoch", "1"])
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    full, feats, model, opt, ano, normal_idx, idx_test = dominant.setup(args, dev)
    model.force_wide = wide
    epoch_fn = dominant.make_epoch(model, opt, feats, full, normal_idx, idx_test)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    epoch_fn()
    torch.cuda.synchronize()
    first = (time.perf_counter() - t0) * 1e3
    epoch_fn()
    graph, _ = capture(epoch_fn, before=opt.zero_grad)
    times = []
    for _ in range(epochs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return dict(n=full.n, f=int(feats.shape[-1]), train_rows=len(normal_idx), test_rows=len(idx_test), median_ms=float(np.median(times)),
                min_ms=float(np.min(times)), max_ms=float(np.max(times)), first_epoch_wall_ms=first, epochs=epochs)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--epochs", type=int, default=30)
    p.add_argument("--sizes", type=str, default="reddit,Amazon,photo,t_finance,elliptic")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    torch.cuda.set_device(0)
    line = dict(what="dominant replayed epoch (device events), embedding_dim 300, synthetic graphs of the published sizes; "
                     "first_epoch_wall_ms = the first eager epoch (GCN branch, row structures, module load); wide = the same epoch "
                     "with the wide path forced", device=torch.cuda.get_device_name(0), reference_epoch="not measured", sizes={})
    for ds in a.sizes.split(","):
        t0 = time.time()
        r = time_path(ds, a.epochs, wide=False)
        r["path"] = "fused" if fused_supported(r["f"], 300) else "wide"
        if r["path"] == "fused":
            r["wide"] = time_path(ds, a.epochs, wide=True)
        line["sizes"][ds] = r
        print(ds, r, "({:.0f} s)".format(time.time() - t0), flush=True)
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
