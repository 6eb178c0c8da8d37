#!/usr/bin/env python3
"""Median replayed epoch of the full-graph GAAN (gaan.py) at the five published sizes (synthetic graphs, embedding_dim 300).

    python scripts/gaan_time.py [--epochs 30] [--sizes reddit,Amazon,...] [--out profiles/gaan_time_line.json]

Per size: the script's setup, two eager epochs, the capture, then `--epochs` replays, each bracketed by device events; the noise draw
and its copy happen before the start event, as in gaan.py.  The host draw (torch.randn(N, 16) on the CPU generator) is timed on its
own per epoch, because a user's wall clock includes it.  Prints and writes one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gaan  # noqa: E402
from ggad_amd.fullgraph_script import capture  # noqa: E402
from ggad_amd.model_gaan import edge_structs  # noqa: E402


def time_size(dataset, epochs):
    args = gaan.parse(["--dataset", dataset, "--synthetic", "--quiet", "--num_epoch", "1"])
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    full, feats, model, opt, opt_gen, ano, all_idx, idx_test = gaan.setup(args, dev)
    epoch_fn = gaan.make_epoch(model, opt, opt_gen, feats, full, all_idx, idx_test)
    for _ in range(2):
        epoch_fn()
    n = full.n
    noise_buf = torch.zeros(n, model.noise_dim, device=dev)
    model.noise_override = noise_buf
    model.emb = None
    opt.zero_grad()
    opt_gen.zero_grad()
    graph, _ = capture(epoch_fn)
    model.noise_override = None
    times, draws = [], []
    for _ in range(epochs):
        t0 = time.perf_counter()
        noise = torch.randn(n, model.noise_dim)
        draws.append((time.perf_counter() - t0) * 1e3)
        noise_buf.copy_(noise)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return dict(n=n, f=int(feats.shape[-1]), m=int(edge_structs(full, all_idx)["m"]), median_ms=float(np.median(times)),
                min_ms=float(np.min(times)), max_ms=float(np.max(times)), host_noise_draw_median_ms=float(np.median(draws)), epochs=epochs)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--epochs", type=int, default=30)
    p.add_argument("--sizes", type=str, default="reddit,Amazon,photo,t_finance,elliptic")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    torch.cuda.set_device(0)
    line = dict(what="gaan replayed epoch (device events, noise draw and copy outside them), embedding_dim 300, synthetic graphs of "
                     "the published sizes; host_noise_draw = torch.randn(N, 16) on the CPU generator, per epoch",
                device=torch.cuda.get_device_name(0), reference_dense_cpu_epoch_reddit="not measured", sizes={})
    for ds in a.sizes.split(","):
        t0 = time.time()
        line["sizes"][ds] = time_size(ds, a.epochs)
        print(ds, line["sizes"][ds], "({:.0f} s)".format(time.time() - t0), flush=True)
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
