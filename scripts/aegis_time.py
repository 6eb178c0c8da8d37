#!/usr/bin/env python3
"""Median replayed main epoch of the full-graph AEGIS (aegis.py) at the five published sizes (synthetic graphs, embedding_dim 300).

    python scripts/aegis_time.py [--epochs 30] [--sizes reddit,Amazon,...] [--out profiles/aegis_time_line.json]

Per size: the script's setup, one eager pre-training epoch, two eager main epochs, the capture, then `--epochs` replays, each bracketed
by device events (the noise draw and its copy happen before the start event, as in aegis.py).  Prints and writes one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aegis  # noqa: E402
from ggad_amd.fullgraph_script import capture  # noqa: E402


def time_size(dataset, epochs):
    args = aegis.parse(["--dataset", dataset, "--synthetic", "--quiet", "--lr", "1e-3", "--num_epoch", "1"])
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    full, feats, model, opt_ae, opt, opt_gen, ano, all_idx, idx_test, normal_idx = aegis.setup(args, dev)
    loss = model.train_forward(feats, full, normal_idx, idx_test)[0]
    loss.backward()
    opt_ae.step()
    loss = None
    main_epoch = aegis.make_main_epoch(model, opt, opt_gen, feats, full, all_idx, idx_test)
    for _ in range(2):
        main_epoch()
    n = full.n
    noise_buf = torch.zeros(n, model.noise_dim, device=dev)
    model.noise_override = noise_buf
    opt_ae.zero_grad()
    opt.zero_grad()
    opt_gen.zero_grad()
    graph, _ = capture(main_epoch)
    model.noise_override = None
    times = []
    for _ in range(epochs):
        noise_buf.copy_(torch.randn(n, model.noise_dim))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return dict(n=n, f=int(feats.shape[-1]), median_ms=float(np.median(times)), min_ms=float(np.min(times)), max_ms=float(np.max(times)),
                epochs=epochs)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--epochs", type=int, default=30)
    p.add_argument("--sizes", type=str, default="reddit,Amazon,photo,t_finance,elliptic")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    torch.cuda.set_device(0)
    line = dict(what="aegis replayed main epoch (device events), embedding_dim 300, synthetic graphs of the published sizes",
                device=torch.cuda.get_device_name(0), sizes={})
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
