#!/usr/bin/env python3
"""Time per epoch of the mini-batch AEGIS handler (`ggad_amd/model_handler_aegis.py`): the default path (per batch `LinearFn`
products, torch batch norm / sigmoid / BCE, autograd, FlatAdam, every launch from the host) against the device path
(`aegis_device: true`: `csrc/aegis_mb.hip`, `ggad_amd/aegis_device.py`), eager and with the epoch's steps replayed as one hipGraph.

    python scripts/aegis_mb_time.py [--epochs 9] [--nodes 3700550] [--out profiles/aegis_mb_time_line.json]

One synthetic power-law graph of DGraph-Fin's node count, held as a `DeviceGraph`; batches of 150, 100 batches per epoch, F = 17;
the same seeds, hence the same split, schedule and initial weights for every run.  Reported per path: the median wall time of an
epoch (one plan of the 100 batch sub-graphs per table, the 100 optimiser steps, a device synchronise; epochs 0 and 1 -- eager
start, capture -- are left out), the plan alone, and one `aegis_scores` sweep over `--sweep` ids (run twice: the first pays for new
buffers).  Prints and writes one JSON line."""
import argparse
import contextlib
import io
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ggad_amd import synth  # noqa: E402
from ggad_amd.graph import DeviceGraph  # noqa: E402
from ggad_amd.model_handler_aegis import ModelHandler  # noqa: E402
from ggad_amd.sage_utils import aegis_scores  # noqa: E402


def run(data, a, sweep, **kw):
    cfg = dict(data_name="synthetic", data_dir="", data=data, seed=72, model="GCN", multi_relation="GNN", emb_size=64, thres=0.4,
               lr=0.005, weight_decay=0.007, batch_size=a.batch, num_epochs=a.epochs, valid_epochs=10 ** 9, num_batches=a.batches,
               save_dir="./pytorch_models/", test_ratio=0.67, device=0)
    cfg.update(kw)
    random.seed(72)
    np.random.seed(72)
    torch.manual_seed(72)
    with contextlib.redirect_stdout(io.StringIO()):
        h = ModelHandler(cfg)
        h.dataset["idx_valid"], h.dataset["y_valid"] = h.dataset["idx_valid"][:2 * a.batch], h.dataset["y_valid"][:2 * a.batch]
        h.train()
    ms = np.array(h.epoch_times[2:]) * 1e3
    out = dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()), epochs=len(ms),
               first_epoch_ms=h.epoch_times[0] * 1e3, second_epoch_ms=h.epoch_times[1] * 1e3,
               last_loss_dis=float(h.epoch_losses[-1][:, 0].mean()), last_loss_g=float(h.epoch_losses[-1][:, 1].mean()))
    enc = h.model.enc
    gen = np.random.default_rng(5)
    n = enc.features.weight.shape[0]
    ts = []
    for _ in range(5):
        batches = [gen.choice(n, size=a.batch, replace=False) for _ in range(a.batches)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc.aggregator.aggregate(batches, enc.adj_lists, a.batches)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    out["plan_ms"] = float(np.median(ts[1:]))
    for key in ("sweep_first_ms", "sweep_ms"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores = aegis_scores(h.model, sweep, a.batch)
        torch.cuda.synchronize()
        out[key] = (time.perf_counter() - t0) * 1e3
    return out, scores, h


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--epochs", type=int, default=9)
    p.add_argument("--batch", type=int, default=150)
    p.add_argument("--batches", type=int, default=100)
    p.add_argument("--feat", type=int, default=17)
    p.add_argument("--nodes", type=int, default=3_700_550)
    p.add_argument("--entries", type=int, default=24_368_502)
    p.add_argument("--max_degree", type=int, default=2000)
    p.add_argument("--sweep", type=int, default=20_000)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("aegis_mb_time.py needs an MI355X")
    if a.epochs < 4:
        sys.exit("--epochs: at least 4 (epochs 0 and 1 are not timed)")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rowptr, col = synth.make_graph_torch(a.nodes, a.entries, 11, dev, max_degree=a.max_degree)
    graph = DeviceGraph(rowptr, col, dev)
    feat = synth.make_features(a.nodes, a.feat, 3)
    labels = synth.make_labels(a.nodes, 15509.0 / 3700550.0, 3)
    data = (graph, feat, labels)
    sweep = np.random.default_rng(6).choice(a.nodes, size=a.sweep, replace=False).astype(np.int64)
    line = dict(what="mini-batch AEGIS handler, median wall ms per epoch (one plan per table for the epoch's batches, `batches` optimiser "
                     "steps, ends in a device synchronise; epochs 0 and 1 left out): default = LinearFn + torch batch norm / BCE + "
                     "autograd + FlatAdam launched from the host, device_eager / device_captured = csrc/aegis_mb.hip (forward, "
                     "backward, FlatAdam per step, one fold per epoch) launched from the host / replayed as one hipGraph; plan_ms = "
                     "the plan alone; sweep = aegis_scores over `sweep_nodes` ids in slices of `batch`",
                device=torch.cuda.get_device_name(0), nodes=a.nodes, entries=int(len(col)), batch=a.batch, batches=a.batches,
                feat=a.feat, sweep_nodes=a.sweep)
    line["device_captured"], s_cap, h_cap = run(data, a, sweep, aegis_device=True)
    print("device_captured", line["device_captured"], flush=True)
    line["device_eager"], s_eag, h_eag = run(data, a, sweep, aegis_device=True, capture=False)
    print("device_eager", line["device_eager"], flush=True)
    line["default"], s_def, _ = run(data, a, sweep)
    print("default", line["default"], flush=True)
    line["captured_equals_eager_bits"] = bool(torch.equal(s_cap, s_eag) and all(np.array_equal(x, y) for x, y in
                                                                                 zip(h_cap.epoch_losses, h_eag.epoch_losses)))
    line["max_abs_score_difference"] = float((s_cap - s_def).abs().max())
    for k in ("device_eager", "device_captured"):
        line["speedup_epoch_" + k] = line["default"]["median_ms"] / line[k]["median_ms"]
        line["speedup_steps_" + k] = ((line["default"]["median_ms"] - line["default"]["plan_ms"]) /
                                      max(line[k]["median_ms"] - line[k]["plan_ms"], 1e-9))
    line["speedup_sweep"] = line["default"]["sweep_ms"] / line["device_captured"]["sweep_ms"]
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
