#!/usr/bin/env python3
"""Time per optimiser step of the GraphSAGE baseline (`MeanAggregator` -> `Encoder` -> `GraphSage`, FlatAdam): the set path (a python
set, `random.sample` and `sorted` per batch row; `ggad_amd/graphsage.py`) against the device path (native sampler, fused step
kernels; `ggad_amd/sage_device.py`, `csrc/sage.hip`, `csrc/sampler.cpp`) and the epoch path (one native sampler call, one upload and
one replayed graph per epoch of `--epoch_steps` steps; `ggad_amd/sage_epoch.py`).

    python scripts/sage_time.py [--steps 60] [--nodes 3700550] [--out profiles/sage_time_line.json]

One synthetic power-law graph of DGraph-Fin's node count, held as a `DeviceGraph` by both paths; batches of 150 + 50 ids, F = 17,
D = 64; the same batches, the same initial weights and the same start of the `random` stream for both.  Reported: the median wall time
of a step that ends in a device synchronise, per path; the native sampler alone per batch; a validation sweep (`to_prob` over
`--sweep` ids: chunks of the batch size on the set path, one call on the device path; run twice, the first pays for new buffers).
The device leg is repeated three times (`device_repeats_ms`), and so is the epoch leg: whole epochs, wall clock from the start of
the host sampling to a synchronise after the replay, divided by the steps of an epoch -- the median of `--epochs` epochs after 2,
once with nothing overlapped (`serial`) and once with the next epoch sampled while the device runs (`overlapped`) --, beside
the scheduler's own time per batch.  Prints and writes one JSON line."""
import argparse
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
from ggad_amd.fullgraph import FlatAdam  # noqa: E402
from ggad_amd.graph import DeviceGraph  # noqa: E402
from ggad_amd.graphsage import Encoder, FeatureTable, GraphSage, MeanAggregator  # noqa: E402
from ggad_amd.sage_device import SageDevice  # noqa: E402
from ggad_amd.sage_epoch import SageEpoch  # noqa: E402
from ggad_amd.sampler import PyCompatRandom  # noqa: E402


def build_model(graph, feats, f, d, seed, rng):
    torch.manual_seed(seed)
    agg = MeanAggregator(feats, cuda=True)
    dev = None if rng is None else SageDevice(graph, feats, f, d, 10, rng=rng)
    enc = Encoder(feats, f, d, graph, agg, gcn=False, cuda=True, sage_device=dev)
    model = GraphSage(2, enc).to(feats.weight.device)
    return model, FlatAdam([p for p in model.parameters() if p.requires_grad], lr=0.005, weight_decay=0.007)


def time_steps(model, opt, batches, labels, warmup):
    times, losses = [], []
    for k, nodes in enumerate(batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad()
        if model.enc.device_path is not None:
            loss = model.loss(nodes, labels[nodes])
        else:
            loss = model.loss(nodes.tolist(), torch.as_tensor(labels[nodes], device="cuda").long())
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
        losses.append(float(loss.item()))
    return dict(median_ms=float(np.median(times)), min_ms=float(np.min(times)), max_ms=float(np.max(times)), steps=len(times),
                first_loss=losses[0], last_loss=losses[-1])


def time_epochs(runner, epochs, ahead):
    """Median wall ms per step over `epochs` epochs after 2: one `run_epoch` call -- host sampling (of this epoch, or with
    ahead="epoch" of the next one while the device runs), upload, replay, the read of the losses -- ends synchronised."""
    per = []
    for e in range(epochs + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = runner.run_epoch(ahead)
        torch.cuda.synchronize()
        if e >= 2:
            per.append((time.perf_counter() - t0) * 1e3 / runner.nb)
    return float(np.median(per)), float(losses[-1])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=60)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--batch", type=int, default=150)
    p.add_argument("--pseudo", type=int, default=50)
    p.add_argument("--feat", type=int, default=17)
    p.add_argument("--emb", type=int, default=64)
    p.add_argument("--nodes", type=int, default=3_700_550)
    p.add_argument("--entries", type=int, default=24_368_502)
    p.add_argument("--max_degree", type=int, default=2000)
    p.add_argument("--sweep", type=int, default=20_000)
    p.add_argument("--epoch_steps", type=int, default=150)
    p.add_argument("--epochs", type=int, default=5)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sage_time.py needs an MI355X")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    rowptr, col = synth.make_graph_torch(a.nodes, a.entries, 11, dev, max_degree=a.max_degree)
    graph = DeviceGraph(rowptr, col, dev)
    feats = FeatureTable(torch.from_numpy(synth.make_features(a.nodes, a.feat, 3)))
    labels = synth.make_labels(a.nodes, 15509.0 / 3700550.0, 3)
    pool = np.flatnonzero(labels == 1)
    gen = np.random.default_rng(5)
    total = a.steps + a.warmup
    batches = [np.concatenate([gen.choice(a.nodes, size=a.batch, replace=False), gen.choice(pool, size=a.pseudo, replace=False)])
               .astype(np.int64) for _ in range(total)]
    sweep = gen.choice(a.nodes, size=a.sweep, replace=False).astype(np.int64)
    line = dict(what="GraphSAGE baseline, median wall ms per optimiser step (loss, backward, FlatAdam; ends in a device synchronise): "
                     "set = python set + random.sample per batch row (graphsage.py), device = native sampler + fused step kernels "
                     "(sage_device.py, csrc/sage.hip); same DeviceGraph, batches, initial weights and random stream; sampler = "
                     "ggad_mt_sample_rows alone per batch; sweep = to_prob over `sweep_nodes` ids (set: chunks of the batch size); "
                     "device_repeats_ms = the device leg three more times; epoch = sage_epoch.py, whole epochs of `steps_per_epoch` "
                     "steps from the start of host sampling to a synchronise after the replay, per step, median of `epochs` epochs "
                     "after 2, three repeats: serial = nothing overlapped, overlapped = the next epoch sampled while the device "
                     "runs; epoch.sampler_ms_per_batch = ggad_sage_sched_epoch alone (shuffles included)",
                device=torch.cuda.get_device_name(0), nodes=a.nodes, entries=int(len(col)), batch=a.batch + a.pseudo, feat=a.feat,
                emb=a.emb, sweep_nodes=a.sweep)
    # ---- the device path
    random.seed(72)
    rng = PyCompatRandom.from_python_state(random.getstate())
    model_d, opt_d = build_model(graph, feats, a.feat, a.emb, 1, rng)
    line["device"] = time_steps(model_d, opt_d, batches, labels, a.warmup)
    for key in ("sweep_first_ms", "sweep_ms"):                    # the first sweep pays the allocation of its buffers
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            pd = model_d.to_prob(sweep)
        torch.cuda.synchronize()
        line["device"][key] = (time.perf_counter() - t0) * 1e3
    state_d = rng.to_python_state()
    print("device", line["device"], flush=True)
    # ---- the device leg again, three times, and the epoch path: same graph, batch shape, initial weights and start of the stream
    line["device_repeats_ms"] = []
    for _ in range(3):
        model_r, opt_r = build_model(graph, feats, a.feat, a.emb, 1, PyCompatRandom(72))
        line["device_repeats_ms"].append(time_steps(model_r, opt_r, batches, labels, a.warmup)["median_ms"])
    train0 = gen.choice(a.nodes, size=a.epoch_steps * a.batch, replace=False).astype(np.int64)
    line["epoch"] = dict(steps_per_epoch=a.epoch_steps, epochs=a.epochs, n_train=int(len(train0)), n_pool=int(len(pool)),
                         serial_ms_per_step=[], overlapped_ms_per_step=[])
    for mode, ahead in (("serial", None), ("overlapped", "epoch")):
        for _ in range(3):
            rng_e = PyCompatRandom(72)
            model_e, opt_e = build_model(graph, feats, a.feat, a.emb, 1, rng_e)
            runner = SageEpoch(model_e.enc.device_path, model_e.enc.weight, model_e.weight, opt_e, train0.copy(),
                               pool.astype(np.int64), labels, a.batch, a.pseudo, a.epoch_steps)
            ms, last = time_epochs(runner, max(a.epochs, 5), ahead)
            line["epoch"][mode + "_ms_per_step"].append(ms)
            line["epoch"]["last_loss"] = last
            assert runner.replays == runner.epochs_run - 1
    ts = []
    for _ in range(max(a.epochs, 5)):                             # the scheduler alone: shuffles and sample tables of one epoch
        t0 = time.perf_counter()
        runner.sample(0)
        ts.append((time.perf_counter() - t0) * 1e3 / a.epoch_steps)
    line["epoch"]["sampler_ms_per_batch"] = float(np.median(ts))
    line["epoch"]["below_device_leg"] = bool(max(line["epoch"]["serial_ms_per_step"]) < min(line["device_repeats_ms"]))
    print("epoch", line["epoch"], "device repeats", line["device_repeats_ms"], flush=True)
    # ---- the native sampler alone
    alone = PyCompatRandom(72)
    t0 = time.perf_counter()
    alone.sample_rows(graph.rowptr_host, graph.col_host, sweep, 10)
    line["sampler_ms_per_sweep"] = (time.perf_counter() - t0) * 1e3
    ts = []
    for nodes in batches:
        t0 = time.perf_counter()
        alone.sample_rows(graph.rowptr_host, graph.col_host, nodes, 10)
        ts.append((time.perf_counter() - t0) * 1e3)
    line["sampler_ms_per_batch"] = dict(median=float(np.median(ts[a.warmup:])), max=float(np.max(ts[a.warmup:])))
    # ---- the set path
    random.seed(72)
    model_s, opt_s = build_model(graph, feats, a.feat, a.emb, 1, None)
    line["set"] = time_steps(model_s, opt_s, batches, labels, a.warmup)
    step = a.batch + a.pseudo
    for key in ("sweep_first_ms", "sweep_ms"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            ps = torch.cat([model_s.to_prob(sweep[s:s + step].tolist()) for s in range(0, len(sweep), step)])
        torch.cuda.synchronize()
        line["set"][key] = (time.perf_counter() - t0) * 1e3
    print("set", line["set"], flush=True)
    line["same_random_stream"] = bool(random.getstate() == state_d)
    line["max_abs_prob_difference"] = float((pd - ps).abs().max())
    line["speedup_step"] = line["set"]["median_ms"] / line["device"]["median_ms"]
    line["speedup_sweep"] = line["set"]["sweep_ms"] / line["device"]["sweep_ms"]
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
