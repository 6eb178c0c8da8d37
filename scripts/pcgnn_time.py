#!/usr/bin/env python3
"""Time per optimiser step of PC-GNN (`IntraAgg` x 3 -> `InterAgg` -> `PCALayer`, FlatAdam), three legs: the set path (python sets
per batch, `ggad_amd/layers.py`), the device path (CSR relations in HBM, `ggad_amd/pcgnn_device.py`, `csrc/pcgnn.hip`) and the
device path with the fused head (`pcgnn_fused`: `csrc/pcgnn_head.hip` behind the relation kernels).

    python scripts/pcgnn_time.py [--steps 30] [--nodes 200000] [--big_nodes 3700550] [--out profiles/pcgnn_time_line.json]

1. Comparison size: three synthetic power-law relations on `--nodes` nodes (a size whose dict-of-sets builds in well under a
   minute); the same relations, batches and initial weights on all three legs; median wall time of a step that ends in a device
   synchronise.  The time to build each path's graph container is reported beside it.
2. The two device legs on three relations of DGraph-Fin's node count (`--big_nodes`, `--big_entries` directed entries each).

Prints and writes one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ggad_amd import synth  # noqa: E402
from ggad_amd.fullgraph import FlatAdam  # noqa: E402
from ggad_amd.graph import DeviceGraph  # noqa: E402
from ggad_amd.graphsage import FeatureTable  # noqa: E402
from ggad_amd.layers import InterAgg, IntraAgg, PCALayer  # noqa: E402


def build_model(relations, feat, d, seed, fused=False):
    torch.manual_seed(seed)
    feats = FeatureTable(torch.from_numpy(feat))
    f = feat.shape[1]
    intras = [IntraAgg(feats, f, d, [], 0.5, cuda=True) for _ in range(3)]
    inter = InterAgg(feats, f, d, [], relations, intras, inter="GNN", cuda=True, fused=fused)
    model = PCALayer(2, inter, 2)
    return model, FlatAdam([p for p in model.parameters() if p.requires_grad], lr=0.005, weight_decay=0.007)


def time_steps(model, opt, batches, labels, warmup):
    times, losses = [], []
    for k, nodes in enumerate(batches):
        lab = torch.as_tensor(labels[nodes], device="cuda").long()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad()
        loss, _ = model.loss(nodes.tolist(), lab)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
        losses.append(float(loss.item()))
    return dict(median_ms=float(np.median(times)), min_ms=float(np.min(times)), max_ms=float(np.max(times)), steps=len(times),
                first_loss=losses[0], last_loss=losses[-1])


def make_batches(n, labels, steps, batch, seed):
    rng = np.random.default_rng(seed)
    pos = np.flatnonzero(labels == 1)
    out = []
    for _ in range(steps):
        b = rng.choice(n, size=batch, replace=False)
        b[:8] = rng.choice(pos, size=8, replace=False)           # both labels in every batch
        out.append(b.astype(np.int64))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--batch", type=int, default=200)
    p.add_argument("--feat", type=int, default=17)
    p.add_argument("--emb", type=int, default=64)
    p.add_argument("--nodes", type=int, default=200_000)
    p.add_argument("--entries", type=int, default=2_000_000, help="directed entries of the first relation; the others hold 1.25x and 1.5x")
    p.add_argument("--big_nodes", type=int, default=3_700_550)
    p.add_argument("--big_entries", type=int, default=24_368_502, help="directed entries per relation (a third of the bench graph's)")
    p.add_argument("--max_degree", type=int, default=2000)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pcgnn_time.py needs an MI355X")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    line = dict(what="PC-GNN, median wall ms per optimiser step (loss, backward, FlatAdam; ends in a device synchronise): set = python-set "
                     "neighbour lists per batch (layers.IntraAgg), device = CSR relations in HBM (pcgnn_device.py, csrc/pcgnn.hip), fused = "
                     "device + the head and loss in csrc/pcgnn_head.hip (pcgnn_fused); same relations, batches and initial weights; "
                     "fused_over_device = fused median / device median; big = the two device legs at DGraph-Fin's node count",
                device=torch.cuda.get_device_name(0), batch=a.batch, feat=a.feat, emb=a.emb)
    total = a.steps + a.warmup
    # ---- 1. comparison size
    rels = [synth.make_graph_torch(a.nodes, int(a.entries * s), 11 + k, dev, max_degree=a.max_degree) for k, s in enumerate((1.0, 1.25, 1.5))]
    feat = synth.make_features(a.nodes, a.feat, 3)
    labels = synth.make_labels(a.nodes, 0.05, 3)
    batches = make_batches(a.nodes, labels, total, a.batch, 5)
    t0 = time.perf_counter()
    sets = [synth.csr_to_adj_lists(rp, ci) for rp, ci in rels]
    t_sets = time.perf_counter() - t0
    t0 = time.perf_counter()
    graphs = [DeviceGraph(rp, ci, dev) for rp, ci in rels]
    model_d, opt_d = build_model(graphs, feat, a.emb, 1)          # (construction runs check_relation once per relation)
    torch.cuda.synchronize()
    t_graphs = time.perf_counter() - t0
    model_f, opt_f = build_model(graphs, feat, a.emb, 1, fused=True)
    model_s, opt_s = build_model(sets, feat, a.emb, 1)
    cmp_ = dict(nodes=a.nodes, entries=[int(len(ci)) for _, ci in rels], build_sets_s=t_sets, build_device_graphs_and_check_s=t_graphs)
    cmp_["device"] = time_steps(model_d, opt_d, batches, labels, a.warmup)
    cmp_["fused"] = time_steps(model_f, opt_f, batches, labels, a.warmup)
    cmp_["set"] = time_steps(model_s, opt_s, batches, labels, a.warmup)
    cmp_["speedup"] = cmp_["set"]["median_ms"] / cmp_["device"]["median_ms"]
    cmp_["fused_over_device"] = cmp_["fused"]["median_ms"] / cmp_["device"]["median_ms"]
    line["comparison"] = cmp_
    print("comparison", cmp_, flush=True)
    del sets, model_s, opt_s, model_d, opt_d, model_f, opt_f, graphs
    # ---- 2. DGraph size, the two device legs
    rels = [synth.make_graph_torch(a.big_nodes, a.big_entries, 21 + k, dev, max_degree=a.max_degree) for k in range(3)]
    feat = synth.make_features(a.big_nodes, a.feat, 4)
    labels = synth.make_labels(a.big_nodes, 15509.0 / 3700550.0, 4)
    batches = make_batches(a.big_nodes, labels, total, a.batch, 6)
    t0 = time.perf_counter()
    graphs = [DeviceGraph(rp, ci, dev) for rp, ci in rels]
    model_d, opt_d = build_model(graphs, feat, a.emb, 1)
    torch.cuda.synchronize()
    big = dict(nodes=a.big_nodes, entries=[int(len(ci)) for _, ci in rels], build_device_graphs_and_check_s=time.perf_counter() - t0)
    big["device"] = time_steps(model_d, opt_d, batches, labels, a.warmup)
    del model_d, opt_d
    model_f, opt_f = build_model(graphs, feat, a.emb, 1, fused=True)
    big["fused"] = time_steps(model_f, opt_f, batches, labels, a.warmup)
    big["fused_over_device"] = big["fused"]["median_ms"] / big["device"]["median_ms"]
    line["big"] = big
    print("big", big, flush=True)
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
