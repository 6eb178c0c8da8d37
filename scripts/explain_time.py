#!/usr/bin/env python3
"""What an explained list costs: `ggad_explain_f32` (csrc/explain.hip) against a torch restatement on the DGraph-size test sweep.

    python scripts/explain_time.py [--nodes 3700550] [--entries 73105508] [--cases 1736598] [--reps 7] [--m 5]
                                   [--out profiles/explain_time_line.json]

On the synthetic graph of bench.py (power-law degrees, 17 features, emb 64) a `ResidentSweep` over `--cases` ids gives the scores and
`top_k` the ranked positions.  One process, a device synchronise around every timed part, every part run `--warmup` times before it
is timed, the routes alternating, medians of `--reps` (all values are kept).  For the top 100 and the top 8,192:

  explain   `ResidentSweep.explain(ranked, m)`: the public call -- the sizing read-back, the allocations, the one launch, the read-back
            of the four meta words
  torch     the same rows restated with torch on the device: the closed rows of every row of the explained rows' slices as (slice, node)
            keys, `torch.unique(..., return_counts=True)` for c_j and `searchsorted` to read it back (index ops), `index_add_` for x1,
            autograd of sum_i z_i for g, two stable sorts for the m greatest per row.  Its sums have no fixed order.

The two are compared: c_j exactly, logits and listed contributions by their greatest difference, the listed ids by the share of rows
whose lists agree (equal float32 values may order differently: torch's sums are not the kernel's).
Prints and writes one JSON line."""
import argparse
import json
import os
import statistics
import sys
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


def closed_entries(graph, nodes):
    """(owner index into `nodes`, node j) of every entry of the closed rows of `nodes` (a node may stand twice), j ascending per owner."""
    rp = graph.rowptr.long()
    deg = rp[nodes + 1] - rp[nodes]
    own = torch.repeat_interleave(torch.arange(len(nodes), device=nodes.device), deg)
    start = torch.cumsum(deg, 0) - deg
    e = rp[nodes][own] + (torch.arange(int(deg.sum()), device=nodes.device) - start[own])
    j = graph.col.long()[e]
    has_self = torch.zeros(len(nodes), dtype=torch.bool, device=nodes.device)
    has_self[own[j == nodes[own]]] = True
    extra = torch.nonzero(~has_self).reshape(-1)
    own, j = torch.cat([own, extra]), torch.cat([j, nodes[extra]])
    order = torch.argsort(own * graph.n + j)
    return own[order], j[order]


def torch_explain(graph, feat, eng, ids, bs, pos, m):
    n, N = ids.numel(), graph.n
    pos = pos.long()
    w = eng.weight.reshape(-1)
    W = eng.enc_weight
    # c_j: every closed row of every row of the explained rows' slices, counted per (slice, node)
    slices = torch.unique(pos // bs)
    lo = slices * bs
    size = torch.clamp(lo + bs, max=n) - lo
    srow = torch.repeat_interleave(torch.arange(len(slices), device=pos.device), size)
    spos = lo[srow] + (torch.arange(int(size.sum()), device=pos.device) - (torch.cumsum(size, 0) - size)[srow])
    own, j = closed_entries(graph, ids[spos])
    keys, counts = torch.unique(srow[own] * N + j, return_counts=True)
    # the explained rows
    k_own, k_j = closed_entries(graph, ids[pos])
    K = pos.numel()
    r = torch.bincount(k_own, minlength=K)
    sl = torch.searchsorted(slices, pos // bs)
    c = counts[torch.searchsorted(keys, sl[k_own] * N + k_j)]
    om = (1.0 / torch.sqrt(r.float()))[k_own] / torch.sqrt(c.float())
    fj = feat[k_j]
    x1 = torch.zeros((K, feat.shape[1]), dtype=torch.float32, device=pos.device).index_add_(0, k_own, om[:, None] * fj)
    x1.requires_grad_(True)
    z = torch.relu(x1 @ W.t()) @ w
    g, = torch.autograd.grad(z.sum(), x1)
    x1 = x1.detach()
    t = om * (fj * g[k_own]).sum(1)
    # the m greatest per row, ties by ascending id: stable sort by -t, then stable by owner
    o1 = torch.sort(-t, stable=True)[1]
    o2 = torch.sort(k_own[o1], stable=True)[1]
    order = o1[o2]
    start = torch.cumsum(r, 0) - r
    slot = torch.arange(m, device=pos.device)[None, :]
    take = (start[:, None] + slot).clamp(max=order.numel() - 1)
    valid = slot < r[:, None]
    idx = order[take]
    nbr_id = torch.where(valid, k_j[idx], torch.full_like(take, -1))
    nbr_t = torch.where(valid, t[idx], torch.zeros_like(t[idx]))
    return dict(logit=z.detach(), feature=g * x1, closed_size=r, nbr_id=nbr_id, nbr_contrib=nbr_t, c=c, t=t, own=k_own)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=3_700_550)
    ap.add_argument("--entries", type=int, default=73_105_508)
    ap.add_argument("--cases", type=int, default=1_736_598)
    ap.add_argument("--m", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("explain_time.py needs an MI355X")
    dev = "cuda:0"
    torch.manual_seed(72)                                          # the encoder's initial weights: which rows rank first
    rp, ci = synth.make_graph_torch(a.nodes, a.entries, 72, dev, kind="powerlaw", max_degree=2000)
    graph = DeviceGraph(rp, ci, dev)
    feat = normalize_features(synth.make_features(a.nodes, 17, 72)).astype(np.float32)
    features = FeatureTable(torch.from_numpy(feat))
    enc = GCNEncoder(features, 17, 64, graph, GCNAggregator(features, cuda=True), gcn=True, cuda=True)
    model = GCN(2, enc)
    eng = enc.engine
    eng.sync_params()
    cases = np.random.default_rng(0).permutation(a.nodes)[:a.cases]
    sweep = ResidentSweep(model, cases, None, 150)
    scores = sweep.scores()
    lib = _lib.load()
    line = dict(what="explaining the top of the test sweep's ranking: seconds, a device synchronise around every part, medians after warm-up, "
                     "the routes alternating", device=torch.cuda.get_device_name(0), nodes=a.nodes, entries=int(graph.nnz),
                scores=sweep.n, batch_size=150, m=a.m, lds_rows=int(lib.ggad_explain_lds_rows()), warmup=a.warmup, reps=a.reps, by_k={})
    for k in (100, 8192):
        ranked = sweep.top_k(k, scores=scores)
        routes = dict(explain=lambda: sweep.explain(ranked, a.m),
                      torch=lambda: torch_explain(graph, features.weight.data, eng, sweep.ids, 150, ranked.pos, a.m))
        for fn in routes.values():
            for _ in range(a.warmup):
                timed(fn)
        ts = {name: [] for name in routes}
        for _ in range(a.reps):                                    # alternating
            for name, fn in routes.items():
                ts[name].append(timed(fn)[0])
        e, t = routes["explain"](), routes["torch"]()
        c_dev = torch.cat([e.neighbours(i)[1] for i in range(min(k, 256))]).long()
        n_first = int(e.closed_size[:min(k, 256)].sum())
        entry = {name: summary(v) for name, v in ts.items()}
        entry.update(max_closed=int(e.closed_size.max()), mean_closed=float(e.closed_size.float().mean()), rows_workspace=e.rows_workspace,
                     completeness=e.completeness(), closed_sizes_equal=bool(torch.equal(e.closed_size.long(), t["closed_size"])),
                     colcounts_equal_first_256_rows=bool(torch.equal(c_dev, t["c"][:n_first])),
                     max_logit_diff=float((e.logit - t["logit"]).abs().max()), max_feature_diff=float((e.feature - t["feature"]).abs().max()),
                     max_listed_contrib_diff=float((e.nbr_contrib - t["nbr_contrib"]).abs().max()),
                     rows_with_equal_lists=float((e.nbr_id == t["nbr_id"]).all(1).float().mean()))
        line["by_k"][str(k)] = entry
        print(k, json.dumps(entry), flush=True)
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
