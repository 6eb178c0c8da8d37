#!/usr/bin/env python3
"""What TAM's truncation round costs on the host and on the device (`tam.py --device_cut`, csrc/tam_nsgt.hip).

    python scripts/tam_cut_time.py [--sizes reddit,Amazon,t_finance] [--rounds 3] [--runs reddit,Amazon,t_finance] [--num_epoch 500]
                                   [--repeats 2] [--out profiles/tam_cut_time_line.json]

1. The per-round setup -- what `tam.py` does between the end of one `train_cut` and the start of the next -- on synthetic graphs of
   the published sizes, `--rounds` rounds each from the same seed, both paths in one process on one GPU, a device synchronise around
   every part:
     host    `graph_nsgt`, `normalize_adj_tensor`, `FullGraphAdj(...)`          (the code path without the flag, unchanged)
     device  `DeviceNsgt.step`, `FullGraphAdj.with_adjacency`                   + once per run: `DeviceNsgt(...)`, the base `FullGraphAdj`
   The SpMM plans, which both paths build from the host arrays inside the first epoch of `train_cut`, are in neither.  The two paths'
   graphs are compared after every round (entry count and value bits).
2. The seconds `tam.py --synthetic --cutting 3 --num_epoch 500` itself prints at its end (distance calculation, every round's setup and
   training, the metric prints), with and without `--device_cut`, alternating `--repeats` times in this process after a 5-epoch
   run of each.

Prints and writes one JSON line."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tam  # noqa: E402
from ggad_amd import tam_utils as T  # noqa: E402
from ggad_amd.fullgraph import FullGraphAdj  # noqa: E402
from ggad_amd.fullgraph_script import synthetic_graph  # noqa: E402


class Clock:
    def __init__(self):
        self.parts = {}

    @contextlib.contextmanager
    def part(self, name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        yield
        torch.cuda.synchronize()
        self.parts.setdefault(name, []).append(time.perf_counter() - t0)


def setup_times(dataset, rounds, dev):
    adj, _, _ = synthetic_graph(dataset, 0)
    n = adj.shape[0]
    raw = (adj + sp.eye(n)).tocsr()
    raw.sort_indices()
    # random distances, symmetric with a zero diagonal like `calc_distance`'s: one draw per unordered pair
    rows = np.repeat(np.arange(n), np.diff(raw.indptr))
    lo, hi = np.minimum(rows, raw.indices).astype(np.int64), np.maximum(rows, raw.indices).astype(np.int64)
    uniq, inv = np.unique(lo * n + hi, return_inverse=True)
    dis = np.random.default_rng(1).random(len(uniq), dtype=np.float32)[inv.reshape(-1)]
    dis[rows == raw.indices] = 0.0
    dis_dev = torch.from_numpy(dis).to(dev)

    host, device, once = Clock(), Clock(), Clock()
    np.random.seed(7)
    cur, host_graphs = raw, []
    for _ in range(rounds):
        with host.part("graph_nsgt"):
            cur = T.graph_nsgt(raw, dis, cur)
        with host.part("normalize_adj_tensor"):
            norm = T.normalize_adj_tensor(cur)
        with host.part("FullGraphAdj"):
            full = FullGraphAdj(norm, raw, dev)
        host_graphs.append((int(norm.nnz), norm.data.copy()))
        del full
    np.random.seed(7)
    with once.part("DeviceNsgt"):
        tree = T.DeviceNsgt(raw, dis_dev, dev)
    with once.part("base FullGraphAdj"):
        ones = sp.csr_matrix((np.ones(raw.nnz, np.float32), raw.indices, raw.indptr), shape=raw.shape)
        base = FullGraphAdj(T.normalize_adj_tensor(ones), raw, dev)
    same = True
    for k in range(rounds):
        with device.part("DeviceNsgt.step"):
            csr = tree.step()
        with device.part("with_adjacency"):
            full = FullGraphAdj.with_adjacency(base, *csr)
        same = same and full.A.nnz == host_graphs[k][0] and np.array_equal(full.A.host.data, host_graphs[k][1])
        del full
    tot = lambda c: [float(sum(v[k] for v in c.parts.values())) for k in range(rounds)]      # noqa: E731
    return dict(nodes=int(n), entries=int(raw.nnz), entries_after=[g[0] for g in host_graphs], graphs_equal=bool(same),
                host_s={k: [float(x) for x in v] for k, v in host.parts.items()}, host_total_s=tot(host),
                device_s={k: [float(x) for x in v] for k, v in device.parts.items()}, device_total_s=tot(device),
                device_once_s={k: float(v[0]) for k, v in once.parts.items()})


def whole_run_seconds(dataset, num_epoch, device_cut):
    argv = ["tam.py", "--dataset", dataset, "--synthetic", "--quiet", "--cutting", "3", "--num_epoch", str(num_epoch)]
    if device_cut:
        argv.append("--device_cut")
    out = io.StringIO()
    old = sys.argv
    sys.argv = argv
    try:
        with contextlib.redirect_stdout(out):
            tam.main()
    finally:
        sys.argv = old
    lines = out.getvalue().strip().splitlines()
    return float(lines[-2]), lines[-3]                           # the script's own `end - start`; its last AUC line


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", type=str, default="reddit,Amazon,t_finance")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--runs", type=str, default="reddit,Amazon,t_finance")
    p.add_argument("--num_epoch", type=int, default=500)
    p.add_argument("--repeats", type=int, default=2)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tam_cut_time.py needs an MI355X")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    line = dict(what="TAM truncation round: (setup) seconds per round of the work between two train_cut calls, host = graph_nsgt + "
                     "normalize_adj_tensor + FullGraphAdj (the path without --device_cut, unchanged), device = DeviceNsgt.step + "
                     "FullGraphAdj.with_adjacency, device_once = per run; synthetic graphs of the published sizes, random symmetric "
                     "distances, a synchronise around every part; (runs) the seconds tam.py --synthetic --cutting 3 prints at its end, "
                     "the two paths alternating after a 5-epoch run of each",
                device=torch.cuda.get_device_name(0), host_threads=torch.get_num_threads(), rounds=a.rounds, num_epoch=a.num_epoch, repeats=a.repeats,
                setup={}, runs={})
    for d in [s for s in a.sizes.split(",") if s]:
        line["setup"][d] = setup_times(d, a.rounds, dev)
        print(d, json.dumps(line["setup"][d]), flush=True)
    for d in [s for s in a.runs.split(",") if s]:
        for flag in (False, True):                                  # first launches, allocator, plan caches: not in the timed runs
            whole_run_seconds(d, 5, flag)
        host_s, dev_s, equal = [], [], True
        for _ in range(a.repeats):                                  # alternating, one process
            hs, host_auc = whole_run_seconds(d, a.num_epoch, False)
            ds, dev_auc = whole_run_seconds(d, a.num_epoch, True)
            host_s.append(hs)
            dev_s.append(ds)
            equal = equal and host_auc == dev_auc
        line["runs"][d] = dict(host_s=host_s, device_cut_s=dev_s, last_auc_line_equal=bool(equal))
        print(d, json.dumps(line["runs"][d]), flush=True)
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
