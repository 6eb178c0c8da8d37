#!/usr/bin/env python3
"""What DeLong's variance and the paired test cost on the device: `ggad_rank_delong_f32` and `ggad_rank_delong_pair_f32`
(csrc/rank_metrics.hip) against the rank metrics they extend and against a torch restatement.

    python scripts/delong_time.py [--warmup 2] [--reps 9] [--out profiles/delong_time_line.json]
    rocprofv3 --kernel-trace -d DIR -o t -- python scripts/delong_time.py --trace dgraph_like [--trace_calls 20]
    python scripts/rocpd_stats.py DIR/.../t_results.db STATS.csv
    python scripts/delong_time.py --shares STATS.csv --input dgraph_like --out profiles/delong_time_line.json

Two inputs, seeded uniform float32 scores with exactly P label-1 entries at seeded places, on the device: `dgraph_like` (n = 1,736,598,
P = 8,313: the DGraph-Fin test sweep) and `five_tiles` (n = 70,000, P = 40,000); the second list is the first plus N(0, 0.5^2) noise.
For every input the routes are alternated in ONE process, a device synchronise around each timed part, every route run `--warmup`
times before it is timed, medians of `--reps` with min-max (all values are kept); `pos_cap` = P:

  rank_wide       the launches of `ggad_rank_wide_f32` alone, into buffers allocated beforehand, no read-back
  delong          the launches of `ggad_rank_delong_f32` alone, likewise: minus rank_wide = the price of the 128-bit sums
  delong_pair     the launches of `ggad_rank_delong_pair_f32` alone, likewise
  auc_ci          the public `metrics.auc_ci`: workspace allocation, the launches, one read-back of sixteen doubles
  compare_auc     the public `metrics.compare_auc`, likewise, twenty-four doubles
  torch_ci        a torch restatement of the variance: two stable sorts, four `searchsorted`, float64 sums, one read-back
  torch_pair      the same for two lists with the covariance (four sorts, eight `searchsorted`)

`--trace NAME` only calls `ggad_rank_delong_pair_f32` on that input, for a kernel trace; `--shares` folds the per-kernel averages of
such a trace (scripts/rocpd_stats.py) into the line as `by_input[NAME].pair_kernels_us` with the cross kernel's share of the call.
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
from ggad_amd import _lib  # noqa: E402
from ggad_amd.metrics import auc_ci, compare_auc  # noqa: E402

INPUTS = (("dgraph_like", 1_736_598, 8313), ("five_tiles", 70000, 40000))
PAIR_KERNELS = ("k_rw_scan", "k_rw_sort", "k_rw_merge", "k_rw_bucket", "k_rd_terms_lt", "k_rd_cross", "k_rd_pair_final")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(xs):
    return dict(median_s=float(statistics.median(xs)), min_s=float(min(xs)), max_s=float(max(xs)), all_s=[float(x) for x in xs])


def make_input(n, p, dev):
    rng = np.random.default_rng(72)
    s = rng.random(n).astype(np.float32)
    sb = (s + np.float32(0.5) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    y = np.zeros(n, dtype=np.uint8)
    y[np.random.default_rng(p).choice(n, p, replace=False)] = 1
    return torch.from_numpy(s).to(dev), torch.from_numpy(sb).to(dev), torch.from_numpy(y).to(dev)


def _placements(s, pos_mask):
    pos, neg = s[pos_mask], s[~pos_mask]
    ps, ns = torch.sort(pos, stable=True)[0], torch.sort(neg, stable=True)[0]
    a = (torch.searchsorted(ns, pos) + torch.searchsorted(ns, pos, right=True)).double() / (2.0 * neg.numel())
    b = (2 * pos.numel() - torch.searchsorted(ps, neg) - torch.searchsorted(ps, neg, right=True)).double() / (2.0 * pos.numel())
    return a, b


def torch_ci(s, yd):
    a, b = _placements(s, yd == 1)
    return float(a.mean()), float(a.var(unbiased=True) / a.numel() + b.var(unbiased=True) / b.numel())


def torch_pair(s, sb, yd):
    mask = yd == 1
    (a1, b1), (a2, b2) = _placements(s, mask), _placements(sb, mask)
    da, db = a1 - a2, b1 - b2
    var_diff = da.var(unbiased=True) / da.numel() + db.var(unbiased=True) / db.numel()
    return float(da.mean()), float(var_diff)


def trace(name, calls):
    n, p = next(c[1:] for c in INPUTS if c[0] == name)
    dev = "cuda:0"
    lib = _lib.load()
    s, sb, yd = make_input(n, p, dev)
    ws = torch.empty(int(lib.ggad_rank_delong_pair_workspace_elems(n, p)), dtype=torch.int32, device=dev)
    out24 = torch.empty(24, dtype=torch.float64, device=dev)
    sums = torch.empty(24, dtype=torch.int64, device=dev)
    for _ in range(calls):
        _lib.call("ggad_rank_delong_pair_f32", _lib.ptr(s), _lib.ptr(sb), _lib.ptr(yd), n, p, 0.5, _lib.ptr(out24), _lib.ptr(sums), _lib.ptr(ws))
    torch.cuda.synchronize()
    print("traced", calls, "calls on", name, "status", out24[23].item())


def shares(csv_path, name, out):
    """Per-kernel microseconds of ONE pair call from the stats of a `--trace` run, into `by_input[name]` of the line at `out`."""
    per = {}
    calls = None
    for ln in open(csv_path).read().splitlines()[1:]:
        k, n_calls, total_us = ln.split(",")[:3]
        if k in PAIR_KERNELS:
            per[k] = (int(n_calls), float(total_us))
        if k == "k_rd_pair_final":
            calls = int(n_calls)
    us = {k: v[1] / calls for k, v in per.items()}                 # (the front's kernels run twice or more per call: summed)
    whole = sum(us.values())
    rec = dict(calls_traced=calls, per_call_us={k: round(v, 2) for k, v in us.items()}, kernels_total_us=round(whole, 2),
               cross_share=round(us["k_rd_cross"] / whole, 4))
    with open(out) as fh:
        line = json.loads(fh.read())
    line["by_input"][name]["pair_kernels_us"] = rec
    with open(out, "w") as fh:
        fh.write(json.dumps(line) + "\n")
    print(name, json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--trace", type=str, default=None, metavar="NAME")
    ap.add_argument("--trace_calls", type=int, default=20)
    ap.add_argument("--shares", type=str, default=None, metavar="STATS.csv")
    ap.add_argument("--input", type=str, default=None, metavar="NAME")
    a = ap.parse_args()
    if a.shares:
        return shares(a.shares, a.input, a.out)
    if not torch.cuda.is_available():
        sys.exit("delong_time.py needs an MI355X")
    if a.trace:
        return trace(a.trace, a.trace_calls)
    dev = "cuda:0"
    lib = _lib.load()
    line = dict(what="DeLong's variance of the AUROC and the paired test of two score lists, n float32 scores with P positives: seconds, "
                     "the routes alternated in one process, a device synchronise around every part, medians after warm-up with min-max",
                device=torch.cuda.get_device_name(0), warmup=a.warmup, reps=a.reps, by_input={})
    for name, n, p in INPUTS:
        s, sb, yd = make_input(n, p, dev)
        ws = torch.empty(int(lib.ggad_rank_delong_pair_workspace_elems(n, p)), dtype=torch.int32, device=dev)
        out8 = torch.empty(8, dtype=torch.float64, device=dev)
        out16 = torch.empty(16, dtype=torch.float64, device=dev)
        out24 = torch.empty(24, dtype=torch.float64, device=dev)
        sums = torch.empty(24, dtype=torch.int64, device=dev)

        def rank_wide():
            _lib.call("ggad_rank_wide_f32", _lib.ptr(s), _lib.ptr(yd), n, p, 0.5, _lib.ptr(out8), _lib.ptr(ws))

        def delong():
            _lib.call("ggad_rank_delong_f32", _lib.ptr(s), _lib.ptr(yd), n, p, 0.5, _lib.ptr(out16), _lib.ptr(sums), _lib.ptr(ws))

        def delong_pair():
            _lib.call("ggad_rank_delong_pair_f32", _lib.ptr(s), _lib.ptr(sb), _lib.ptr(yd), n, p, 0.5, _lib.ptr(out24), _lib.ptr(sums),
                      _lib.ptr(ws))

        routes = dict(rank_wide=rank_wide, delong=delong, delong_pair=delong_pair, auc_ci=lambda: auc_ci(s, yd, pos_cap=p),
                      compare_auc=lambda: compare_auc(s, sb, yd, pos_cap=p), torch_ci=lambda: torch_ci(s, yd),
                      torch_pair=lambda: torch_pair(s, sb, yd))
        for _ in range(a.warmup):
            for fn in routes.values():
                timed(fn)
        times = {k: [] for k in routes}
        res = {}
        for _ in range(a.reps):                                    # alternating
            for k, fn in routes.items():
                t, res[k] = timed(fn)
                times[k].append(t)
        ci, cmp, tc, tp = res["auc_ci"], res["compare_auc"], res["torch_ci"], res["torch_pair"]
        rec = {k: summary(v) for k, v in times.items()}
        med = {k: rec[k]["median_s"] for k in routes}
        rec.update(n=n, positives=p, workspace_bytes=int(ws.numel() * 4), variance_extra_s=med["delong"] - med["rank_wide"],
                   out8_bits_equal=bool(torch.equal(out8.view(torch.int64), out16[:8].view(torch.int64))),
                   auc=ci.auc, var=ci.var, se=ci.se, var_diff=cmp.var_diff, z=cmp.z,
                   torch_var_rel_off=abs(tc[1] - ci.var) / ci.var, torch_var_diff_rel_off=abs(tp[1] - cmp.var_diff) / cmp.var_diff)
        line["by_input"][name] = rec
        print(name, json.dumps(rec), flush=True)
        del ws, yd, s, sb
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
