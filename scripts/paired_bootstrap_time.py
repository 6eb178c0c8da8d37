#!/usr/bin/env python3
"""What the paired stratified bootstrap of two models' average precision costs on the device: `ggad_rank_bootstrap_pair_f32`
(csrc/rank_metrics.hip) against two unpaired `ggad_rank_bootstrap_f32` calls and against a torch restatement of the same paired scheme.

    python scripts/paired_bootstrap_time.py [--warmup 2] [--reps 9] [--boot 1000] [--out profiles/paired_bootstrap_time_line.json]
    rocprofv3 --kernel-trace -d DIR -o t -- python scripts/paired_bootstrap_time.py --trace dgraph_like [--trace_calls 5]
    python scripts/rocpd_stats.py DIR/.../t_results.db STATS.csv
    python scripts/paired_bootstrap_time.py --shares STATS.csv --input dgraph_like --out profiles/paired_bootstrap_time_line.json

Two inputs, the seeded lists of scripts/bootstrap_time.py with a second model that is a noisy copy of the first (b = a + 0.3 N(0, 1)), on
the device: `dgraph_like` (n = 1,736,598, P = 8,313) and `five_tiles_cut` (n = 39,216, P = 9,216).  For every input the routes are
alternated in ONE process, a device synchronise around each timed part, every route run `--warmup` times before it is timed, medians
of `--reps` with min-max (all values are kept); `pos_cap` = P, B = `--boot` replicates:

  fronts          two `ggad_rank_wide_f32` calls, into buffers allocated beforehand, no read-back: what the pair call runs first
  pair            the launches of `ggad_rank_bootstrap_pair_f32` alone, likewise (no `hist_out`)
  compare_ap      the public `metrics.compare_ap`: workspace allocation, the launches, one read-back of 24 + 4 B words, the quantiles
  two_unpaired    two `ggad_rank_bootstrap_f32` calls, one per model: the unpaired price, for contrast
  torch_pair      a torch restatement on the device of the SAME paired scheme: per model the positives sorted, every element's rank or
                  (ub, tie) by `searchsorted`; then per chunk of replicates `randint` over the positive and the negative numbers, one
                  gather per model and draw, `bincount` into (w, cU, cE), `cumsum`, the two sums; one read-back.  torch's generator, so
                  its replicates differ from the kernel's: the standard errors of both differences are in the line
The cell kernel and the replicate kernel are told apart by a kernel trace in a run of its own (`--trace`, `--shares`: the per-kernel
microseconds of ONE pair call go into `by_input[NAME].pair_kernels_us`).  Prints and writes one JSON line."""
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
from ggad_amd.metrics import compare_ap  # noqa: E402

INPUTS = (("dgraph_like", 1_736_598, 8313, None), ("five_tiles_cut", 70000, 40000, "cap"))
CHUNK_DRAWS = 1 << 25                        # draws of the negatives per chunk of the torch restatement (256 MB of int64)
PAIR_KERNELS = ("k_rw_scan", "k_rw_sort", "k_rw_merge", "k_rw_bucket", "k_rw_terms", "k_rw_final", "k_rp_cells", "k_rp_boot")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(xs):
    return dict(median_s=float(statistics.median(xs)), min_s=float(min(xs)), max_s=float(max(xs)), all_s=[float(x) for x in xs])


def make_input(n, p, cut, dev):
    rng = np.random.default_rng(72)
    s = rng.random(n).astype(np.float32)
    y = np.zeros(n, dtype=np.uint8)
    y[np.random.default_rng(p).choice(n, p, replace=False)] = 1
    if cut is not None:
        keep = np.ones(n, dtype=bool)
        keep[np.flatnonzero(y == 1)[cut:]] = False
        s, y = s[keep], y[keep]
    sb = (s + 0.3 * np.random.default_rng(73).standard_normal(len(s))).astype(np.float32)
    return tuple(torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (s, sb, y))


def torch_pair(sa, sb, yd, reps, gen):
    """(AP*_A - AP*_B float64[reps], AUROC*_A - AUROC*_B float64[reps]) on the host."""
    mask = yd == 1
    P, Nn = int(mask.sum()), int((~mask).sum())
    tables = []
    for s in (sa, sb):
        pos = torch.sort(s[mask])[0]
        neg = s[~mask]
        ub = torch.searchsorted(pos, neg, right=True)
        tie = (ub >= 1) & (pos[(ub - 1).clamp(min=0)] == neg)
        rank = torch.searchsorted(pos, s[mask])
        tables.append((rank, ub, tie, torch.searchsorted(pos, pos), torch.searchsorted(pos, pos, right=True) - 1))
    aps, nums = ([], []), ([], [])
    chunk = max(1, min(reps, CHUNK_DRAWS // max(Nn, 1)))
    for r0 in range(0, reps, chunk):
        c = min(chunk, reps - r0)
        row = (torch.arange(c, device=sa.device) * (P + 1)).unsqueeze(1)
        j = torch.randint(0, P, (c, P), device=sa.device, generator=gen)
        u = torch.randint(0, Nn, (c, Nn), device=sa.device, generator=gen)
        for m, (rank, ub, tie, run_s, run_e) in enumerate(tables):
            w = torch.bincount((rank[j] + row).reshape(-1), minlength=c * (P + 1)).view(c, P + 1)[:, :P]
            b = ub[u]
            c_u = torch.bincount((b + row).reshape(-1), minlength=c * (P + 1)).view(c, P + 1)
            c_e = torch.bincount((b - 1 + row)[tie[u]], minlength=c * (P + 1)).view(c, P + 1)
            del b
            L = torch.cumsum(c_u, 1)[:, :P]
            suffix = torch.flip(torch.cumsum(torch.flip(w, (1,)), 1), (1,))
            tp = suffix[:, run_s]
            q = (w * tp).double() / (tp + Nn - L).double()
            aps[m].append(torch.where(w > 0, q, torch.zeros_like(q)).sum(1) / P)
            nums[m].append((w * (2 * L + c_e[:, run_e])).sum(1))
    ap = [torch.cat(a).cpu().numpy() for a in aps]
    num = [torch.cat(a).cpu().numpy() for a in nums]
    return ap[0] - ap[1], (num[0] - num[1]).astype(np.float64) / float(2 * P * Nn)


def trace(name, calls, B):
    n, p, cut = next(c[1:] for c in INPUTS if c[0] == name)
    dev = "cuda:0"
    lib = _lib.load()
    s, sb, yd = make_input(n, p, int(lib.ggad_rank_bootstrap_max_pos()) if cut else None, dev)
    n, p = s.numel(), int(yd.sum())
    ws = torch.empty(int(lib.ggad_rank_bootstrap_pair_workspace_elems(n, p)), dtype=torch.int32, device=dev)
    out24 = torch.empty(24, dtype=torch.float64, device=dev)
    rep_ap = torch.empty(2 * B, dtype=torch.float64, device=dev)
    rep_num = torch.empty(2 * B, dtype=torch.int64, device=dev)
    for _ in range(calls):
        _lib.call("ggad_rank_bootstrap_pair_f32", _lib.ptr(s), _lib.ptr(sb), _lib.ptr(yd), n, p, 0.5, 72, B, _lib.ptr(out24), _lib.ptr(rep_ap),
                  _lib.ptr(rep_num), 0, _lib.ptr(ws))
    torch.cuda.synchronize()
    print("traced", calls, "calls on", name, "status", out24[23].item())


def shares(csv_path, name, out):
    """Per-kernel microseconds of ONE pair call from the stats of a `--trace` run, into `by_input[name]` of the line at `out`."""
    per = {}
    for ln in open(csv_path).read().splitlines()[1:]:
        k, n_calls, total_us = ln.split(",")[:3]
        if k in PAIR_KERNELS:
            per[k] = (int(n_calls), float(total_us))
    calls = per["k_rp_boot"][0]
    us = {k: v[1] / calls for k, v in per.items()}                 # (the front's kernels run twice or more per call: summed)
    whole = sum(us.values())
    rec = dict(calls_traced=calls, per_call_us={k: round(v, 2) for k, v in us.items()}, kernels_total_us=round(whole, 2),
               cells_share=round(us["k_rp_cells"] / whole, 4), replicates_share=round(us["k_rp_boot"] / whole, 4))
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
    ap.add_argument("--boot", type=int, default=1000)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--trace", type=str, default=None, metavar="NAME")
    ap.add_argument("--trace_calls", type=int, default=5)
    ap.add_argument("--shares", type=str, default=None, metavar="STATS.csv")
    ap.add_argument("--input", type=str, default=None, metavar="NAME")
    a = ap.parse_args()
    if a.shares:
        return shares(a.shares, a.input, a.out)
    if not torch.cuda.is_available():
        sys.exit("paired_bootstrap_time.py needs an MI355X")
    if a.trace:
        return trace(a.trace, a.trace_calls, a.boot)
    dev = "cuda:0"
    lib = _lib.load()
    cap = int(lib.ggad_rank_bootstrap_max_pos())
    B = a.boot
    line = dict(what="paired stratified bootstrap of two models' average precision and AUROC, B replicates of n float32 scores with P "
                     "positives: seconds, the routes alternated in one process, a device synchronise around every part, medians after "
                     "warm-up with min-max", device=torch.cuda.get_device_name(0), warmup=a.warmup, reps=a.reps, replicates=B, by_input={})
    for name, n, p, cut in INPUTS:
        s, sb, yd = make_input(n, p, cap if cut else None, dev)
        n, p = s.numel(), int(yd.sum())
        ws = torch.empty(int(lib.ggad_rank_bootstrap_pair_workspace_elems(n, p)), dtype=torch.int32, device=dev)
        half = int(lib.ggad_rank_bootstrap_workspace_elems(n, p))
        out8 = torch.empty(16, dtype=torch.float64, device=dev)
        out24 = torch.empty(24, dtype=torch.float64, device=dev)
        out16 = torch.empty(32, dtype=torch.float64, device=dev)
        rep_ap = torch.empty(2 * B, dtype=torch.float64, device=dev)
        rep_num = torch.empty(2 * B, dtype=torch.int64, device=dev)
        one_ap = torch.empty(2 * B, dtype=torch.float64, device=dev)
        one_num = torch.empty(2 * B, dtype=torch.int64, device=dev)
        gen = torch.Generator(device=dev).manual_seed(72)
        second = (half + 3) // 4 * 16                              # byte offset of a second, 16-byte aligned chain workspace inside ws

        def fronts():
            for m, x in enumerate((s, sb)):
                _lib.call("ggad_rank_wide_f32", _lib.ptr(x), _lib.ptr(yd), n, p, 0.5, _lib.ptr(out8) + 64 * m, _lib.ptr(ws) + second * m)

        def pair():
            _lib.call("ggad_rank_bootstrap_pair_f32", _lib.ptr(s), _lib.ptr(sb), _lib.ptr(yd), n, p, 0.5, 72, B, _lib.ptr(out24),
                      _lib.ptr(rep_ap), _lib.ptr(rep_num), 0, _lib.ptr(ws))

        def two_unpaired():
            for m, x in enumerate((s, sb)):
                _lib.call("ggad_rank_bootstrap_f32", _lib.ptr(x), _lib.ptr(yd), n, p, 0.5, 72 + m, B, _lib.ptr(out16) + 128 * m,
                          _lib.ptr(one_ap) + 8 * B * m, _lib.ptr(one_num) + 8 * B * m, 0, _lib.ptr(ws) + second * m)

        routes = dict(fronts=fronts, pair=pair, compare_ap=lambda: compare_ap(s, sb, yd, reps=B, seed=72, pos_cap=p),
                      two_unpaired=two_unpaired, torch_pair=lambda: torch_pair(s, sb, yd, B, gen))
        for _ in range(a.warmup):
            for fn in routes.values():
                timed(fn)
        times = {k: [] for k in routes}
        res = {}
        for _ in range(a.reps):                                    # alternating
            for k, fn in routes.items():
                t, res[k] = timed(fn)
                times[k].append(t)
        pair()                                                     # (the buffers hold the pair call's words again)
        torch.cuda.synchronize()
        c, (t_ap, t_auc) = res["compare_ap"], res["torch_pair"]
        rec = {k: summary(v) for k, v in times.items()}
        med = {k: rec[k]["median_s"] for k in routes}
        kernel_diff = (rep_ap[:B] - rep_ap[B:]).cpu().numpy()
        unpaired = (one_ap[:B] - one_ap[B:]).cpu().numpy()
        rec.update(n=n, positives=p, workspace_bytes=int(ws.numel() * 4), cells_and_replicates_s=med["pair"] - med["fronts"],
                   draws_per_model=int(n * B), gathers_per_s=float(2 * n * B / max(med["pair"] - med["fronts"], 1e-12)),
                   status=float(out24[23].item()), kernel_replicates_equal_compare_ap=bool(np.array_equal(kernel_diff, c.diff_reps)),
                   ap_a=c.ap_a, ap_b=c.ap_b, diff=c.diff, diff_se=c.diff_se, diff_lo=c.diff_lo, diff_hi=c.diff_hi, p=c.p,
                   auc_diff=c.auc_diff, auc_diff_se=c.auc_diff_se, torch_diff_se=float(t_ap.std(ddof=1)),
                   torch_auc_diff_se=float(t_auc.std(ddof=1)), unpaired_diff_se=float(unpaired.std(ddof=1)),
                   pair_over_two_unpaired=med["pair"] / med["two_unpaired"], torch_over_pair=med["torch_pair"] / med["pair"])
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
