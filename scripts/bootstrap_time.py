#!/usr/bin/env python3
"""What the stratified bootstrap of average precision costs on the device: `ggad_rank_bootstrap_f32` (csrc/rank_metrics.hip) against the
rank metrics it extends and against a torch restatement of the same scheme.

    python scripts/bootstrap_time.py [--warmup 2] [--reps 9] [--boot 1000] [--out profiles/bootstrap_time_line.json]

Two inputs, seeded uniform float32 scores with exactly P label-1 entries at seeded places, on the device: `dgraph_like` (n = 1,736,598,
P = 8,313: the DGraph-Fin test sweep) and `five_tiles_cut` (the 70,000 scores with 40,000 positives of the other time lines with the
positives beyond ggad_rank_bootstrap_max_pos() = 9,216 dropped: n = 39,216).  For every input the routes are alternated in ONE process,
a device synchronise around each timed part, every route run `--warmup` times before it is timed, medians of `--reps` with min-max (all
values are kept); `pos_cap` = P, B = `--boot` replicates:

  rank_wide       the launches of `ggad_rank_wide_f32` alone, into buffers allocated beforehand, no read-back
  bootstrap       the launches of `ggad_rank_bootstrap_f32` alone, likewise (no `hist_out`): minus rank_wide = the replicate kernel
  ap_ci           the public `metrics.ap_ci`: workspace allocation, the launches, one read-back of 16 + 2 B words, the quantiles
  torch_boot      a torch restatement on the device of the SAME scheme (bins, not elements): the positives sorted, the negatives
                  binned by `searchsorted` + `bincount`; then per chunk of replicates `randint` over the ranks and over the negatives,
                  `searchsorted` in the prefix of histU, `bincount` into (w, cU, cE), `cumsum`, the two sums; one read-back.  torch's
                  generator, so its replicates differ from the kernel's: the standard errors of both are in the line
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
from ggad_amd.metrics import ap_ci  # noqa: E402

INPUTS = (("dgraph_like", 1_736_598, 8313, None), ("five_tiles_cut", 70000, 40000, "cap"))
CHUNK_DRAWS = 1 << 25                        # draws of the negatives per chunk of the torch restatement (256 MB of int64)


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
    return torch.from_numpy(np.ascontiguousarray(s)).to(dev), torch.from_numpy(np.ascontiguousarray(y)).to(dev)


def torch_boot(s, yd, reps, gen):
    """(AP* float64[reps], AUROC* float64[reps]) on the host."""
    mask = yd == 1
    pos = torch.sort(s[mask])[0]
    neg = s[~mask]
    P, Nn = pos.numel(), neg.numel()
    ub = torch.searchsorted(pos, neg, right=True)
    hist_u = torch.bincount(ub, minlength=P + 1)
    tie = (ub >= 1) & (pos[(ub - 1).clamp_(min=0)] == neg)
    hist_e = torch.bincount(ub[tie] - 1, minlength=P + 1)
    cum = torch.cumsum(hist_u, 0)
    start = cum - hist_u
    run_s, run_e = torch.searchsorted(pos, pos), torch.searchsorted(pos, pos, right=True) - 1
    aps, nums = [], []
    chunk = max(1, min(reps, CHUNK_DRAWS // max(Nn, 1)))
    for r0 in range(0, reps, chunk):
        c = min(chunk, reps - r0)
        row = (torch.arange(c, device=s.device) * (P + 1)).unsqueeze(1)
        k = torch.randint(0, P, (c, P), device=s.device, generator=gen)
        w = torch.bincount((k + row).reshape(-1), minlength=c * (P + 1)).view(c, P + 1)[:, :P]
        u = torch.randint(0, Nn, (c, Nn), device=s.device, generator=gen)
        b = torch.searchsorted(cum, u, right=True)
        c_u = torch.bincount((b + row).reshape(-1), minlength=c * (P + 1)).view(c, P + 1)
        below = (b - 1).clamp_(min=0)
        tied = (b >= 1) & (u - start[b] < hist_e[below])
        c_e = torch.bincount((below + row)[tied], minlength=c * (P + 1)).view(c, P + 1)
        del u, b, below, tied
        L = torch.cumsum(c_u, 1)[:, :P]
        suffix = torch.flip(torch.cumsum(torch.flip(w, (1,)), 1), (1,))
        tp = suffix[:, run_s]
        q = (w * tp).double() / (tp + Nn - L).double()
        aps.append(torch.where(w > 0, q, torch.zeros_like(q)).sum(1) / P)
        nums.append((w * (2 * L + c_e[:, run_e])).sum(1))
    ap, num = torch.cat(aps).cpu().numpy(), torch.cat(nums).cpu().numpy()
    return ap, num.astype(np.float64) / float(2 * P * Nn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--boot", type=int, default=1000)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bootstrap_time.py needs an MI355X")
    dev = "cuda:0"
    lib = _lib.load()
    cap = int(lib.ggad_rank_bootstrap_max_pos())
    B = a.boot
    line = dict(what="stratified bootstrap of average precision and AUROC, B replicates of n float32 scores with P positives: seconds, the "
                     "routes alternated in one process, a device synchronise around every part, medians after warm-up with min-max",
                device=torch.cuda.get_device_name(0), warmup=a.warmup, reps=a.reps, replicates=B, by_input={})
    for name, n, p, cut in INPUTS:
        s, yd = make_input(n, p, cap if cut else None, dev)
        n, p = s.numel(), int(yd.sum())
        ws = torch.empty(int(lib.ggad_rank_bootstrap_workspace_elems(n, p)), dtype=torch.int32, device=dev)
        out8 = torch.empty(8, dtype=torch.float64, device=dev)
        out16 = torch.empty(16, dtype=torch.float64, device=dev)
        rep_ap = torch.empty(B, dtype=torch.float64, device=dev)
        rep_num = torch.empty(B, dtype=torch.int64, device=dev)
        gen = torch.Generator(device=dev).manual_seed(72)

        def rank_wide():
            _lib.call("ggad_rank_wide_f32", _lib.ptr(s), _lib.ptr(yd), n, p, 0.5, _lib.ptr(out8), _lib.ptr(ws))

        def bootstrap():
            _lib.call("ggad_rank_bootstrap_f32", _lib.ptr(s), _lib.ptr(yd), n, p, 0.5, 72, B, _lib.ptr(out16), _lib.ptr(rep_ap),
                      _lib.ptr(rep_num), 0, _lib.ptr(ws))

        routes = dict(rank_wide=rank_wide, bootstrap=bootstrap, ap_ci=lambda: ap_ci(s, yd, reps=B, seed=72, pos_cap=p),
                      torch_boot=lambda: torch_boot(s, yd, B, gen))
        for _ in range(a.warmup):
            for fn in routes.values():
                timed(fn)
        times = {k: [] for k in routes}
        res = {}
        for _ in range(a.reps):                                    # alternating
            for k, fn in routes.items():
                t, res[k] = timed(fn)
                times[k].append(t)
        ci, (t_ap, t_auc) = res["ap_ci"], res["torch_boot"]
        rec = {k: summary(v) for k, v in times.items()}
        med = {k: rec[k]["median_s"] for k in routes}
        rec.update(n=n, positives=p, workspace_bytes=int(ws.numel() * 4), replicate_kernel_s=med["bootstrap"] - med["rank_wide"],
                   negative_draws=int((n - p) * B), draws_per_s=float((n - p) * B / max(med["bootstrap"] - med["rank_wide"], 1e-12)),
                   out8_bits_equal=bool(torch.equal(out8.view(torch.int64), out16[:8].view(torch.int64))), status=float(out16[15].item()),
                   kernel_replicates_equal_ap_ci=bool(np.array_equal(rep_ap.cpu().numpy(), ci.ap_reps)),
                   ap=ci.ap, ap_se=ci.ap_se, ap_lo=ci.ap_lo, ap_hi=ci.ap_hi, ap_bias=ci.ap_bias, auc=ci.auc, auc_se=ci.auc_se,
                   torch_ap_se=float(t_ap.std(ddof=1)), torch_auc_se=float(t_auc.std(ddof=1)), torch_ap_mean=float(t_ap.mean()),
                   kernel_ap_mean=float(ci.ap_reps.mean()), torch_over_bootstrap=med["torch_boot"] / med["bootstrap"])
        line["by_input"][name] = rec
        print(name, json.dumps(rec), flush=True)
        del ws, yd, s
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
