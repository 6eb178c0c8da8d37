#!/usr/bin/env python3
"""What choosing the alert threshold on the device costs: `ggad_rank_operating_f32` (csrc/rank_metrics.hip) against the rank metrics it
extends and against a torch route.

    python scripts/operating_point_time.py [--warmup 2] [--reps 9] [--out profiles/operating_point_time_line.json]

Three inputs, seeded uniform float32 scores with exactly P label-1 entries at seeded places, on the device: `dgraph_like` (n = 1,736,598,
P = 8,313: the DGraph-Fin test sweep), `five_tiles` (n = 70,000, P = 40,000) and `at_wide_cap` (n = 1,051,576, P = 1,048,576) -- the
shapes of the cases of those names in tests/rank_wide_ref.py.  For every input the routes are alternated in ONE process, a device
synchronise around each timed part, every route run `--warmup` times before it is timed, medians of `--reps` with min-max (all values
are kept); `pos_cap` = P, criterion `f1`:

  rank_wide          the launches of `ggad_rank_wide_f32` alone, into buffers allocated beforehand, no read-back
  operating          the launches of `ggad_rank_operating_f32` alone, likewise: minus rank_wide = the price of the arg-max
  operating_curve    the same with the three curve arrays: minus operating = the price of the curve stores
  operating_point    the public `metrics.operating_point`: workspace allocation, the launches, one read-back of sixteen doubles
  torch              a stable descending `torch.sort`, two cumulative sums, the last element of every run of equal scores, F1 in
                     float64 and `argmax`, one read-back of the index (no exact comparison, no stated tie rule)

The chosen thresholds and counts of the routes are compared.  Prints and writes one JSON line."""
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
from ggad_amd.metrics import operating_point  # noqa: E402

INPUTS = (("dgraph_like", 1_736_598, 8313), ("five_tiles", 70000, 40000), ("at_wide_cap", (1 << 20) + 3000, 1 << 20))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(xs):
    return dict(median_s=float(statistics.median(xs)), min_s=float(min(xs)), max_s=float(max(xs)), all_s=[float(x) for x in xs])


def torch_route(scores, yd, n_pos):
    s, order = torch.sort(scores, descending=True, stable=True)
    y = yd[order].to(torch.int64)
    tp = torch.cumsum(y, 0)
    fp = torch.cumsum(1 - y, 0)
    last = torch.ones_like(y, dtype=torch.bool)
    last[:-1] = s[:-1] != s[1:]
    f1 = torch.where(last, 2.0 * tp.double() / (tp + fp + n_pos).double(), torch.zeros((), dtype=torch.float64, device=s.device))
    i = int(torch.argmax(f1))
    return float(s[i]), int(tp[i]), int(fp[i])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("operating_point_time.py needs an MI355X")
    dev = "cuda:0"
    lib = _lib.load()
    line = dict(what="the operating point (criterion f1) of n float32 scores with P positives: seconds, the routes alternated in one "
                     "process, a device synchronise around every part, medians after warm-up with min-max",
                device=torch.cuda.get_device_name(0), warmup=a.warmup, reps=a.reps, by_input={})
    for name, n, p in INPUTS:
        scores = torch.from_numpy(np.random.default_rng(72).random(n).astype(np.float32)).to(dev)
        y = np.zeros(n, dtype=np.uint8)
        y[np.random.default_rng(p).choice(n, p, replace=False)] = 1
        yd = torch.from_numpy(y).to(dev)
        ws = torch.empty(int(lib.ggad_rank_operating_workspace_elems(n, p)), dtype=torch.int32, device=dev)
        out8 = torch.empty(8, dtype=torch.float64, device=dev)
        out16 = torch.empty(16, dtype=torch.float64, device=dev)
        out16c = torch.empty(16, dtype=torch.float64, device=dev)
        ct, ctp, cfp = (torch.empty(p, dtype=torch.float32, device=dev), torch.empty(p, dtype=torch.int32, device=dev),
                        torch.empty(p, dtype=torch.int32, device=dev))

        def rank_wide():
            _lib.call("ggad_rank_wide_f32", _lib.ptr(scores), _lib.ptr(yd), n, p, 0.5, _lib.ptr(out8), _lib.ptr(ws))

        def operating():
            _lib.call("ggad_rank_operating_f32", _lib.ptr(scores), _lib.ptr(yd), n, p, 0.5, 0, 0.0, _lib.ptr(out16), 0, 0, 0, _lib.ptr(ws))

        def operating_curve():
            _lib.call("ggad_rank_operating_f32", _lib.ptr(scores), _lib.ptr(yd), n, p, 0.5, 0, 0.0, _lib.ptr(out16c), _lib.ptr(ct),
                      _lib.ptr(ctp), _lib.ptr(cfp), _lib.ptr(ws))

        routes = dict(rank_wide=rank_wide, operating=operating, operating_curve=operating_curve,
                      operating_point=lambda: operating_point(scores, yd, "f1", pos_cap=p), torch=lambda: torch_route(scores, yd, p))
        for _ in range(a.warmup):
            for fn in routes.values():
                timed(fn)
        times = {k: [] for k in routes}
        res = {}
        for _ in range(a.reps):                                    # alternating
            for k, fn in routes.items():
                t, res[k] = timed(fn)
                times[k].append(t)
        o, op, tr = out16.cpu().tolist(), res["operating_point"], res["torch"]
        rec = {k: summary(v) for k, v in times.items()}
        med = {k: rec[k]["median_s"] for k in routes}
        rec.update(n=n, positives=p, workspace_bytes=int(ws.numel() * 4), status=int(o[15]), candidates=int(o[14]),
                   argmax_extra_s=med["operating"] - med["rank_wide"], curve_extra_s=med["operating_curve"] - med["operating"],
                   out8_bits_equal=bool(torch.equal(out8.view(torch.int64), out16[:8].view(torch.int64))),
                   curve_call_bits_equal=bool(torch.equal(out16.view(torch.int64), out16c.view(torch.int64))),
                   native_equals_public=bool((o[8], int(o[9]), int(o[10])) == (op.thres, op.tp, op.fp)),
                   torch_agrees=bool(tr == (op.thres, op.tp, op.fp)), thres=op.thres, tp=op.tp, fp=op.fp, value=op.value)
        line["by_input"][name] = rec
        print(name, json.dumps(rec), flush=True)
        del ws, yd, scores, ct, ctp, cfp
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
