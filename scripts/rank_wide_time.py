#!/usr/bin/env python3
"""What the rank metrics cost above the 8,192 positives of csrc/rank_metrics.hip: `metrics.rank_report_wide` (csrc/rank_metrics.hip)
against what runs today.

    python scripts/rank_wide_time.py [--n 1736598] [--positives 8313,7427,65536,1048576] [--warmup 2] [--reps 7]
                                     [--out profiles/rank_wide_time_line.json]

`--n` seeded float32 scores (uniform, the size of the DGraph-Fin test sweep) with exactly P label-1 entries at seeded places, on the
device.  For every P the routes are alternated in ONE process, a device synchronise around each timed part, every route run
`--warmup` times before it is timed, medians of `--reps` with min-max (all values are kept):

  binary_report      two float64 device sorts: what `rank_report` falls back to above 8,192 positives (the real split today)
  rank_report        the four narrow counting launches (P <= 8,192 only: the price of the wide route where the narrow one would do)
  rank_report_wide   the public wide call with `pos_cap` = P: workspace allocation, the launches, one read-back
  native             the launches of `ggad_rank_wide_f32` alone, into buffers allocated beforehand, no read-back

The results of the routes are compared (integers equal, auc / ap differences).  Prints and writes one JSON line."""
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
from ggad_amd.metrics import binary_report, rank_report, rank_report_wide  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(xs):
    return dict(median_s=float(statistics.median(xs)), min_s=float(min(xs)), max_s=float(max(xs)), all_s=[float(x) for x in xs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_736_598)
    ap.add_argument("--positives", type=str, default="8313,7427,65536,1048576")
    ap.add_argument("--thres", type=float, default=0.4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rank_wide_time.py needs an MI355X")
    dev = "cuda:0"
    lib = _lib.load()
    narrow_cap, wide_cap = int(lib.ggad_rank_metrics_max_pos()), int(lib.ggad_rank_wide_max_pos())
    scores = torch.from_numpy(np.random.default_rng(72).random(a.n).astype(np.float32)).to(dev)
    line = dict(what="rank metrics of n float32 scores with P positives: seconds, the routes alternated in one process, a device "
                     "synchronise around every part, medians after warm-up with min-max",
                device=torch.cuda.get_device_name(0), n=a.n, narrow_max_pos=narrow_cap, wide_max_pos=wide_cap, warmup=a.warmup,
                reps=a.reps, by_positives={})
    for p in (int(x) for x in a.positives.split(",")):
        y = np.zeros(a.n, dtype=np.uint8)
        y[np.random.default_rng(p).choice(a.n, p, replace=False)] = 1
        yd = torch.from_numpy(y).to(dev)
        ws = torch.empty(int(lib.ggad_rank_wide_workspace_elems(a.n, p)), dtype=torch.int32, device=dev)
        out8 = torch.empty(8, dtype=torch.float64, device=dev)

        def native():
            _lib.call("ggad_rank_wide_f32", _lib.ptr(scores), _lib.ptr(yd), a.n, p, a.thres, _lib.ptr(out8), _lib.ptr(ws))

        routes = dict(binary_report=lambda: binary_report(scores, yd, a.thres),
                      rank_report_wide=lambda: rank_report_wide(scores, yd, a.thres, pos_cap=p), native=native)
        if p <= narrow_cap:
            routes["rank_report"] = lambda: rank_report(scores, yd, a.thres)
        for _ in range(a.warmup):
            for fn in routes.values():
                timed(fn)
        times = {k: [] for k in routes}
        res = {}
        for _ in range(a.reps):                                    # alternating
            for k, fn in routes.items():
                t, res[k] = timed(fn)
                times[k].append(t)
        b, w = res["binary_report"], res["rank_report_wide"]
        o = out8.cpu().tolist()
        rec = {k: summary(v) for k, v in times.items()}
        rec.update(workspace_bytes=int(ws.numel() * 4), status=int(o[7]),
                   integers_equal=all(b[k] == w[k] for k in ("tp", "fp", "fn", "tn", "f1_1", "f1_0", "f1_macro", "gmean")),
                   auc_abs_diff=abs(b["auc"] - w["auc"]), ap_abs_diff=abs(b["ap"] - w["ap"]),
                   native_equals_public=bool(o[0] == w["auc"] and o[1] == w["ap"]))
        if "rank_report" in res:
            rec.update(auc_equals_rank_report=bool(res["rank_report"]["auc"] == w["auc"]),
                       ap_abs_diff_rank_report=abs(res["rank_report"]["ap"] - w["ap"]))
        line["by_positives"][str(p)] = rec
        print(p, json.dumps(rec), flush=True)
        del ws, yd
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
