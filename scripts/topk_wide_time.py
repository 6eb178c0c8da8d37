#!/usr/bin/env python3
"""What the ranked list costs above 16,384 ranks: `ggad_topk_wide_f32` (csrc/topk.hip) against `ggad_topk_f32` where both serve
and against torch at every depth.

    python scripts/topk_wide_time.py [--scores 1736598] [--all 3700550] [--reps 7] [--warmup 3] [--profile-k K]
                                     [--out profiles/topk_wide_time_line.json]

The scores are float32 sigmoids of N(0, 10^2) logits drawn on the device from a fixed seed (the size of the DGraph-Fin test list, a
saturated head of exact 1.0f by the ten thousand, as the `saturated` case of tests/topk_ref.py), labels 0.42 % positive.  One process,
a device synchronise around every timed part, every part run `--warmup` times before it is timed, the routes alternating, medians of
`--reps` (all values kept).

  narrow        the six launches of `ggad_topk_f32` into buffers allocated beforehand (k up to 16,384, its cap)
  wide          the launches of `ggad_topk_wide_f32` into buffers allocated beforehand
  top_k         `metrics.top_k(scores, k, labels, wide=True)`: allocations, the launches and the read-back of the four meta words
  torch_sort    `torch.sort(scores, descending=True, stable=True)` cut at k, the labels gathered at its indices and `cumsum`: the route a
                user has today, with the same definition (ties by position); its positions are compared to wide's

on `--scores` scores at k = 1,000, 8,192 and 16,384 (where both calls serve), 65,536, 2^20 and k = n (the full ranking), and on `--all`
scores at k = 2^22.
`--profile-k K`: only warm up and repeat the wide call at that k on `--scores` scores (for a kernel trace of its own).
Prints and writes one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ggad_amd import _lib  # noqa: E402
from ggad_amd.metrics import top_k  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(xs):
    return dict(median_s=float(statistics.median(xs)), min_s=float(min(xs)), max_s=float(max(xs)), all_s=[float(x) for x in xs])


def make_scores(n, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    scores = torch.sigmoid(10.0 * torch.randn(n, generator=g, device=dev)).float().contiguous()
    labels = (torch.rand(n, generator=g, device=dev) < 0.0042).to(torch.uint8)
    return scores, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scores", type=int, default=1_736_598)
    ap.add_argument("--all", type=int, default=3_700_550)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--profile-k", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("topk_wide_time.py needs an MI355X")
    dev = "cuda:0"
    lib = _lib.load()
    narrow_cap, wide_cap = int(lib.ggad_topk_max_k()), int(lib.ggad_topk_wide_max_k())

    def buffers(entry, n, k):
        return (torch.empty(k, dtype=torch.int32, device=dev), torch.empty(k, dtype=torch.float32, device=dev),
                torch.empty(k, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int64, device=dev),
                torch.empty(int(getattr(lib, entry + "_workspace_elems")(n, k)), dtype=torch.int32, device=dev))

    def native(entry, scores, labels, k, b):
        _lib.call(entry + "_f32", _lib.ptr(scores), _lib.ptr(labels), scores.numel(), k, _lib.ptr(b[0]), _lib.ptr(b[1]), _lib.ptr(b[2]),
                  _lib.ptr(b[3]), _lib.ptr(b[4]))
        return b

    def torch_sort(scores, labels, k):
        v, i = torch.sort(scores, descending=True, stable=True)
        i = i[:k]
        return i, v[:k], torch.cumsum(labels[i].to(torch.int32), 0)

    if a.profile_k:
        scores, labels = make_scores(a.scores, dev, 72)
        b = buffers("ggad_topk_wide", a.scores, a.profile_k)
        for _ in range(a.warmup + a.reps):
            timed(lambda: native("ggad_topk_wide", scores, labels, a.profile_k, b))
        print(json.dumps(dict(profiled_k=a.profile_k, calls=a.warmup + a.reps, scores=a.scores)))
        return

    line = dict(what="top-k above 16,384 ranks: seconds, a device synchronise around every part, medians after warm-up, the routes "
                     "alternating; scores = sigmoid(10 N(0,1)) float32 from a fixed seed",
                device=torch.cuda.get_device_name(0), narrow_max_k=narrow_cap, wide_max_k=wide_cap, warmup=a.warmup, reps=a.reps, by_case=[])
    plan = [(a.scores, 72, k) for k in (1000, 8192, narrow_cap, 65536, 1 << 20, a.scores)] + [(a.all, 73, wide_cap)]
    held = {}
    for n, seed, k in plan:
        if k > wide_cap or n < 1:
            continue
        if n not in held:
            held.clear()
            torch.cuda.empty_cache()
            held[n] = make_scores(n, dev, seed)
        scores, labels = held[n]
        bw = buffers("ggad_topk_wide", n, k)
        routes = dict(wide=lambda: native("ggad_topk_wide", scores, labels, k, bw), top_k=lambda: top_k(scores, k, labels, wide=True),
                      torch_sort=lambda: torch_sort(scores, labels, k))
        if k <= narrow_cap:
            bn = buffers("ggad_topk", n, k)
            routes["narrow"] = lambda: native("ggad_topk", scores, labels, k, bn)
        for fn in routes.values():
            for _ in range(a.warmup):
                timed(fn)
        ts = {name: [] for name in routes}
        for _ in range(a.reps):                                    # alternating
            for name, fn in routes.items():
                ts[name].append(timed(fn)[0])
        native("ggad_topk_wide", scores, labels, k, bw)
        isrt, vs, cs = torch_sort(scores, labels, k)
        m = min(n, k)
        entry = dict(scores=n, k=k, m=m, positives=int(labels.sum()), saturated=int((scores == 1.0).sum()),
                     workspace_bytes=4 * int(bw[4].numel()), **{name: summary(v) for name, v in ts.items()})
        entry.update(meta=[int(v) for v in bw[3].tolist()], positions_equal_torch_sort=bool(torch.equal(bw[0][:m].long(), isrt)),
                     scores_equal_torch_sort=bool(torch.equal(bw[1][:m], vs)),
                     cum_pos_equal_torch_sort=bool(torch.equal(bw[2][:m], cs.to(torch.int32))))
        if k <= narrow_cap:
            native("ggad_topk", scores, labels, k, bn)
            entry["outputs_equal_narrow"] = all(bool(torch.equal(x, z)) for x, z in zip(bw[:4], bn[:4]))
        line["by_case"].append(entry)
        print(json.dumps(entry), flush=True)
        del bw, isrt, vs, cs
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
