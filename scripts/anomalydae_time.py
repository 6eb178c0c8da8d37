#!/usr/bin/env python3
"""Epoch time of the full-graph AnomalyDAE model (anomalyDAE.py) at the five published sizes (synthetic graphs of run.py's SIZES).

    python scripts/anomalydae_time.py [--sizes reddit,photo,...] [--steps 20] [--warmup 5] [--cpu] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o adae -- python scripts/anomalydae_time.py --profile-epochs 3
    python scripts/rocpd_stats.py DIR/adae_results.db STATS.csv
    python scripts/anomalydae_time.py --shares STATS.csv --line TIMING_LINE.json --profile-epochs 3

Timing mode prints one JSON line: per size the median device time of one replayed hipGraph epoch (2 eager epochs, the capture,
`--warmup` replays, then `--steps` replays timed one by one with device events), the test scoring on idx_test (the forward
kernels over |T| rows, done on every 5th epoch), and the shape-derived floor of the structure loss.  `--cpu` adds the same
epoch on the CPU in torch float32 on 16 threads, in the reference's dense formulation (s_ = sigmoid(z z^T) materialised, the GAT
on an edge list built once) at the Reddit and Amazon sizes.

Profile mode runs `--profile-epochs` eager epochs (each with the test scoring) per size (to be run under `rocprofv3 --kernel-trace --stats`); `--shares` reads
the resulting kernel_stats CSV and prints, per structure-loss kernel, its time per call and its share of the bound computed from
the shapes: exact-f32 MFMA at 157.3 TFLOP/s, or the issue floor of one v_exp_f32 + one v_rcp_f32 (8 cycles each per wave of 64
lanes on one SIMD: 256 CUs x 4 SIMDs x 64 lanes / 16 cycles x 2.4 GHz = 153.6 G sigmoids/ms), whichever is larger.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_F32 = 157.3e12            # FLOP/s, MI355X_MICROARCH.md
SIGMOID_RATE = 256 * 4 * 64 / 16 * 2.4e9      # sigmoids/s at the v_exp_f32 + v_rcp_f32 issue floor


def _args(dataset):
    return types.SimpleNamespace(dataset=dataset, synthetic=True, seed=0, quiet=True, lr=None, weight_decay=0.0, embedding_dim=300,
                                 negsamp_ratio=1, readout="avg")


def _setup(dataset, dev):
    import anomalyDAE
    a = _args(dataset)
    a.lr = anomalyDAE.LR[dataset]
    torch.manual_seed(0)
    return anomalyDAE.setup(a, dev)


def shapes(n, F, n_r, n_t):
    """Floors of the structure-loss kernels from the shapes: (flops, sigmoids) per call."""
    k4, k16 = (F + 3) // 4 * 4, (F + 15) // 16 * 16
    return {"adae_stru_fwd_dense": (2 * n_r * n * k4, n_r * n),
            "adae_stru_bwd_dense_rows": (2 * n_r * n * (k4 + k16), n_r * n),
            "adae_stru_bwd_dense_cols": (2 * n_r * n * (k4 + k16), n_r * n),
            "adae_score_test": (2 * n_t * n * k4, n_t * n)}


def floor_s(flops, sig):
    return max(flops / MFMA_F32, sig / SIGMOID_RATE)


def time_gpu(dataset, steps, warmup, dev):
    import anomalyDAE
    from ggad_amd.fullgraph_script import capture
    from ggad_amd.model_anomalydae import recon_score
    full, feats, model, opt, ano, idx_test, normal_idx = _setup(dataset, dev)
    ep = anomalyDAE.make_epoch(model, opt, feats, full, normal_idx)
    for _ in range(2):
        ep()
    g, static = capture(ep)
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    sc = []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        recon_score(static[1], static[2], feats[0], full, idx_test)
        e1.record()
        e1.synchronize()
        if i >= warmup:
            sc.append(e0.elapsed_time(e1))
    n, F = full.n, feats.shape[-1]
    sh = shapes(n, F, len(normal_idx), len(idx_test))
    train_floor = sum(floor_s(*sh[k]) for k in ("adae_stru_fwd_dense", "adae_stru_bwd_dense_rows", "adae_stru_bwd_dense_cols"))
    assert np.isfinite(static[0].item())
    return {"n": n, "f": int(F), "n_train_rows": int(len(normal_idx)), "n_test_rows": int(len(idx_test)),
            "epoch_ms_median": float(np.median(ts)), "epoch_ms_min": float(np.min(ts)), "nodes_per_s": n / (np.median(ts) * 1e-3),
            "test_scoring_ms_median": float(np.median(sc)), "stru_loss_floor_ms_per_epoch": train_floor * 1e3,
            "test_scoring_floor_ms": floor_s(*sh["adae_score_test"]) * 1e3}


def time_cpu(dataset, steps=3):
    """One reference-formulation epoch on the CPU (float32, 16 threads): dense s_, GAT on an edge list built once."""
    import scipy.sparse as sp
    from ggad_amd.utils import normalize_adj, preprocess_features
    from run import load
    torch.set_num_threads(16)
    a = _args(dataset)
    adj, features, ano, idx_test, normal_idx, _ = load(a)
    x = torch.from_numpy(np.asarray(preprocess_features(features), dtype=np.float32))
    n, F = x.shape
    A = (normalize_adj(adj) + sp.eye(n)).tocsr()
    A_dense = torch.from_numpy(np.asarray(A.todense(), dtype=np.float32))
    coo = A.tocoo()
    keep = (coo.row != coo.col) & (coo.data > 0)
    src = torch.from_numpy(np.concatenate([coo.row[keep], np.arange(n)]).astype(np.int64))
    dst = torch.from_numpy(np.concatenate([coo.col[keep], np.arange(n)]).astype(np.int64))
    torch.manual_seed(0)
    H = 300
    W_s, W_g, W_1, W_2 = (torch.nn.Linear(i, o) for i, o in ((F, H), (H, F), (F, H), (H, F)))
    a_s, a_d = torch.nn.Parameter(torch.randn(F) * 0.1), torch.nn.Parameter(torch.randn(F) * 0.1)
    params = [p for m in (W_s, W_g, W_1, W_2) for p in m.parameters()] + [a_s, a_d]
    opt = torch.optim.Adam(params, lr=1e-3)
    R, T = torch.as_tensor(normal_idx), torch.as_tensor(idx_test)

    def epoch():
        opt.zero_grad()
        y = torch.relu(W_s(x)) @ W_g.weight.T
        e = torch.nn.functional.leaky_relu((y @ a_s)[src] + (y @ a_d)[dst], 0.2)
        m = torch.full((n,), -float("inf")).scatter_reduce(0, dst, e.detach(), "amax")
        ex = (e - m[dst]).exp()
        p = ex / (torch.zeros(n).index_add(0, dst, ex)[dst] + 1e-16)
        z = torch.zeros(n, F).index_add(0, dst, p[:, None] * y[src]) + W_g.bias
        s_ = torch.sigmoid(z @ z.T)
        xh = W_2(torch.relu(W_1(x)))
        score = 0.5 * torch.sqrt(((x[R] - xh[R]) ** 2).sum(1)) + 0.5 * torch.sqrt(((A_dense[R] - s_[R]) ** 2).sum(1))
        loss = score.mean()
        with torch.no_grad():
            0.5 * torch.sqrt(((x[T] - xh[T]) ** 2).sum(1)) + 0.5 * torch.sqrt(((A_dense[T] - s_[T]) ** 2).sum(1))
        loss.backward()
        opt.step()

    epoch()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        epoch()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"n": n, "f": int(F), "threads": 16, "epoch_ms_median": float(np.median(ts)), "epochs_timed": steps, "warmup": 1}


def shares(csv_path, line_path, epochs):
    """Share of bound of the structure-loss kernels from the kernel stats (scripts/rocpd_stats.py CSV: kernel, calls, total_us)
    of a `--profile-epochs` run over the sizes of a timing line (whose shapes it reads)."""
    tot = {}
    for ln in open(csv_path).read().splitlines()[1:]:
        name, calls, total_us = ln.rsplit(",", 6)[:3]       # (kernel names may hold commas)
        tot[name] = (int(calls), float(total_us) * 1e3)
    line = json.load(open(line_path))
    flops = {"k_stru_fwd_dense": 0, "k_stru_bwd_dense": 0}
    sig = dict(flops)
    for d, v in line["gpu"].items():    # per profiled epoch: the training forward + the test scoring, and the two recompute passes
        for k, (fl, sg) in shapes(v["n"], v["f"], v["n_train_rows"], v["n_test_rows"]).items():
            key = "k_stru_bwd_dense" if "bwd" in k else "k_stru_fwd_dense"
            flops[key] += fl * epochs
            sig[key] += sg * epochs
    out = {}
    for key in flops:
        hit = [(n, c, t) for n, (c, t) in tot.items() if key in n]
        if not hit:
            continue
        calls, ns = sum(h[1] for h in hit), sum(h[2] for h in hit)
        bound = max(flops[key] / MFMA_F32, sig[key] / SIGMOID_RATE)
        out[key] = {"calls": calls, "total_ms": ns * 1e-6, "floor_ms": bound * 1e3, "share_of_bound": bound / (ns * 1e-9),
                    "bound": "f32 MFMA" if flops[key] / MFMA_F32 >= sig[key] / SIGMOID_RATE else "exp/rcp issue",
                    "achieved_tflops": flops[key] / (ns * 1e-9) / 1e12}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="reddit,photo,Amazon,t_finance,elliptic")
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--cpu", action="store_true")
    p.add_argument("--out")
    p.add_argument("--profile-epochs", type=int, default=0)
    p.add_argument("--shares", help="kernel stats CSV of a --profile-epochs run (scripts/rocpd_stats.py output)")
    p.add_argument("--line", help="timing line whose shapes the --shares computation uses")
    a = p.parse_args()
    sizes = a.sizes.split(",")
    res = {"workload": "anomalyDAE full-graph epoch (synthetic graphs of run.py SIZES, embedding 300)",
           "warmup": "2 eager epochs, capture, {} replays".format(a.warmup), "steps": a.steps}
    if a.shares:
        res = {"shares": shares(a.shares, a.line, a.profile_epochs)}
    elif a.profile_epochs:
        import anomalyDAE
        dev = torch.device("cuda", 0)
        for d in sizes:                                  # eager epochs: one forward + backward each, plus the test scoring
            from ggad_amd.model_anomalydae import recon_score
            full, feats, model, opt, ano, idx_test, normal_idx = _setup(d, dev)
            ep = anomalyDAE.make_epoch(model, opt, feats, full, normal_idx)
            for _ in range(a.profile_epochs):
                _, z, xh = ep()
                recon_score(z, xh, feats[0], full, idx_test)
            torch.cuda.synchronize()
        res = {"profiled_epochs_per_size": a.profile_epochs, "sizes": sizes}
    else:
        if not torch.cuda.is_available():
            sys.exit("the timing needs an MI355X")
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        res["gpu"] = {d: time_gpu(d, a.steps, a.warmup, dev) for d in sizes}
        if a.cpu:
            res["cpu_float32_dense"] = {d: time_cpu(d) for d in ("reddit", "Amazon")}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
