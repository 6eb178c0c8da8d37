#!/usr/bin/env python3
"""What the device-resident generator (ggad_amd/rng.py, csrc/rng.hip) costs and what it buys.

    python scripts/noise_time.py [--epochs 200] [--repeats 2] [--shapes 238x300,...] [--runs run:reddit,run:photo,gaan:reddit,...]
                                 [--out profiles/device_noise_time_line.json]

1. The kernel alone: `DeviceMT.randn_` (both launches: the serial word generator and the wide Box-Muller pass) at the draw sizes of
   the scripts -- 238 x 300 and 844 x 300 (run.py on Reddit and Photo: labelled anomalies x embedding_dim), 10,984 x 16, 39,357 x 16 and
   46,564 x 16 (gaan.py / aegis.py: N x 16).  Device events around 20 back-to-back calls, 15 rounds; median and minimum per call.
2. The median wall time per epoch that each script itself reports ("median epoch ... ms": host clock around an epoch that ends in a
   device synchronise, draw included), with and without `--device_noise`, the two alternating in one process.  Without the flag the
   scripts run exactly the code of the commit before the flag existed (host draw, copy, replay; run.py with its look-ahead).

Prints and writes one JSON line."""
import argparse
import contextlib
import io
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aegis  # noqa: E402
import gaan  # noqa: E402
import run  # noqa: E402
from ggad_amd.rng import DeviceMT  # noqa: E402

KERNEL_SHAPES = ((238, 300), (844, 300), (10984, 16), (39357, 16), (46564, 16))
SCRIPTS = {"run": run, "gaan": gaan, "aegis": aegis}


def time_kernel(rows, cols, calls=20, rounds=15):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    mt = DeviceMT.from_host(dev)
    buf = torch.zeros(rows, cols, device=dev)
    for _ in range(3):
        mt.randn_(buf, 0.01, 0.02)
    torch.cuda.synchronize()
    per_call = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            mt.randn_(buf, 0.01, 0.02)
        b.record()
        b.synchronize()
        per_call.append(a.elapsed_time(b) * 1e3 / calls)
    t0 = time.perf_counter()
    for _ in range(rounds):
        torch.randn(rows, cols)
    host = (time.perf_counter() - t0) / rounds * 1e6
    n = rows * cols
    return dict(n=n, words=n + (16 if n % 16 else 0), median_us=float(np.median(per_call)), min_us=float(np.min(per_call)),
                host_torch_randn_us=float(host))


def script_median_ms(name, dataset, epochs, device_noise):
    argv = [name + ".py", "--dataset", dataset, "--synthetic", "--quiet", "--num_epoch", str(epochs)]
    if name == "aegis" and dataset not in aegis.LR:
        argv += ["--lr", "1e-3"]
    if device_noise:
        argv.append("--device_noise")
    out = io.StringIO()
    old = sys.argv
    sys.argv = argv
    try:
        with contextlib.redirect_stdout(out):
            SCRIPTS[name].main()
    finally:
        sys.argv = old
    m = re.search(r"median epoch ([0-9.]+) ms", out.getvalue())
    if m is None or ("captured" not in out.getvalue() and name != "run"):
        raise RuntimeError("no median / no capture in the output of " + " ".join(argv))
    return float(m.group(1))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--epochs", type=int, default=200)
    p.add_argument("--repeats", type=int, default=2)
    p.add_argument("--runs", type=str, default="run:reddit,run:photo,gaan:reddit,gaan:photo,gaan:elliptic,aegis:reddit")
    p.add_argument("--shapes", type=str, default=",".join("{}x{}".format(r, c) for r, c in KERNEL_SHAPES), help="kernel part: ROWSxCOLS,...")
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit("noise_time.py needs an MI355X")
    torch.cuda.set_device(0)
    line = dict(what="device-resident MT19937 normal draw: (kernel) DeviceMT.randn_ per call, device events around 20 calls, 15 rounds; "
                     "(epochs) the script's own 'median epoch' wall time, draw included, synthetic graphs of the published sizes; "
                     "host = without --device_noise, which is the code path of the commit before the flag, unchanged",
                device=torch.cuda.get_device_name(0), epochs_per_run=a.epochs, kernel={}, epochs={})
    for rows, cols in [tuple(int(v) for v in sh.split("x")) for sh in a.shapes.split(",") if sh]:
        line["kernel"]["{}x{}".format(rows, cols)] = time_kernel(rows, cols)
        print(rows, cols, line["kernel"]["{}x{}".format(rows, cols)], flush=True)
    for item in [r for r in a.runs.split(",") if r]:
        name, dataset = item.split(":")
        host, device = [], []
        for _ in range(a.repeats):                      # alternating, one process
            host.append(script_median_ms(name, dataset, a.epochs, False))
            device.append(script_median_ms(name, dataset, a.epochs, True))
        line["epochs"]["{}.py {}".format(name, dataset)] = dict(host_median_ms=host, device_median_ms=device)
        print(item, line["epochs"]["{}.py {}".format(name, dataset)], flush=True)
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
