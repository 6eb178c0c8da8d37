"""Dense steps of a chunk on the wide launch chain (csrc/step_wide.hip), alone on the chip, DGraph-size synthetic graph, batches of
150 + 50 rows -- measured as scripts/xcd_step_time.py measures the launch chain: `train_chunk` of a built chunk between two
synchronisations, five repetitions, median, divided by the number of batches.

Rows: chain 2 at D = 64 (the layered D <= 64 kernels: the yardstick), chain 3 at D = 64 (the wide kernels at one channel slot),
the wide chain at D = 128 and D = 256.  Each row also holds the time of `ggad_mb_project` and of `ggad_mb_bwd_flat` alone (device
events around one launch per batch of the chunk, back to back) and their share of the step.

Usage (GPU box): python scripts/wide_step_time.py [batches]      -> profiles/wide_step_time_line.json"""
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from ggad_amd import synth  # noqa: E402
from ggad_amd._lib import call, ptr  # noqa: E402
from ggad_amd.dgraph import normalize_features, split_dgraphfin  # noqa: E402
from ggad_amd.graph import DeviceGraph  # noqa: E402
from ggad_amd.minibatch import MiniBatchEngine  # noqa: E402
from ggad_amd.sampler import PyCompatRandom  # noqa: E402
from ggad_amd.trainer import BatchSchedule, DGraphTrainer  # noqa: E402

dev = torch.device('cuda:0')
torch.cuda.set_device(dev)
k = int(sys.argv[1]) if len(sys.argv) > 1 else 20
n, ne = 3_700_550, 73_105_508
rp, ci = synth.make_graph_torch(n, ne, 72, dev, max_degree=2000)
g = DeviceGraph(rp, ci, dev)
feat = torch.from_numpy(normalize_features(synth.make_features(n, 17, 72)).astype(np.float32)).to(dev)
lab = synth.make_labels(n, 15509.0 / 3700550.0, 72).astype(np.int32)
sp = split_dgraphfin(lab, 72, with_test=False)
sched = BatchSchedule(sp['idx_train'], sp['idx_anomaly'], sp['labels'], 150, PyCompatRandom.from_python_state(random.getstate()))
bn, bl = sched.next_batches(k)


def events_us(fn, reps=5):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(1e3 * e0.elapsed_time(e1))
    return sorted(ts)[reps // 2]


rows = []
for name, d, chain in (("chain2_d64", 64, 2), ("chain3_d64", 64, 3), ("wide_d128", 128, 0), ("wide_d256", 256, 0)):
    tr = DGraphTrainer(g, feat, d, sched, chunk_batches=k, overlap=False, prefetch=False, chain=chain, resident=False)
    ch = tr.chunk
    ch.build(bn, bl)
    torch.cuda.synchronize()
    torch.manual_seed(0)
    w0 = (torch.nn.init.xavier_uniform_(torch.empty(1, d)), torch.nn.init.xavier_uniform_(torch.empty(d, 17)),
          torch.nn.init.xavier_uniform_(torch.empty(d, d)))
    eng = MiniBatchEngine(17, d, dev, chain=chain, resident=False)
    ts = []
    for rep in range(5):
        eng.load_params(*w0)
        eng.reset_optimizer()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.train_chunk(ch)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    step_us = 1e6 * sorted(ts)[2] / k
    losses = eng.losses(k)
    assert np.isfinite(losses).all()
    # the two entry-flat kernels alone, through the layered entry points -- which dispatch on D, so at D = 64 they reach the D <= 64
    # kernels only: the chain-3 row has no such pair (None)
    proj_us = bwd_us = None
    if chain != 3:
        def project():
            for b in range(k):
                e0, e1 = ch.batch_ents(b)
                call("ggad_mb_project", ptr(eng.params), d, 17, ptr(ch.x2), ptr(ch.ent_own), e0, e1 - e0, ptr(eng.h2))

        def bwd_flat():
            for b in range(k):
                r0, r1 = ch.batch_rows(b)
                e0, e1 = ch.batch_ents(b)
                call("ggad_mb_bwd_flat", d, 17, ptr(ch.x1), ptr(ch.x2), ptr(eng.h2), ptr(ch.ent_own), ptr(ch.ent_row), r0, r1 - r0, e0,
                     e1 - e0, ptr(ch.coef_a), ptr(ch.coef_g), ptr(eng.dw_part))
        proj_us, bwd_us = events_us(project) / k, events_us(bwd_flat) / k
    row = dict(name=name, D=d, chain=chain, batches=k, entries_per_batch=ch.n_ents / k, step_us_median=step_us,
               step_us_best=1e6 * min(ts) / k, project_us=proj_us, bwd_flat_us=bwd_us,
               project_share=None if proj_us is None else proj_us / step_us,
               bwd_flat_share=None if bwd_us is None else bwd_us / step_us, first_loss=float(losses[0, 0]))
    rows.append(row)
    print(json.dumps(row), flush=True)
    del tr, ch, eng
    torch.cuda.empty_cache()

out = dict(what="dense steps of a chunk on the launch chain, us per optimiser step (median of 5 train_chunk calls / batches), DGraph-size "
                "synthetic graph, 150 + 50 rows; project / bwd_flat: the layered entry point alone, one launch per batch back to back "
                "(device events)", device=torch.cuda.get_device_name(dev), rows=rows)
os.makedirs("profiles", exist_ok=True)
with open(os.path.join("profiles", "wide_step_time_line.json"), "w") as fh:
    json.dump(out, fh)
    fh.write("\n")
print("wrote profiles/wide_step_time_line.json")
