#!/usr/bin/env python3
"""Median replayed epoch of one TAM truncation round (`tam_utils.train_cut`) and of the affinity head alone, composed against fused
(`--fused_head`), at Reddit and Amazon size (synthetic graphs of `SIZES`, embedding_dim 128).

    python scripts/tam_time.py [--epochs 400] [--sizes reddit,Amazon] [--out profiles/tam_time_line.json]

Per size, in one process, on the same truncated graph and the same initial weights for both paths: the epoch of `train_cut` (forward,
loss, the composed path's second affinity pass, backward, Adam) after two eager epochs and the capture, `--epochs` replays each
bracketed by device events; then the head alone (forward + backward on a fixed embedding: `max_message` + `inference` + backward
against `max_message_fused` + backward), captured and replayed the same way.  The two paths alternate in blocks (composed, fused,
composed, fused) so that a drift of the device clock shows in both; the medians are over all blocks of a path.
Prints and writes one JSON line."""
import argparse
import copy
import json
import os
import random
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ggad_amd import tam_utils as T  # noqa: E402
from ggad_amd.fullgraph import FlatAdam, FullGraphAdj  # noqa: E402
from ggad_amd.fullgraph_script import capture, synthetic_graph  # noqa: E402
from ggad_amd.model_tam import Model  # noqa: E402
from ggad_amd.utils import preprocess_features  # noqa: E402


def setup(dataset, dev, h, seed=0):
    """tam.py's setup up to the first truncation round: (adj, feats, initial state_dict, normal_label_idx, ft_size)."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    adj, feat, ano = synthetic_graph(dataset, seed)
    n = adj.shape[0]
    normal, _ = T.split_nodes(ano)
    features = np.asarray(preprocess_features(feat)) if dataset == "Amazon" else np.asarray(feat.todense())
    raw = (adj + sp.eye(n)).tocsr()
    raw.sort_indices()
    feats = torch.FloatTensor(np.asarray(features, dtype=np.float32)[np.newaxis]).to(dev)
    dis = T.calc_distance(raw, feats[0])
    cut = T.graph_nsgt(raw, dis, raw.copy())
    full = FullGraphAdj(T.normalize_adj_tensor(cut), raw, dev)
    model = Model(features.shape[1], h, "prelu", 2, "avg").to(dev)
    return full, feats, copy.deepcopy(model.state_dict()), normal, features.shape[1], raw


def warm_capture(fn, warm=2):
    for _ in range(warm):
        fn()
    return capture(fn)[0]


def replay_ms(graph, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(ts):
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), n=len(ts))


def time_size(dataset, epochs, h):
    dev = torch.device("cuda", 0)
    full, feats, init, normal, ft, raw = setup(dataset, dev, h)
    idx = torch.as_tensor(np.asarray(normal, dtype=np.int64), device=dev)
    head = T.TamHead(full, normal)
    graphs = {}
    keep = []
    # the two paths on the same embedding at this size, before anything is timed: loss, message, gradient
    m0 = Model(ft, h, "prelu", 2, "avg").to(dev)
    m0.load_state_dict(init)
    e0 = m0.forward(feats, full)[0][0].detach()
    ec, ef = e0.clone().requires_grad_(True), e0.clone().requires_grad_(True)
    lc, _ = T.max_message(ec, full, idx)
    mc = T.inference(ec.detach(), full)
    lc.backward()
    lf, _, mf = T.max_message_fused(ef, full, idx, head=head, want_m=False)
    lf.backward()
    check = dict(loss_composed=float(lc), loss_fused=float(lf), message_max_abs_diff=float((mc - mf).abs().max()),
                 message_max_abs=float(mc.abs().max()), grad_max_abs_diff=float((ec.grad - ef.grad).abs().max()),
                 grad_max_abs=float(ec.grad.abs().max()))
    for fused in (False, True):
        model = Model(ft, h, "prelu", 2, "avg").to(dev)
        model.load_state_dict(init)
        model.train()
        opt = FlatAdam(model.parameters(), lr=1e-5, weight_decay=0.0)
        opt.zero_grad()

        def epoch(model=model, opt=opt, fused=fused):                    # the epoch of train_cut
            node_emb, _, _ = model.forward(feats, full)
            if fused:
                loss, _, msg = T.max_message_fused(node_emb[0], full, idx, head=head, want_m=False)
            else:
                loss, _ = T.max_message(node_emb[0], full, idx)
                with torch.no_grad():
                    msg = T.inference(node_emb[0].detach(), full)
            loss.backward()
            opt.step()
            return msg

        emb = model.forward(feats, full)[0][0].detach().clone().requires_grad_(True)

        def head_only(emb=emb, fused=fused):                             # what the epoch spends behind the second GCN layer
            emb.grad = None
            if fused:
                loss, _, msg = T.max_message_fused(emb, full, idx, head=head, want_m=False)
            else:
                loss, _ = T.max_message(emb, full, idx)
                with torch.no_grad():
                    msg = T.inference(emb.detach(), full)
            loss.backward()
            return msg

        tag = "fused" if fused else "composed"
        graphs[("epoch", tag)] = warm_capture(epoch)
        graphs[("head", tag)] = warm_capture(head_only)
        keep.append((model, opt, emb))
    times = {k: [] for k in graphs}
    blocks = 2
    for _ in range(blocks):
        for k, gr in graphs.items():
            replay_ms(gr, 3)                                             # back to a steady state after the other graph
            times[k] += replay_ms(gr, max(1, epochs // blocks))
    res = dict(n=int(full.n), nnz_raw=int(raw.nnz), h=h, hubs=head.n_hub, hub_pieces=head.n_pieces, k_normal=int(head.k_total),
               check=check)
    for (what, tag), ts in times.items():
        res[f"{what}_{tag}"] = stats(ts)
    for what in ("epoch", "head"):
        res[f"{what}_fused_over_composed"] = res[f"{what}_fused"]["median_ms"] / res[f"{what}_composed"]["median_ms"]
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--epochs", type=int, default=400)
    p.add_argument("--sizes", type=str, default="reddit,Amazon")
    p.add_argument("--h", type=int, default=128)
    p.add_argument("--out", type=str, default=None)
    a = p.parse_args()
    torch.cuda.set_device(0)
    line = dict(what="TAM: replayed epoch of a train_cut round and the affinity head alone (forward + backward), composed path against "
                     "--fused_head, device events, synthetic graphs of the published sizes, same graph and weights for both paths",
                device=torch.cuda.get_device_name(0), sizes={})
    for ds in a.sizes.split(","):
        t0 = time.time()
        line["sizes"][ds] = time_size(ds, a.epochs, a.h)
        print(ds, line["sizes"][ds], "({:.0f} s)".format(time.time() - t0), flush=True)
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
