"""`ModelHandler` of the mini-batch DOMINANT-style comparison model -- drop-in for `src/model_handler_dominate.py`.

    ModelHandler(config).train() -> None          (prints per-epoch loss / time and the validation AUROC / AP)

Same config keys as the GGAD handler (`src/dgraph.yml`), the reference's split (15 % of the real anomalies contaminate the
training list, 10 % of the labelled normals are relabelled, `:29-56`), its batch schedule (one in-place `random.shuffle` of
the whole training list per epoch, the first 150 slices of `batch_size`, `:134-151`), Adam with weight decay.  Where the work
runs differs: one plan of the epoch's 150 batch sub-graphs + 1-hop aggregates (the GGAD plan / gather kernels), then per batch
two MFMA projections, the reconstruction kernel and the flat Adam kernel; validation scores a thousand slices per plan.

Extra, optional config keys: ``device``, ``num_batches`` (default = the reference's hard override), ``recon_device``
(default false; true = the epoch's optimiser steps in one fused launch and the validation score in another), ``data`` =
(adj_lists | DeviceGraph | (rowptr, col), feat_data, labels).  Results: ``self.epoch_losses``, ``self.epoch_times``,
``self.valid_history`` [(epoch, auc, ap)].

`train` below is the one epoch loop of the DOMINANT, AnomalyDAE and AEGIS handlers: schedule the epoch's node order, plan its batch
sub-graphs, run the batches -- eagerly in epoch 0, from epoch 1 on as ONE hipGraph (`fullgraph_script.CapturedEpoch`) replayed on the
plan buffers of the new epoch --, read the losses back, print, validate.  What differs between the models is in the small methods
behind it, which `model_handler_aegis.py` overrides.
"""
from __future__ import annotations

import argparse
import random
import time
import types

import numpy as np
import torch
import torch.nn as nn

from . import graphsage_dominant as _model
from .fullgraph import FlatAdam
from .fullgraph_script import CapturedEpoch
from .graphsage import FeatureTable
from .handler_loop import device_graph, load_and_split
from .sage_utils import test_recon
from .sampler import PyCompatRandom


class ModelHandler(object):
    model_module = _model
    pseudo_frac = 0.10                  # src/model_handler_dominate.py:43
    default_num_batches = 150           # :140

    def __init__(self, config):
        self.args, self.dataset = load_and_split(argparse.Namespace(**config), real_frac=0.15, pseudo_frac=self.pseudo_frac)

    def build_model(self, dev):
        args = self.args
        feat_data = self.dataset["feat_data"]
        n, f = feat_data.shape
        nn.Embedding(n, f)                  # the reference's frozen table draws N x F normals before the model is built (:109)
        graph = device_graph(self.dataset["adj_lists"], n, dev)
        m = self.model_module
        features = FeatureTable(torch.FloatTensor(np.asarray(feat_data, dtype=np.float32)))
        agg_gcn = m.GCNAggregator(features, cuda=True)
        dev_path = True if bool(getattr(args, "recon_device", False)) else None
        enc_gcn = m.GCNEncoder(features, f, args.emb_size, graph, agg_gcn, gcn=True, cuda=True, recon_device=dev_path)
        return graph, features, m.GCN(2, enc_gcn)

    # ---- what `train` asks of a model; `st` carries model, enc, optimizer, graph, attr (the feature table), dev, num_batches, bs
    def node_pool(self):
        """(the nodes an epoch's batches are sliced from, what the "do not fit" error calls them)."""
        return np.asarray(self.dataset["idx_train"], dtype=np.int64).copy(), "the training list"

    def epoch_order(self, pool, rng):
        rng.shuffle(pool)                                                    # :136, in place: epochs compound
        return pool

    def begin(self, st, n_pool):
        """Buffers that live as long as the loop (a captured epoch holds their addresses); returns whether epochs are captured."""
        st.target = torch.empty(min(st.num_batches * st.bs, n_pool), st.attr.shape[1], dtype=torch.float32, device=st.dev)
        st.losses = torch.empty(st.num_batches, dtype=torch.float32, device=st.dev)
        # config key `recon_device: true` (recon_device.py): the optimiser steps of an epoch are ONE launch of `csrc/recon_mb.hip` on
        # the FlatAdam's own state; nothing is captured and `capture` is ignored
        st.rd = st.enc.recon_device
        if st.rd is not None:
            st.rd.bind(st.enc, st.optimizer)
        return bool(getattr(self.args, "capture", True)) and st.rd is None

    def plan(self, st, batches):
        """Aggregate the epoch's batches in one plan; returns (the tensors the batches read -- a plan buffer that moves is captured
        again --, the batch offsets)."""
        x1, bp = st.enc.aggregator.aggregate(batches, st.graph, st.num_batches)       # all 150 batch sub-graphs in one plan
        nodes_dev = torch.from_numpy(np.concatenate(batches)).to(st.dev)
        torch.index_select(st.attr, 0, nodes_dev, out=st.target)                     # torch.tensor(feat_data)[batch_nodes]  :155
        return (x1,), bp

    def run_batches(self, st, x1, bp):
        if st.rd is not None:
            st.rd.steps(x1, st.target, bp[:st.num_batches + 1], *st.model.recon_weights, losses=st.losses)
            return
        for b in range(st.num_batches):
            st.optimizer.zero_grad()
            loss = st.model.loss_rows(x1[bp[b]:bp[b + 1]], st.target[bp[b]:bp[b + 1]])
            loss.backward()
            st.optimizer.step()
            st.losses[b] = loss.detach()

    def report(self, epoch, l, num_batches, epoch_time):
        # the reference prints (last batch loss * 2) / num_batches (`loss += loss.item()` on the tensor, :162-164)
        print(f"Epoch: {epoch}, loss: {2.0 * l[-1] / num_batches},  time: {epoch_time}s")

    def validate(self, st, idx_valid, y_valid):
        return test_recon(idx_valid, y_valid, st.model, st.bs, st.attr, self.args.thres)

    # ---- the loop
    def train(self):
        args = self.args
        if not torch.cuda.is_available():
            raise RuntimeError("ModelHandler.train needs an MI355X: there is no CPU fallback")
        dev = torch.device("cuda", int(getattr(args, "device", torch.cuda.current_device())))
        torch.cuda.set_device(dev)
        graph, features, gnn_model = self.build_model(dev)
        self.model = gnn_model
        optimizer = FlatAdam([p for p in gnn_model.parameters() if p.requires_grad], lr=args.lr, weight_decay=args.weight_decay)
        pool, pool_name = self.node_pool()
        idx_valid, y_valid = self.dataset["idx_valid"], self.dataset["y_valid"]
        num_batches = int(getattr(args, "num_batches", self.default_num_batches))
        bs = int(args.batch_size)
        if (num_batches - 1) * bs >= len(pool):
            raise ValueError(f"{num_batches} batches of {bs} do not fit {pool_name} ({len(pool)} nodes)")
        rng = PyCompatRandom.from_python_state(random.getstate())
        self.epoch_losses, self.epoch_times, self.valid_history = [], [], []
        st = types.SimpleNamespace(model=gnn_model, enc=gnn_model.enc, optimizer=optimizer, graph=graph, attr=features.weight.data,
                                   dev=dev, num_batches=num_batches, bs=bs)
        # epoch 0 runs eagerly (it also creates the Adam state and sizes every buffer); after it the optimiser steps of an epoch are
        # ONE hipGraph, replayed on the plan buffers of the new epoch (fixed addresses, fixed batch boundaries)
        cap = CapturedEpoch(lambda: self.run_batches(st, *st.plan), enabled=self.begin(st, len(pool)), at=1,
                            before_capture=optimizer.zero_grad)
        for epoch in range(args.num_epochs):
            order = self.epoch_order(pool, rng)
            t0 = time.time()
            batches = [order[b * bs:min((b + 1) * bs, len(order))] for b in range(num_batches)]
            tensors, bp = self.plan(st, batches)
            st.plan = (*tensors, bp)
            cap.step(epoch, key=tuple(t.data_ptr() for t in tensors))
            torch.cuda.synchronize()
            epoch_time = time.time() - t0
            l = st.losses.cpu().numpy().astype(np.float64)
            self.epoch_losses.append(l)
            self.epoch_times.append(epoch_time)
            self.report(epoch, l, num_batches, epoch_time)
            if epoch % args.valid_epochs == 0:
                print("Valid at epoch {}".format(epoch))
                auc, ap = self.validate(st, idx_valid, y_valid)
                self.valid_history.append((epoch, auc, ap))
        random.setstate(rng.to_python_state())
        return None
