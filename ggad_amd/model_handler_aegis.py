"""`ModelHandler` of the mini-batch AEGIS-style comparison model -- drop-in for `src/model_handler_aegis.py`.

    ModelHandler(config).train() -> None          (prints per-epoch loss_g / loss_gen / time and the validation AP / AUC)

Same config keys as the GGAD handler (`src/dgraph.yml`), the reference's split (15 % of the real anomalies contaminate the training list,
5 % of the labelled normals are relabelled, `:29-56`), its batch schedule (per epoch the concatenation idx_train + idx_test, shuffled
with python's `random`, the first 100 slices of `batch_size`, `:131-147`), both losses back-propagated before one Adam step
(`:156-158`), validation with `test_aegis` every `valid_epochs` (`:167-169`).  Where the work runs differs: one plan per epoch for its
100 batch sub-graphs and their two 1-hop aggregates (feature table and noise table: the GGAD plan / gather kernels), then per batch
the projections and the discriminator's linears on the MFMA GEMM and the flat Adam kernel.

Parity of this model is unpinned (see `ggad_amd/graphsage_aegis.py`: `torch_geometric.nn.MLP` is restated, not imported).
Extra, optional config keys: ``device``, ``num_batches`` (default = the reference's hard override 100), ``data`` = (adj_lists |
DeviceGraph | (rowptr, col), feat_data, labels).  Results: ``self.epoch_losses`` [(loss_g, loss_gen) per batch], ``self.epoch_times``,
``self.valid_history`` [(epoch, auc, ap)].

The epoch loop is `model_handler_dominate.ModelHandler.train`; this file holds what AEGIS does differently in it.  Config key
`aegis_device: true` (aegis_device.py): per batch one forward and one backward launch of `csrc/aegis_mb.hip` and the flat Adam kernel,
one fold of the batch norm's running buffers per epoch; from epoch 1 on the `num_batches` steps of an epoch are ONE hipGraph (config
key `capture: false` turns it off).  The default path is never captured.  Same schedule, same `random` stream on either path.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import graphsage_aegis as _model
from .graphsage import FeatureTable
from .handler_loop import device_graph
from .model_handler_dominate import ModelHandler as _Base
from .sage_utils import test_aegis


class ModelHandler(_Base):
    model_module = _model
    pseudo_frac = 0.05                  # src/model_handler_aegis.py:43
    default_num_batches = 100           # :136

    def build_model(self, dev):
        args = self.args
        feat_data = self.dataset["feat_data"]
        n, f = feat_data.shape
        nn.Embedding(n, f)                  # the reference's frozen table draws N x F normals before the model is built (:105)
        graph = device_graph(self.dataset["adj_lists"], n, dev)
        m = self.model_module
        features = FeatureTable(torch.FloatTensor(np.asarray(feat_data, dtype=np.float32)))
        agg_gcn = m.GCNAggregator(features, feat_data, cuda=True)                                    # :110 (draws the noise table)
        dev_path = True if bool(getattr(args, "aegis_device", False)) else None
        enc_gcn = m.GCNEncoder(features, f, args.emb_size, graph, agg_gcn, gcn=True, cuda=True, aegis_device=dev_path)     # :111-112
        return graph, features, m.GCN(2, enc_gcn).to(dev)

    def node_pool(self):
        return np.concatenate([np.asarray(self.dataset[k], dtype=np.int64) for k in ("idx_train", "idx_test")]), "idx_train + idx_test"

    def epoch_order(self, pool, rng):
        sampled = pool.copy()                                                # :132 a fresh concatenation every epoch
        rng.shuffle(sampled)                                                 # :133
        return sampled

    def begin(self, st, n_pool):
        st.losses = torch.empty(st.num_batches, 2, dtype=torch.float32, device=st.dev)
        st.ad = st.enc.aegis_device
        if st.ad is not None:
            st.ad.reserve(min(st.bs, n_pool), st.num_batches)
        return bool(getattr(self.args, "capture", True)) and st.ad is not None

    def plan(self, st, batches):
        x_feat, x_noise, bp = st.enc.aggregator.aggregate(batches, st.graph, st.num_batches)      # all batch sub-graphs, both tables
        return (x_feat, x_noise), bp

    def run_batches(self, st, x_feat, x_noise, bp):
        for b in range(st.num_batches):
            st.optimizer.zero_grad()
            if st.ad is not None:
                st.ad.step(x_feat[bp[b]:bp[b + 1]], x_noise[bp[b]:bp[b + 1]], out=st.losses[b], slot=b, fold=False)
                st.optimizer.step()
                continue
            loss_g, loss_gen = st.model.loss_rows(x_feat[bp[b]:bp[b + 1]], x_noise[bp[b]:bp[b + 1]])
            (loss_g + loss_gen).backward()                                   # :156-157: two backward passes into the same .grad
            st.optimizer.step()
            st.losses[b, 0], st.losses[b, 1] = loss_g.detach(), loss_gen.detach()
        if st.ad is not None:
            st.ad.fold(st.num_batches, 0)

    def report(self, epoch, l, num_batches, epoch_time):
        print(f"Epoch: {epoch}, loss_g: {l[:, 0].sum() / num_batches}, loss_gen: {l[:, 1].sum() / num_batches}, time: {epoch_time}s")

    def validate(self, st, idx_valid, y_valid):
        return test_aegis(idx_valid, y_valid, st.model, st.bs, self.args.thres)
