"""A validation sweep that stays on the device between validations (config key `eval_cache`).

`sage_utils.score_nodes` plans every slice of `batch_size` ids again on every sweep, although an inference plan is 1-hop only
and its output -- the aggregated row `x1[i]` of every id -- depends on the graph, the frozen feature table, the id list and the
slice boundaries (the aggregation normalises per slice, quirk 2), never on the weights.  The score is
`sigmoid(w . relu(W x1[i]))`, row by row (`k_score`, csrc/step.hip: one wave per row, a fixed fma order, nothing that depends on
the launch size).  `ResidentSweep` therefore builds the plans ONCE, keeps the `(n, F)` rows, and a sweep is one `ggad_mb_score`
launch over them: bit for bit what `score_nodes` returns.  The metrics come from the counting kernels of csrc/rank_metrics.hip
(`metrics.rank_report`) instead of two device sorts; above their 8,192 positives, with config key `rank_wide`, from those of
csrc/rank_metrics.hip (`metrics.rank_report_wide`).
"""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np
import torch

from ._lib import call, ptr
from .minibatch import BatchChunk


class ResidentSweep:
    """The aggregated inference rows of `test_cases`, cached on the device, and the uint8 labels beside them (`labels=None`: an
    unlabelled id list, which `top_k` ranks and `report` refuses).

    The cache depends on: the graph (`model.enc.adj_lists`), the feature table (`model.enc.features.weight`), the ids of
    `test_cases` in their order, `batch_size` (the slice boundaries) -- and on nothing else; the weights enter in `scores()` only.
    A caller that changes the feature table or the graph calls `invalidate()`; the rows are then rebuilt by the next `scores()`.
    The ids are copied at construction: a list mutated in place afterwards is NOT detected (build a new sweep for a new list)."""

    def __init__(self, model, test_cases: Sequence[int], labels, batch_size: int, batches_per_launch: int = 2048,
                 rank_wide: bool = False):
        self.model = model
        self.rank_wide = bool(rank_wide)                         # config key `rank_wide`: see report()
        self.n_pos = None                                        # with rank_wide: the label-1 entries, counted once on the host
        self.engine = model.enc.engine
        self.cases = np.array(test_cases, dtype=np.int64).reshape(-1)
        self.n = int(len(self.cases))
        self.labels = None                                       # `labels=None`: an unlabelled id list (top_k only; report() raises)
        if labels is not None:
            lab = np.asarray(labels).reshape(-1)
            if len(lab) != self.n:
                raise ValueError("ResidentSweep: labels / test_cases length mismatch")
            self.labels = torch.from_numpy(lab.astype(np.uint8)).to(self.engine.dev)      # uploaded once
            if self.rank_wide:
                self.n_pos = int(np.count_nonzero(lab == 1))                              # (the labels never change)
        self.ids = torch.from_numpy(self.cases).to(self.engine.dev)                       # for top_k, uploaded once
        self.batch_size = int(batch_size)
        self.batches_per_launch = int(batches_per_launch)
        self.x1 = None
        self.builds = 0                 # plans built so far (tests: none between two sweeps)
        self._build()

    def _build(self) -> None:
        """Walk the ids exactly as `score_nodes` does (same slices, same `per_launch` bound, same plan) and keep every chunk's x1."""
        enc, eng = self.model.enc, self.engine
        F = eng.F
        self.x1 = torch.empty((self.n, F), dtype=torch.float32, device=eng.dev)
        if self.n == 0:
            return
        from .graphsage import _as_graph
        graph = _as_graph(enc.adj_lists, enc.features.weight.shape[0], eng.dev)
        bs = self.batch_size
        per_launch = int(max(1, min(self.batches_per_launch, (1 << 29) // max(1, graph.n))))
        # local: its two counter arrays are per_launch x N ints each (gigabytes at DGraph size) and nothing needs them afterwards
        ch = BatchChunk(graph, enc.features.weight.data, enc.embed_dim, per_launch, per_launch * bs, per_launch * bs * 8, train=False)
        step = per_launch * bs
        for s in range(0, self.n, step):
            part = self.cases[s:s + step]
            batches = [part[i:i + bs] for i in range(0, len(part), bs)]
            ch.build(batches)
            self.builds += 1
            # device to device, on the stream the build ran on
            self.x1[s:s + len(part)].copy_(ch.x1[:ch.n_rows * F].view(ch.n_rows, F))
        torch.cuda.current_stream(eng.dev).synchronize()          # the chunk's buffers go back to the allocator below
        del ch

    def invalidate(self) -> None:
        """Drop the cached rows; the next `scores()` builds them again.  For callers that change what the cache depends on: the graph
        (`model.enc.adj_lists`) or the feature table (`model.enc.features.weight`).  The weights are not among its inputs.  The ids
        and `batch_size` are fixed at construction: an id list mutated in place afterwards is NOT detected, here or anywhere."""
        self.x1 = None

    def scores(self) -> torch.Tensor:
        """Device float32 `(n,)` probabilities under the engine's CURRENT weights: one `ggad_mb_score` launch over the cache."""
        if self.x1 is None:
            self._build()
        eng = self.engine
        out = torch.empty(self.n, dtype=torch.float32, device=eng.dev)
        eng.sync_params()
        if self.n:
            call("ggad_mb_score", ptr(eng.params), eng.D, eng.F, ptr(self.x1), self.n, ptr(out))
        return out

    def report(self, thres: float, scores: torch.Tensor = None) -> Dict[str, float]:
        """The dict of `metrics.binary_report` for the current weights, from `metrics.rank_report` (the faster of the two metric blocks
        at 1.74 M scores: profiles/eval_cache_time_line.json).  `scores`: a result of `scores()` the caller already holds.
        A sweep built with `rank_wide=True` whose list holds more positives than `ggad_rank_metrics_max_pos()` reports through
        `metrics.rank_report_wide` with `pos_cap` = its count of positives, where `rank_report` would fall back to `binary_report`;
        a list at or under the cap takes `rank_report` either way."""
        from .metrics import rank_report, rank_report_wide
        if self.labels is None:
            raise ValueError("ResidentSweep.report: this sweep was built without labels (an id list to rank: use top_k)")
        scores = self.scores() if scores is None else scores
        if self.rank_wide and self.n_pos > int(self.engine.lib.ggad_rank_metrics_max_pos()):
            return rank_report_wide(scores, self.labels, thres, pos_cap=min(self.n_pos, int(self.engine.lib.ggad_rank_wide_max_pos())))
        return rank_report(scores, self.labels, thres)

    def operating_point(self, criterion: str, param: float = None, thres: float = 0.5, scores: torch.Tensor = None):
        """`metrics.operating_point` of the current weights' scores (or of `scores`, a result of `scores()` the caller already
        holds) on the resident labels: the alert threshold that is best under `criterion`, with its counts.  `pos_cap` is the
        sweep's own count of positives (counted once on the host), so the workspace and the grids are as small as they can be."""
        from .metrics import operating_point
        if self.labels is None:
            raise ValueError("ResidentSweep.operating_point: this sweep was built without labels")
        if self.n_pos is None:
            self.n_pos = int((self.labels == 1).sum())
        cap = int(self.engine.lib.ggad_rank_wide_max_pos())
        if self.n_pos > cap:
            raise ValueError(f"ResidentSweep.operating_point: the list holds {self.n_pos} positives, more than "
                             f"ggad_rank_wide_max_pos() = {cap}")
        return operating_point(self.scores() if scores is None else scores, self.labels, criterion, param, thres,
                               pos_cap=max(1, self.n_pos))

    def _own_pos_cap(self, who: str) -> int:
        """The sweep's own count of positives as the `pos_cap` of a run-merge call (counted once), as `operating_point` takes it."""
        if self.labels is None:
            raise ValueError(f"ResidentSweep.{who}: this sweep was built without labels")
        if self.n_pos is None:
            self.n_pos = int((self.labels == 1).sum())
        cap = int(self.engine.lib.ggad_rank_wide_max_pos())
        if self.n_pos > cap:
            raise ValueError(f"ResidentSweep.{who}: the list holds {self.n_pos} positives, more than ggad_rank_wide_max_pos() = {cap}")
        return max(1, self.n_pos)

    def auc_ci(self, level: float = 0.95, scores: torch.Tensor = None):
        """`metrics.auc_ci` of the current weights' scores (or of `scores`, a result of `scores()` the caller already holds) on the
        resident labels: the AUROC with DeLong's standard error and the normal interval at `level`."""
        from .metrics import auc_ci
        cap = self._own_pos_cap("auc_ci")
        return auc_ci(self.scores() if scores is None else scores, self.labels, level, pos_cap=cap)

    def ap_ci(self, level: float = 0.95, reps: int = 1000, seed: int = 0, scores: torch.Tensor = None):
        """`metrics.ap_ci` of the current weights' scores (or of `scores`, a result of `scores()` the caller already holds) on the
        resident labels: average precision and AUROC with the percentile intervals of `reps` stratified bootstrap replicates."""
        from .metrics import ap_ci
        cap = self._own_pos_cap("ap_ci")
        return ap_ci(self.scores() if scores is None else scores, self.labels, level, reps, seed, pos_cap=cap)

    def compare(self, scores_b: torch.Tensor, scores: torch.Tensor = None):
        """`metrics.compare_auc` of the current weights' scores (or of `scores`) against `scores_b`, another model's scores of the
        same list, on the resident labels: DeLong's paired test of the two AUROCs."""
        from .metrics import compare_auc
        cap = self._own_pos_cap("compare")
        return compare_auc(self.scores() if scores is None else scores, scores_b, self.labels, pos_cap=cap)

    def compare_ap(self, scores_b: torch.Tensor, scores: torch.Tensor = None, level: float = 0.95, reps: int = 1000, seed: int = 0):
        """`metrics.compare_ap` of the current weights' scores (or of `scores`) against `scores_b`, another model's scores of the
        same list, on the resident labels: the paired stratified bootstrap of the two average precisions."""
        from .metrics import compare_ap
        cap = self._own_pos_cap("compare_ap")
        return compare_ap(self.scores() if scores is None else scores, scores_b, self.labels, level, reps, seed, pos_cap=cap)

    def top_k(self, k: int, scores: torch.Tensor = None, wide: bool = False):
        """`metrics.top_k` of the current weights' scores (or of `scores`, a result of `scores()` the caller already holds) with the
        sweep's ids and resident labels: the `Ranked` head of the list, `ids` = node ids.  Nothing is uploaded and no plan is built.
        `wide`: `metrics.top_k(..., wide=True)`, k above 16,384 up to a full ranking of the list."""
        from .metrics import top_k
        return top_k(self.scores() if scores is None else scores, k, self.labels, self.ids, wide=wide)

    def explain(self, ranked_or_positions, m: int):
        """`explain.explain` of positions of this sweep (a `Ranked` of `top_k`, or a device tensor of positions) with the sweep's ids and
        `batch_size` under the current weights: the `Explanation`, `m` neighbours listed per row.  Nothing is uploaded and no plan is
        built; the kernel reads the graph and the feature table, not the cached rows."""
        from .explain import explain
        return explain(self.model, self.ids, self.batch_size, ranked_or_positions, m)
