"""Binary classification metrics on the device: AUROC, average precision, F1 (class 1 / class 0 /
macro), confusion matrix and G-mean of `test_sage` (`src/utils.py:232-247`) and of `run.py:236-239`, computed from
scores that never leave HBM: one device sort + prefix sums in fp64 instead of a 1.7 M-element copy to the host and
sklearn.  Definitions follow scikit-learn's (the reference's metric library), including its handling of tied scores:

  roc_auc_score            trapezoids over the DISTINCT thresholds of the ROC curve
  average_precision_score  sum_n (R_n - R_{n-1}) P_n over the distinct thresholds, descending
  f1_score / confusion     from the thresholded predictions (score >= thres)

sklearn itself stays the checker in the tests (tests/test_metrics.py).

`rank_report` returns the same dict from float32 scores and uint8 labels through the counting kernels of csrc/rank_metrics.hip:
no full sort (only the positives are sorted), four launches and ONE read-back.  `rank_report_wide` is the same for more than the
8,192 positives one workgroup sorts, up to 1,048,576, through the run-merge chain of the same file.

`top_k` is the ranked list: the k highest scores in a FIXED order (score descending, equal scores by ascending position; the head
of a saturated sigmoid ranking is full of exact ties, and `torch.topk` fixes neither which tied elements it returns nor their
order), with the running count of positives beside it, from `ggad_topk_f32` (csrc/topk.hip): six launches and ONE read-back.
`top_k(..., wide=True)` is the same list for more than the 16,384 ranks one workgroup sorts, up to 4,194,304, through
`ggad_topk_wide_f32` of the same file.

`operating_point` turns a score into an alert rule: the threshold, among the distinct scores of the positives, that is best under
F1, macro-F1, G-mean, or recall at a bound on precision or on the false-positive rate, with its exact confusion counts, from
`ggad_rank_operating_f32` (the run-merge chain of csrc/rank_metrics.hip with an arg-max behind it): one call, one read-back.
`pr_curve` is the curve behind it; `parse_criterion` reads the criterion's spelling in the configs and on the command lines.

`auc_ci` says how far an AUROC can be trusted -- DeLong's variance, standard error and normal interval -- and `compare_auc` whether two
models' AUROCs on the same labels differ (DeLong's paired z and p), from `ggad_rank_delong_f32` / `ggad_rank_delong_pair_f32`: the
same chain with the variance's numerators as exact 128-bit integers, one call and one read-back each.

`ap_ci` does the same for average precision, which has no closed-form variance: the percentile interval, standard error and bias of a
stratified bootstrap whose replicates `ggad_rank_bootstrap_f32` makes from the chain's sorted positives and two histograms alone, one
workgroup per replicate; the AUROC's bootstrap interval comes with it.  `compare_ap` says whether two models' average precisions on the
same labels differ: a PAIRED bootstrap (`ggad_rank_bootstrap_pair_f32`), whose replicates draw elements and count each at its own bin
under either model -- the interval, standard error and two-sided p-value of the difference."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch


def _curve_counts(scores: torch.Tensor, labels: torch.Tensor):
    """tps / fps at the last element of every run of equal scores, scores descending (sklearn `_binary_clf_curve`)."""
    s, order = torch.sort(scores.double(), descending=True, stable=True)
    y = labels[order].double()
    n = s.numel()
    last = torch.ones(n, dtype=torch.bool, device=s.device)
    if n > 1:
        last[:-1] = s[:-1] != s[1:]
    tps = torch.cumsum(y, 0)[last]
    fps = torch.cumsum(1.0 - y, 0)[last]
    return tps, fps


def roc_auc(scores: torch.Tensor, labels: torch.Tensor) -> float:
    tps, fps = _curve_counts(scores, labels)
    if tps.numel() == 0 or tps[-1] == 0 or fps[-1] == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    zero = torch.zeros(1, dtype=torch.float64, device=tps.device)
    tpr = torch.cat([zero, tps / tps[-1]])
    fpr = torch.cat([zero, fps / fps[-1]])
    return float(torch.trapezoid(tpr, fpr))


def average_precision(scores: torch.Tensor, labels: torch.Tensor) -> float:
    tps, fps = _curve_counts(scores, labels)
    if tps.numel() == 0 or tps[-1] == 0:
        return 0.0
    precision = tps / (tps + fps)
    recall = tps / tps[-1]
    prev = torch.cat([torch.zeros(1, dtype=torch.float64, device=tps.device), recall[:-1]])
    return float(((recall - prev) * precision).sum())


def _confusion_scores(tp: int, fp: int, fn: int, tn: int) -> Dict[str, float]:
    """F1 of class 1 and of class 0, macro-F1 and G-mean of a confusion matrix, and its four counts."""
    def f1(t, f_p, f_n):
        d = 2 * t + f_p + f_n
        return 2.0 * t / d if d else 0.0

    f1_1, f1_0 = f1(tp, fp, fn), f1(tn, fn, fp)
    gmean = float((tp * tn / ((tp + fn) * (tn + fp))) ** 0.5) if (tp + fn) and (tn + fp) else float("nan")
    return {"f1_1": f1_1, "f1_0": f1_0, "f1_macro": 0.5 * (f1_1 + f1_0), "gmean": gmean, "tp": tp, "fp": fp, "fn": fn, "tn": tn}


def binary_report(scores: torch.Tensor, labels: torch.Tensor, thres: float) -> Dict[str, float]:
    """Everything `test_sage` prints and returns, one host read-back of a handful of scalars."""
    labels = labels.to(scores.device)
    pred = scores >= thres                                     # prob2pred, src/utils.py:250-260
    pos = labels == 1
    tp = int((pred & pos).sum())
    fp = int((pred & ~pos).sum())
    fn = int((~pred & pos).sum())
    tn = int((~pred & ~pos).sum())
    return {"auc": roc_auc(scores, labels), "ap": average_precision(scores, labels), **_confusion_scores(tp, fp, fn, tn)}


_ONE_CLASS = "Only one class present in y_true. ROC AUC score is not defined in that case."


def _rank_call(scores: torch.Tensor, labels_u8: torch.Tensor, thres: float, pos_cap: Optional[int], wide: bool) -> Dict[str, float]:
    """The body of `rank_report` and `rank_report_wide`: the checks, the workspace, one call and one read-back of eight doubles."""
    from . import _lib
    if scores.dtype != torch.float32 or labels_u8.dtype != torch.uint8 or scores.dim() != 1 or scores.shape != labels_u8.shape:
        raise ValueError("rank_report takes float32 scores and uint8 labels of the same 1-D shape")
    if scores.device.type != "cuda" or labels_u8.device != scores.device:
        raise ValueError("rank_report takes scores and labels on the same GPU (there is no CPU path: use binary_report)")
    lib = _lib.load()
    n = scores.numel()
    if wide:
        cap = int(lib.ggad_rank_wide_max_pos())
        if pos_cap is None:
            pos_cap = max(1, min(n, cap))
        if int(pos_cap) != pos_cap or not 1 <= int(pos_cap) <= cap:
            raise ValueError(f"rank_report_wide: pos_cap = {pos_cap} is outside 1..ggad_rank_wide_max_pos() = {cap}")
        entry, sized = "ggad_rank_wide", (n, int(pos_cap))
    else:
        entry, sized = "ggad_rank_metrics", (n,)
    scores, labels_u8 = scores.contiguous(), labels_u8.contiguous()
    with torch.cuda.device(scores.device):
        ws = torch.empty(max(1, int(getattr(lib, entry + "_workspace_elems")(*sized))), dtype=torch.int32, device=scores.device)
        out8 = torch.empty(8, dtype=torch.float64, device=scores.device)
        _lib.call(entry + "_f32", _lib.ptr(scores), _lib.ptr(labels_u8), *sized, float(thres), _lib.ptr(out8), _lib.ptr(ws))
        return _report_from_out8(out8.cpu().tolist(), lambda: binary_report(scores, labels_u8, thres))


def rank_report(scores: torch.Tensor, labels_u8: torch.Tensor, thres: float) -> Dict[str, float]:
    """`binary_report` (same keys) for float32 device scores and uint8 device labels from `ggad_rank_metrics_f32`: AUROC as one
    float64 division of exact integer counts, AP as a fixed-order float64 sum, the confusion counts as integers; one read-back of
    eight doubles.  One class only: the `ValueError` of `binary_report`.  More positives than `ggad_rank_metrics_max_pos()`: the
    result of `binary_report` (its two device sorts).  A NaN score or a label other than 0/1: `ValueError`."""
    return _rank_call(scores, labels_u8, thres, None, False)


def rank_report_wide(scores: torch.Tensor, labels_u8: torch.Tensor, thres: float, pos_cap: Optional[int] = None) -> Dict[str, float]:
    """`rank_report` for up to `ggad_rank_wide_max_pos()` = 1,048,576 positives, from `ggad_rank_wide_f32` (csrc/rank_metrics.hip: the
    positives sorted in runs of 2,048 and merged, the same formulas): same arguments, same checks, same dict, one read-back.
    `pos_cap`: the caller's upper bound on the positives, which sizes the workspace and the launches (`None`: min(n, the cap); a
    tight bound means fewer merge passes and less workspace).  More positives than `pos_cap`: the result of `binary_report`.
    Timings against `binary_report` and `rank_report`: profiles/rank_wide_time_line.json."""
    return _rank_call(scores, labels_u8, thres, pos_cap, True)


def _report_from_out8(o, fallback) -> Dict[str, float]:
    """The `binary_report` dict from the eight numbers of `ggad_rank_metrics_f32` (host values); `fallback()` serves status 2."""
    status = int(o[7])
    if status == 3:
        raise ValueError("rank_report: a score is NaN")
    if status == 4:
        raise ValueError("rank_report: a label is neither 0 nor 1")
    if status == 2:
        return fallback()
    if status == 1:
        raise ValueError(_ONE_CLASS)
    return {"auc": float(o[0]), "ap": float(o[1]), **_confusion_scores(*(int(v) for v in o[2:6]))}


CRITERIA = ("f1", "f1_macro", "gmean", "precision", "fpr")          # the codes of ggad_rank_operating_f32, in order


def parse_criterion(text) -> Tuple[str, Optional[float]]:
    """(name, param) of `f1`, `f1_macro`, `gmean`, `precision:0.9` (the greatest recall at a precision of at least 0.9) or
    `fpr:0.01` (the greatest recall at a false-positive rate of at most 0.01); anything else: `ValueError`.  The one parser of
    config key `thres_select` and of `run.py --threshold`."""
    name, sep, tail = str(text).strip().partition(":")
    if name not in CRITERIA:
        raise ValueError(f"threshold criterion {text!r}: expected one of f1, f1_macro, gmean, precision:X, fpr:X")
    if name in ("precision", "fpr"):
        try:
            param = float(tail)
        except ValueError:
            raise ValueError(f"threshold criterion {text!r}: `{name}` takes a bound in [0, 1], as in `{name}:0.9`") from None
        if not 0.0 <= param <= 1.0:
            raise ValueError(f"threshold criterion {text!r}: the bound {tail} is outside [0, 1]")
        return name, param
    if sep:
        raise ValueError(f"threshold criterion {text!r}: `{name}` takes no bound")
    return name, None


@dataclass
class OperatingPoint:
    """The alert rule `score >= thres` that `operating_point` chose.  `thres`: a Python float that is exactly a float32 (the score
    of a positive; +inf when `feasible` is false: alert on nothing).  `tp, fp, fn, tn`: its confusion counts; `value`: the
    criterion's value there (F1, macro-F1, G-mean, or the recall under the constraint); `n_candidates`: the distinct positive
    scores; `report`: the `binary_report` dict at `thres`."""
    thres: float
    tp: int
    fp: int
    fn: int
    tn: int
    value: float
    criterion: str
    param: Optional[float]
    n_candidates: int
    feasible: bool
    report: Dict[str, float]


def _criterion_code(criterion, param) -> Tuple[int, float]:
    if criterion not in CRITERIA:
        raise ValueError(f"operating_point: unknown criterion {criterion!r} (one of {', '.join(CRITERIA)})")
    code = CRITERIA.index(criterion)
    if code >= 3:
        if param is None or not 0.0 <= float(param) <= 1.0:
            raise ValueError(f"operating_point: criterion `{criterion}` needs a param in [0, 1], got {param!r}")
        return code, float(param)
    return code, 0.0


def _operating_call(scores, labels_u8, code: int, param: float, thres: float, pos_cap, curve: bool):
    """The checks of `rank_report_wide`, the workspace and ONE `ggad_rank_operating_f32` call: (out16 on the device, the three curve
    tensors or None, pos_cap)."""
    from . import _lib
    if scores.dtype != torch.float32 or labels_u8.dtype != torch.uint8 or scores.dim() != 1 or scores.shape != labels_u8.shape:
        raise ValueError("operating_point takes float32 scores and uint8 labels of the same 1-D shape")
    if scores.device.type != "cuda" or labels_u8.device != scores.device:
        raise ValueError("operating_point takes scores and labels on the same GPU (there is no CPU path)")
    lib = _lib.load()
    n = scores.numel()
    cap = int(lib.ggad_rank_wide_max_pos())
    if pos_cap is None:
        pos_cap = max(1, min(n, cap))
    if int(pos_cap) != pos_cap or not 1 <= int(pos_cap) <= cap:
        raise ValueError(f"operating_point: pos_cap = {pos_cap} is outside 1..ggad_rank_wide_max_pos() = {cap}")
    pos_cap = int(pos_cap)
    scores, labels_u8 = scores.contiguous(), labels_u8.contiguous()
    dev = scores.device
    with torch.cuda.device(dev):
        ws = torch.empty(max(1, int(lib.ggad_rank_operating_workspace_elems(n, pos_cap))), dtype=torch.int32, device=dev)
        out16 = torch.empty(16, dtype=torch.float64, device=dev)
        cur = None
        if curve:
            cur = (torch.empty(pos_cap, dtype=torch.float32, device=dev), torch.empty(pos_cap, dtype=torch.int32, device=dev),
                   torch.empty(pos_cap, dtype=torch.int32, device=dev))
        _lib.call("ggad_rank_operating_f32", _lib.ptr(scores), _lib.ptr(labels_u8), n, pos_cap, float(thres), code, param,
                  _lib.ptr(out16), *((_lib.ptr(c) for c in cur) if cur else (0, 0, 0)), _lib.ptr(ws))
    return out16, cur, pos_cap


def _raise_on_status(who: str, status: int, n_pos: int, pos_cap: int) -> None:
    if status == 3:
        raise ValueError(f"{who}: a score is NaN")
    if status == 4:
        raise ValueError(f"{who}: a label is neither 0 nor 1")
    if status == 2:
        raise ValueError(f"{who}: {n_pos} positives are more than pos_cap = {pos_cap} (there is no fallback: pass a pos_cap that "
                         "bounds them, at most ggad_rank_wide_max_pos())")
    if status == 1:
        raise ValueError(_ONE_CLASS)


def operating_point(scores: torch.Tensor, labels_u8: torch.Tensor, criterion: str = "f1", param: Optional[float] = None,
                    thres: float = 0.5, pos_cap: Optional[int] = None) -> OperatingPoint:
    """The threshold among the distinct scores of the positives that is best under `criterion` (`CRITERIA`; `param`: the bound of
    `precision` and `fpr`), equal values going to the higher threshold, with its exact confusion counts: one
    `ggad_rank_operating_f32` call (csrc/rank_metrics.hip) and one read-back of sixteen doubles.  `thres` and `pos_cap` are
    `rank_report_wide`'s: the call also leaves that report's eight numbers, from which `report` takes AUROC and AP.  `ValueError`
    for an unknown criterion, a missing or out-of-range `param`, a NaN score, a label other than 0/1, one class only, or more
    positives than `pos_cap`.  No candidate meets the constraint: `feasible` is false and `thres` is +inf."""
    code, par = _criterion_code(criterion, param)
    out16, _, pos_cap = _operating_call(scores, labels_u8, code, par, thres, pos_cap, False)
    o = out16.cpu().tolist()
    status = int(o[15])
    _raise_on_status("operating_point", int(o[7]), int(o[6]), pos_cap)
    tp, fp, fn, tn = (int(v) for v in o[9:13])
    return OperatingPoint(thres=float(o[8]), tp=tp, fp=fp, fn=fn, tn=tn, value=float(o[13]), criterion=criterion,
                          param=None if code < 3 else par, n_candidates=int(o[14]), feasible=status == 0,
                          report={"auc": float(o[0]), "ap": float(o[1]), **_confusion_scores(tp, fp, fn, tn)})


def pr_curve(scores: torch.Tensor, labels_u8: torch.Tensor, pos_cap: Optional[int] = None):
    """(thres float32, tp int32, fp int32) on the device, one entry per distinct score of a positive, descending: the confusion
    counts of `score >= thres[i]` (precision tp / (tp + fp), recall tp / tp[-1]).  The kernels store one entry per positive; the
    runs of equal scores are folded here with `torch.unique_consecutive`, which reads back the number of distinct scores."""
    out16, cur, pos_cap = _operating_call(scores, labels_u8, 0, 0.0, 0.5, pos_cap, True)
    o = out16.cpu().tolist()
    _raise_on_status("pr_curve", int(o[7]), int(o[6]), pos_cap)
    p = int(o[6])
    tp, first = torch.unique_consecutive(cur[1][:p], return_inverse=True)      # distinct runs have distinct tp, ascending along j
    head = torch.ones(p, dtype=torch.bool, device=tp.device)
    head[1:] = first[1:] != first[:-1]
    return cur[0][:p][head], tp, cur[2][:p][head]


@dataclass
class AucInterval:
    """AUROC with DeLong's standard error (`auc_ci`).  `var`: the variance of the AUROC, `se` its root; `lo`, `hi`: `auc -+ q se`
    clipped to [0, 1], q the two-sided normal quantile of `level`; `report`: the `binary_report` dict at the call's `thres`."""
    auc: float
    var: float
    se: float
    lo: float
    hi: float
    level: float
    n_pos: int
    n_neg: int
    status_ok: bool
    report: Dict[str, float]


@dataclass
class AucComparison:
    """Two AUROCs on the same labels (`compare_auc`): `diff = auc_a - auc_b`, the two variances, their covariance, the variance of
    the difference, `z = diff / sqrt(var_diff)` and the two-sided p-value of z under a standard normal.  `identical`: the two score
    lists induce the same placements (`var_diff` is exactly 0): `z = 0.0`, `p = 1.0`."""
    auc_a: float
    auc_b: float
    diff: float
    var_a: float
    var_b: float
    cov: float
    var_diff: float
    z: float
    p: float
    n_pos: int
    n_neg: int
    identical: bool


_TOO_FEW = "needs at least two positives and two negatives"


def format_auc_ci(ci: AucInterval) -> str:
    """The one `[auc_ci]` line of `main.py --auc_ci` and `run.py --auc_ci`."""
    return (f"[auc_ci] AUROC {ci.auc!r} ± {ci.se!r} ({ci.level:.0%}: [{ci.lo!r}, {ci.hi!r}]) on {ci.n_pos} positives, "
            f"{ci.n_neg} negatives")


def format_compare(c: AucComparison) -> str:
    """The one `[compare]` line of `--score CKPT --compare CKPT_B`."""
    return f"[compare] AUROC A {c.auc_a!r} B {c.auc_b!r} diff {c.diff!r} z {c.z!r} p {c.p!r}"


def _delong_call(who: str, lists, labels_u8, thres: float, pos_cap):
    """`operating_point`'s checks for every score list of `lists` (one: `ggad_rank_delong_f32`, two: `ggad_rank_delong_pair_f32`),
    the workspace, ONE native call and ONE read-back: (the 16 or 24 doubles as a list, pos_cap)."""
    from . import _lib
    for scores in lists:
        if scores.dtype != torch.float32 or labels_u8.dtype != torch.uint8 or scores.dim() != 1 or scores.shape != labels_u8.shape:
            raise ValueError(f"{who} takes float32 scores and uint8 labels of the same 1-D shape")
        if scores.device.type != "cuda" or labels_u8.device != scores.device:
            raise ValueError(f"{who} takes scores and labels on the same GPU (there is no CPU path)")
    lib = _lib.load()
    n = labels_u8.numel()
    cap = int(lib.ggad_rank_wide_max_pos())
    if pos_cap is None:
        pos_cap = max(1, min(n, cap))
    if int(pos_cap) != pos_cap or not 1 <= int(pos_cap) <= cap:
        raise ValueError(f"{who}: pos_cap = {pos_cap} is outside 1..ggad_rank_wide_max_pos() = {cap}")
    pos_cap = int(pos_cap)
    lists, labels_u8 = [s.contiguous() for s in lists], labels_u8.contiguous()
    dev = labels_u8.device
    entry = "ggad_rank_delong_pair" if len(lists) == 2 else "ggad_rank_delong"
    with torch.cuda.device(dev):
        ws = torch.empty(max(1, int(getattr(lib, entry + "_workspace_elems")(n, pos_cap))), dtype=torch.int32, device=dev)
        out = torch.empty(8 + 8 * len(lists), dtype=torch.float64, device=dev)
        sums = torch.empty(12 * len(lists), dtype=torch.int64, device=dev)
        _lib.call(entry + "_f32", *(_lib.ptr(s) for s in lists), _lib.ptr(labels_u8), n, pos_cap, float(thres), _lib.ptr(out),
                  _lib.ptr(sums), _lib.ptr(ws))
        return out.cpu().tolist(), pos_cap


def auc_ci(scores: torch.Tensor, labels_u8: torch.Tensor, level: float = 0.95, thres: float = 0.5,
           pos_cap: Optional[int] = None) -> AucInterval:
    """AUROC with DeLong's variance and the normal interval at `level`: one `ggad_rank_delong_f32` call (csrc/rank_metrics.hip: the
    run-merge chain, the variance's numerators exact 128-bit integers) and one read-back of sixteen doubles.  `thres` and `pos_cap` are
    `rank_report_wide`'s.  `ValueError` for a `level` outside (0, 1), a NaN score, a label other than 0/1, one class only, more
    positives than `pos_cap`, or fewer than two positives or two negatives."""
    from statistics import NormalDist
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"auc_ci: level = {level!r} is outside (0, 1)")
    o, pos_cap = _delong_call("auc_ci", [scores], labels_u8, thres, pos_cap)
    _raise_on_status("auc_ci", int(o[7]), int(o[6]), pos_cap)
    tp, fp, fn, tn = (int(v) for v in o[2:6])
    if int(o[15]) == 6:
        raise ValueError(f"auc_ci: {tp + fn} positives and {fp + tn} negatives: DeLong's variance {_TOO_FEW}")
    auc, var, se = float(o[0]), float(o[8]), float(o[11])
    q = NormalDist().inv_cdf(0.5 + float(level) / 2)
    return AucInterval(auc=auc, var=var, se=se, lo=max(0.0, auc - q * se), hi=min(1.0, auc + q * se), level=float(level),
                       n_pos=tp + fn, n_neg=fp + tn, status_ok=int(o[15]) == 0,
                       report={"auc": auc, "ap": float(o[1]), **_confusion_scores(tp, fp, fn, tn)})


def compare_auc(scores_a: torch.Tensor, scores_b: torch.Tensor, labels_u8: torch.Tensor, pos_cap: Optional[int] = None) -> AucComparison:
    """DeLong's paired test of two score lists on the same labels: one `ggad_rank_delong_pair_f32` call and one read-back of
    twenty-four doubles.  The variance of the difference comes from exact integer numerators of its own, not from
    `var_a + var_b - 2 cov`.  The `ValueError`s of `auc_ci`, for either list."""
    import math
    o, pos_cap = _delong_call("compare_auc", [scores_a, scores_b], labels_u8, 0.5, pos_cap)
    _raise_on_status("compare_auc", int(o[23]) if int(o[23]) in (1, 2, 3, 4) else 0, int(o[6]), pos_cap)
    n_pos, n_neg = int(o[2]) + int(o[4]), int(o[3]) + int(o[5])
    if int(o[23]) == 6:
        raise ValueError(f"compare_auc: {n_pos} positives and {n_neg} negatives: DeLong's variance {_TOO_FEW}")
    same = int(o[23]) == 7
    z = 0.0 if same else float(o[21])
    return AucComparison(auc_a=float(o[0]), auc_b=float(o[8]), diff=float(o[20]), var_a=float(o[16]), var_b=float(o[17]),
                         cov=float(o[18]), var_diff=float(o[19]), z=z, p=1.0 if same else math.erfc(abs(z) / 2 ** 0.5),
                         n_pos=n_pos, n_neg=n_neg, identical=same)


@dataclass(eq=False)
class BootstrapInterval:
    """Average precision and AUROC with stratified-bootstrap percentile intervals (`ap_ci`).  `ap`, `auc`: the point estimates of the
    list; `*_lo`, `*_hi`: the `(1 - level) / 2` and `(1 + level) / 2` quantiles of the replicates (numpy's linear method); `*_se`:
    their standard deviation (`ddof=1`; NaN for one replicate); `ap_bias`: the replicates' mean minus `ap`.  `ap_reps` float64 and
    `auc_reps` float64 hold the `reps` replicates in replicate order; `report`: the `binary_report` dict at the call's `thres`."""
    ap: float
    ap_lo: float
    ap_hi: float
    ap_se: float
    ap_bias: float
    auc: float
    auc_lo: float
    auc_hi: float
    auc_se: float
    level: float
    reps: int
    seed: int
    n_pos: int
    n_neg: int
    report: Dict[str, float]
    ap_reps: "numpy.ndarray"
    auc_reps: "numpy.ndarray"

    def __eq__(self, other):
        if not isinstance(other, BootstrapInterval):
            return NotImplemented
        mine, theirs = dict(self.__dict__), dict(other.__dict__)
        return all(mine.pop(k).tobytes() == theirs.pop(k).tobytes() for k in ("ap_reps", "auc_reps")) and repr(mine) == repr(theirs)


def format_ap_ci(ci: BootstrapInterval) -> str:
    """The one `[ap_ci]` line of `main.py --ap_ci` and `run.py --ap_ci`."""
    return (f"[ap_ci] AP {ci.ap!r} ± {ci.ap_se!r} ({ci.level:.0%}: [{ci.ap_lo!r}, {ci.ap_hi!r}], bias {ci.ap_bias!r}) "
            f"AUROC {ci.auc!r} ({ci.level:.0%}: [{ci.auc_lo!r}, {ci.auc_hi!r}]) from {ci.reps} stratified replicates, seed {ci.seed}, "
            f"on {ci.n_pos} positives, {ci.n_neg} negatives")


def _bootstrap_call(who: str, lists, labels_u8, level, reps, seed, thres: float, pos_cap):
    """The argument checks of `ap_ci` / `compare_ap` for every score list of `lists` (one: `ggad_rank_bootstrap_f32`, two:
    `ggad_rank_bootstrap_pair_f32`), the workspace, ONE native call, ONE read-back and the `ValueError` of every status: (the 16 or
    24 doubles as a list, the replicate words behind them -- every list's `rep_ap`, then every list's `rep_auc_num` as int64 words
    -- as a float64 array, reps, seed)."""
    from . import _lib
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f"{who}: level = {level!r} is outside (0, 1)")
    for scores in lists:
        if scores.dtype != torch.float32 or labels_u8.dtype != torch.uint8 or scores.dim() != 1 or scores.shape != labels_u8.shape:
            raise ValueError(f"{who} takes float32 scores and uint8 labels of the same 1-D shape")
        if scores.device.type != "cuda" or labels_u8.device != scores.device:
            raise ValueError(f"{who} takes scores and labels on the same GPU (there is no CPU path)")
    lib = _lib.load()
    max_reps, boot_cap, cap = int(lib.ggad_rank_bootstrap_max_reps()), int(lib.ggad_rank_bootstrap_max_pos()), int(lib.ggad_rank_wide_max_pos())
    if int(reps) != reps or not 1 <= int(reps) <= max_reps:
        raise ValueError(f"{who}: reps = {reps!r} is outside 1..ggad_rank_bootstrap_max_reps() = {max_reps}")
    if int(seed) != seed or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"{who}: seed = {seed!r} is not an unsigned 64-bit integer")
    reps, seed, n = int(reps), int(seed), labels_u8.numel()
    if pos_cap is None:
        pos_cap = max(1, min(n, boot_cap))
    if int(pos_cap) != pos_cap or not 1 <= int(pos_cap) <= cap:
        raise ValueError(f"{who}: pos_cap = {pos_cap} is outside 1..ggad_rank_wide_max_pos() = {cap}")
    pos_cap = int(pos_cap)
    too_many = ("{} positives are more than ggad_rank_bootstrap_max_pos() = {}: a replicate's histograms no longer fit one "
                "workgroup's LDS, and there is no fallback")
    lists, labels_u8 = [s.contiguous() for s in lists], labels_u8.contiguous()
    dev = labels_u8.device
    entry = "ggad_rank_bootstrap_pair" if len(lists) == 2 else "ggad_rank_bootstrap"
    head, per = 8 + 8 * len(lists), reps * len(lists)
    with torch.cuda.device(dev):
        ws = torch.empty(max(1, int(getattr(lib, entry + "_workspace_elems")(n, pos_cap))), dtype=torch.int32, device=dev)
        out = torch.empty(head + 2 * per, dtype=torch.float64, device=dev)         # the head, rep_ap, rep_auc_num (int64 words)
        base = _lib.ptr(out)
        _lib.call(entry + "_f32", *(_lib.ptr(s) for s in lists), _lib.ptr(labels_u8), n, pos_cap, float(thres), seed, reps, base,
                  base + head * 8, base + (head + per) * 8, 0, _lib.ptr(ws))
        host = out.cpu().numpy()
    o = host[:head].tolist()
    status, n_pos = int(o[head - 1]), int(o[6])
    if status == 2 and pos_cap >= boot_cap:
        raise ValueError(f"{who}: " + too_many.format(n_pos, boot_cap))
    _raise_on_status(who, status if status in (1, 2, 3, 4) else 0, n_pos, pos_cap)
    if status == 9:
        raise ValueError(f"{who}: " + too_many.format(n_pos, boot_cap))
    if status == 8:
        raise ValueError(f"{who}: {int(o[2]) + int(o[4])} positives and {int(o[3]) + int(o[5])} negatives: a stratified bootstrap {_TOO_FEW}")
    if status != 0:
        raise ValueError(f"{who}: {entry}_f32 left status {status}")
    return o, host[head:], reps, seed


def ap_ci(scores: torch.Tensor, labels_u8: torch.Tensor, level: float = 0.95, reps: int = 1000, seed: int = 0, thres: float = 0.5,
          pos_cap: Optional[int] = None) -> BootstrapInterval:
    """Average precision (and AUROC) with the percentile interval of a stratified bootstrap at `level`: one `ggad_rank_bootstrap_f32`
    call (csrc/rank_metrics.hip: the run-merge chain, then one workgroup per replicate that redraws the positives' ranks and the
    negatives' bins with Philox4x32-10 under `seed` and never touches the elements again) and one read-back of `16 + 2 reps` words.
    Stratified: every replicate holds the list's own counts of positives and negatives.  `thres` and `pos_cap` are
    `rank_report_wide`'s (default `pos_cap`: the bootstrap's cap).  `ValueError` for a `level` outside (0, 1), `reps` outside
    1..ggad_rank_bootstrap_max_reps(), a seed outside 64 bits, a NaN score, a label other than 0/1, one class only, fewer than two
    positives or two negatives, more positives than `pos_cap` or than ggad_rank_bootstrap_max_pos() (an error: there is no second route)."""
    import numpy as np
    o, words, reps, seed = _bootstrap_call("ap_ci", [scores], labels_u8, level, reps, seed, thres, pos_cap)
    tp, fp, fn, tn = (int(v) for v in o[2:6])
    ap_reps = words[:reps].copy()
    auc_reps = words[reps:].view(np.int64).astype(np.float64) / float(2 * (tp + fn) * (fp + tn))
    q = [(1.0 - float(level)) / 2, (1.0 + float(level)) / 2]
    ap_lo, ap_hi = (float(v) for v in np.quantile(ap_reps, q))
    auc_lo, auc_hi = (float(v) for v in np.quantile(auc_reps, q))
    nan = float("nan")
    ap, auc = float(o[1]), float(o[0])
    return BootstrapInterval(ap=ap, ap_lo=ap_lo, ap_hi=ap_hi, ap_se=float(ap_reps.std(ddof=1)) if reps > 1 else nan,
                             ap_bias=float(ap_reps.mean() - ap), auc=auc, auc_lo=auc_lo, auc_hi=auc_hi,
                             auc_se=float(auc_reps.std(ddof=1)) if reps > 1 else nan, level=float(level), reps=reps, seed=seed,
                             n_pos=tp + fn, n_neg=fp + tn, report={"auc": auc, "ap": ap, **_confusion_scores(tp, fp, fn, tn)},
                             ap_reps=ap_reps, auc_reps=auc_reps)


@dataclass(eq=False)
class ApComparison:
    """Two models' average precision (and AUROC) on the same labels from a paired stratified bootstrap (`compare_ap`).  `ap_a`,
    `ap_b`, `diff = ap_a - ap_b`: the point estimates; `diff_lo`, `diff_hi`: the `(1 - level) / 2` and `(1 + level) / 2` quantiles of
    the replicate differences (numpy's linear method); `diff_se`: their standard deviation (`ddof=1`; NaN for one replicate); `p`: the
    two-sided bootstrap p-value min(1, 2 min((1 + #{d* <= 0}) / (B + 1), (1 + #{d* >= 0}) / (B + 1))); the `auc_*` fields alike for
    the AUROC.  `identical`: every replicate difference, AP and AUROC numerator, is exactly 0 (then `p = 1.0`).  `diff_reps` and
    `auc_diff_reps` float64 hold the `reps` replicate differences in replicate order."""
    ap_a: float
    ap_b: float
    diff: float
    diff_lo: float
    diff_hi: float
    diff_se: float
    p: float
    auc_a: float
    auc_b: float
    auc_diff: float
    auc_diff_lo: float
    auc_diff_hi: float
    auc_diff_se: float
    level: float
    reps: int
    seed: int
    n_pos: int
    n_neg: int
    identical: bool
    diff_reps: "numpy.ndarray"
    auc_diff_reps: "numpy.ndarray"

    def __eq__(self, other):
        if not isinstance(other, ApComparison):
            return NotImplemented
        mine, theirs = dict(self.__dict__), dict(other.__dict__)
        return all(mine.pop(k).tobytes() == theirs.pop(k).tobytes() for k in ("diff_reps", "auc_diff_reps")) and repr(mine) == repr(theirs)


def format_compare_ap(c: ApComparison) -> str:
    """The one `[compare_ap]` line of `--score CKPT --compare CKPT_B --compare_ap`."""
    return (f"[compare_ap] AP A {c.ap_a!r} B {c.ap_b!r} diff {c.diff!r} ± {c.diff_se!r} ({c.level:.0%}: [{c.diff_lo!r}, {c.diff_hi!r}]) "
            f"p {c.p!r} AUROC diff {c.auc_diff!r} ({c.level:.0%}: [{c.auc_diff_lo!r}, {c.auc_diff_hi!r}]) from {c.reps} paired stratified "
            f"replicates, seed {c.seed}, on {c.n_pos} positives, {c.n_neg} negatives")


def compare_ap(scores_a: torch.Tensor, scores_b: torch.Tensor, labels_u8: torch.Tensor, level: float = 0.95, reps: int = 1000,
               seed: int = 0, pos_cap: Optional[int] = None) -> ApComparison:
    """Whether two models' average precisions on the same labels differ: a paired stratified bootstrap, one
    `ggad_rank_bootstrap_pair_f32` call (csrc/rank_metrics.hip: the run-merge chain for either list, a table of where every element
    falls under either model, then one workgroup per replicate that draws ELEMENTS with Philox4x32-10 under `seed` and counts each
    at its own bin under A and under B) and one read-back of `24 + 4 reps` words.  Two unpaired `ap_ci` intervals are no substitute:
    on the same labels the two APs are strongly correlated.  The `ValueError`s of `ap_ci`, for either list."""
    import numpy as np
    o, words, reps, seed = _bootstrap_call("compare_ap", [scores_a, scores_b], labels_u8, level, reps, seed, 0.5, pos_cap)
    n_pos, n_neg = int(o[2]) + int(o[4]), int(o[3]) + int(o[5])
    ap_reps, num_reps = words[:2 * reps], words[2 * reps:].view(np.int64)
    d_ap = ap_reps[:reps] - ap_reps[reps:]
    d_num = num_reps[:reps] - num_reps[reps:]                                      # exact int64
    d_auc = d_num.astype(np.float64) / float(2 * n_pos * n_neg)
    same = not d_ap.any() and not d_num.any()
    q = [(1.0 - float(level)) / 2, (1.0 + float(level)) / 2]
    lo, hi = (float(v) for v in np.quantile(d_ap, q))
    alo, ahi = (float(v) for v in np.quantile(d_auc, q))
    nan = float("nan")
    p = min(1.0, 2.0 * min(1 + int((d_ap <= 0).sum()), 1 + int((d_ap >= 0).sum())) / (reps + 1))
    return ApComparison(ap_a=float(o[1]), ap_b=float(o[9]), diff=float(o[1]) - float(o[9]), diff_lo=lo, diff_hi=hi,
                        diff_se=float(d_ap.std(ddof=1)) if reps > 1 else nan, p=1.0 if same else p, auc_a=float(o[0]), auc_b=float(o[8]),
                        auc_diff=float(o[0]) - float(o[8]), auc_diff_lo=alo, auc_diff_hi=ahi,
                        auc_diff_se=float(d_auc.std(ddof=1)) if reps > 1 else nan, level=float(level), reps=reps, seed=seed,
                        n_pos=n_pos, n_neg=n_neg, identical=same, diff_reps=d_ap, auc_diff_reps=d_auc)


@dataclass
class Ranked:
    """The head of a ranking (`top_k`): rank j is the j-th highest score, equal scores in ascending position.  `pos` int32 positions
    in the scored array, `ids` int64 (the caller's ids at those positions, or `pos` widened), `scores` float32, `cum_pos` int32 --
    the label-1 elements among ranks 0..j -- or None without labels; all four on the device, `m` = min(k, n) long.  `n_pos`: the
    label-1 elements among ALL scored elements (0 without labels); `tied_left_out`: elements that tie with the last rank's score and
    did not make the list (> 0: the cut fell inside a tie)."""
    pos: torch.Tensor
    ids: torch.Tensor
    scores: torch.Tensor
    cum_pos: Optional[torch.Tensor]
    m: int
    n_pos: int
    tied_left_out: int


def top_k(scores: torch.Tensor, k: int, labels_u8: Optional[torch.Tensor] = None, ids: Optional[torch.Tensor] = None,
          wide: bool = False) -> Ranked:
    """The `min(k, n)` highest of float32 device `scores`, ranked by score descending and, among equal scores, by ascending position
    (-0.0 ties with +0.0): one `ggad_topk_f32` call and one read-back of its four meta words.  `labels_u8` (uint8, same shape):
    `cum_pos` and `n_pos` are filled.  `ids` (int64, same shape): `Ranked.ids = ids[pos]`.  A NaN score, a label other than 0/1 or a
    `k` outside 1..ggad_topk_max_k(): `ValueError`.  `wide=True`: `ggad_topk_wide_f32` (csrc/topk.hip: the candidates sorted in
    runs of 2,048 and merged), k up to ggad_topk_wide_max_k() = 4,194,304; the same list, and the same bits where both routes serve.
    Timings of both against a torch sort: profiles/topk_wide_time_line.json."""
    from . import _lib
    if scores.dtype != torch.float32 or scores.dim() != 1:
        raise ValueError("top_k takes float32 scores of a 1-D shape")
    if scores.device.type != "cuda":
        raise ValueError("top_k takes scores on a GPU (there is no CPU path)")
    if labels_u8 is not None and (labels_u8.dtype != torch.uint8 or labels_u8.shape != scores.shape or labels_u8.device != scores.device):
        raise ValueError("top_k takes uint8 labels of the scores' shape on the same GPU")
    if ids is not None and (ids.shape != scores.shape or ids.device != scores.device):
        raise ValueError("top_k takes ids of the scores' shape on the same GPU")
    lib = _lib.load()
    check_k(k, "top_k", lib, wide)
    k = int(k)
    entry = "ggad_topk_wide" if wide else "ggad_topk"
    n = scores.numel()
    scores = scores.contiguous()
    labels_u8 = labels_u8.contiguous() if labels_u8 is not None else None
    dev = scores.device
    with torch.cuda.device(dev):
        ws = torch.empty(int(getattr(lib, entry + "_workspace_elems")(n, k)), dtype=torch.int32, device=dev)
        pos = torch.empty(k, dtype=torch.int32, device=dev)
        val = torch.empty(k, dtype=torch.float32, device=dev)
        cum = torch.empty(k, dtype=torch.int32, device=dev) if labels_u8 is not None else None
        meta = torch.empty(4, dtype=torch.int64, device=dev)
        _lib.call(entry + "_f32", _lib.ptr(scores), _lib.ptr(labels_u8), n, k, _lib.ptr(pos), _lib.ptr(val), _lib.ptr(cum),
                  _lib.ptr(meta), _lib.ptr(ws))
        m, status, n_pos, left = (int(v) for v in meta.cpu().tolist())
    if status == 3:
        raise ValueError("top_k: a score is NaN")
    if status == 4:
        raise ValueError("top_k: a label is neither 0 nor 1")
    pos = pos[:m]
    pos64 = pos.long()
    return Ranked(pos=pos, ids=ids.long()[pos64] if ids is not None else pos64, scores=val[:m], cum_pos=cum[:m] if cum is not None else None,
                  m=m, n_pos=n_pos, tied_left_out=left)


def check_k(k, who: str, lib=None, wide: bool = False) -> None:
    """`ValueError` unless 1 <= k <= ggad_topk_max_k() -- `wide`: ggad_topk_wide_max_k() -- (asked of the library: no GPU needed)."""
    from . import _lib
    lib = lib or _lib.load()
    if wide:
        cap = int(lib.ggad_topk_wide_max_k())
        if int(k) != k or not 1 <= int(k) <= cap:
            raise ValueError(f"{who}: k = {k} is outside 1..ggad_topk_wide_max_k() = {cap}")
        return
    cap = int(lib.ggad_topk_max_k())
    if int(k) != k or not 1 <= int(k) <= cap:
        raise ValueError(f"{who}: k = {k} is outside 1..ggad_topk_max_k() = {cap} (the pairs one workgroup sorts in LDS)")


def precision_recall_at(ranked: Ranked, j: int) -> Tuple[float, float]:
    """(precision@j, recall@j) of a labelled `Ranked`, 1 <= j <= m: hits among the first j ranks over j and over `n_pos` (NaN when
    there are no positives at all)."""
    if ranked.cum_pos is None:
        raise ValueError("precision_recall_at needs a ranking made with labels")
    if not 1 <= int(j) <= ranked.m:
        raise ValueError(f"precision_recall_at: j = {j} is outside 1..m = {ranked.m}")
    hits = int(ranked.cum_pos[int(j) - 1])
    return hits / int(j), (hits / ranked.n_pos if ranked.n_pos else float("nan"))


def write_ranked(path, ranked, labels=None):
    """The `.npz` of config key `top_k_out`: `node` int64, `score` float32, `label` uint8, `cum_positives` int32 (both empty without
    labels), `n_pos`, `tied_left_out`.  `labels`: the labels of the scored list, indexed by `ranked.pos`.  Entries are stored with a
    fixed date, so equal rankings give equal files byte for byte."""
    import numpy as np
    pos = ranked.pos.cpu().numpy()
    has = labels is not None and ranked.cum_pos is not None
    arrays = {"node": ranked.ids.cpu().numpy().astype(np.int64), "score": ranked.scores.cpu().numpy().astype(np.float32),
              "label": np.asarray(labels).reshape(-1)[pos].astype(np.uint8) if has else np.zeros(0, dtype=np.uint8),
              "cum_positives": ranked.cum_pos.cpu().numpy().astype(np.int32) if has else np.zeros(0, dtype=np.int32),
              "n_pos": np.int64(ranked.n_pos), "tied_left_out": np.int64(ranked.tied_left_out)}
    write_npz_fixed_date(path, arrays)


def write_npz_fixed_date(path, arrays) -> None:
    """An uncompressed `.npz` of `arrays` (name -> array, in this order) whose entries carry a fixed date: equal arrays give equal
    files byte for byte (`write_ranked`, `explain.write_explained`)."""
    import zipfile

    import numpy as np
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            with z.open(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), "w", force_zip64=True) as fh:
                np.lib.format.write_array(fh, np.asanyarray(a), allow_pickle=False)
