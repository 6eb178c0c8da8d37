"""Numpy restatement of `ggad_select_decide_f64` and `ggad_select_copy_f32` (csrc/select.hip): plain loops over a list of
(auroc, ap, status) triples and parameter snapshots.  tests/test_select_cpu.py holds this against hand-worked cases;
tests/test_select_gpu.py holds the kernels against this."""
import numpy as np

NAN = float("nan")


def initial_state():
    """state4 = {best_value, best_epoch, epoch, taken} as the host initialises it."""
    return np.array([NAN, -1.0, 0.0, 0.0], dtype=np.float64)


def decide(state4, triple, which, curve=None):
    """One `ggad_select_decide_f64` call, in place on `state4` (and `curve`, (cap, 3) float64 or None); returns `taken`."""
    assert which in (0, 1)
    auroc, ap, status = (float(v) for v in triple)
    e = int(state4[2])
    if curve is not None and e < len(curve):
        curve[e] = (auroc, ap, status)
    value = ap if which else auroc
    taken = status == 0.0 and value == value and (state4[1] < 0.0 or value > state4[0])
    if taken:
        state4[0] = value
        state4[1] = float(e)
    state4[2] = float(e + 1)
    state4[3] = 1.0 if taken else 0.0
    return bool(taken)


def copy(state4, src, dst):
    """One or more `ggad_select_copy_f32` calls after one decide: every tensor of `src` replaces its `dst` (in place, bit for bit) if
    and only if state4[3] == 1."""
    if state4[3] == 1.0:
        for s, d in zip(src, dst):
            d.view(np.uint32)[...] = np.asarray(s).view(np.uint32)


def run(triples, which, params_by_epoch=None, curve_cap=None):
    """The whole sequence: dict(state4, curve, taken (list of bool), snapshot (list of arrays or None)).  `params_by_epoch[e]`: the list
    of float32 arrays the model holds when epoch e is decided."""
    state4 = initial_state()
    curve = np.full((len(triples) if curve_cap is None else curve_cap, 3), NAN, dtype=np.float64)
    snapshot = None
    if params_by_epoch is not None:
        snapshot = [np.full_like(np.asarray(p, dtype=np.float32), NAN) for p in params_by_epoch[0]]
    taken = []
    for e, t in enumerate(triples):
        taken.append(decide(state4, t, which, curve))
        if snapshot is not None:
            copy(state4, [np.asarray(p, dtype=np.float32) for p in params_by_epoch[e]], snapshot)
    return dict(state4=state4, curve=curve, taken=taken, snapshot=snapshot)


def same(a, b):
    """`==` on float64 arrays with NaNs compared by position."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# the sequence the CPU and GPU tests share: (auroc, ap, status) per epoch
#   0 invalid first epoch (one class only: status 1, auroc NaN)      -> never taken, best_epoch stays -1
#   1 first valid epoch                                              -> taken by both metrics
#   2 AUROC ties epoch 1 (strict >: not taken), AP improves          -> which = 1 takes it
#   3 AUROC improves, AP falls                                       -> which = 0 takes it
#   4 a NaN value with status 0 (cannot come from the metric kernels, but the rule must hold) -> never taken
#   5 better than everything, but status 2 (too many positives)     -> never taken
#   6 AUROC ties epoch 3, AP ties epoch 2                            -> neither
#   7 both improve                                                   -> both
#   8 both fall                                                      -> neither
SEQUENCE = [(NAN, 0.0, 1.0), (0.625, 0.25, 0.0), (0.625, 0.5, 0.0), (0.75, 0.125, 0.0), (NAN, NAN, 0.0), (0.99, 0.99, 2.0),
            (0.75, 0.5, 0.0), (0.875, 0.625, 0.0), (0.5, 0.0625, 0.0)]
TAKEN = {0: [False, True, False, True, False, False, False, True, False], 1: [False, True, True, False, False, False, False, True, False]}
# without the last two epochs the two metrics disagree on the best epoch: AUROC says 3, AP says 2
DISAGREE = SEQUENCE[:7]
