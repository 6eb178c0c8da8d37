"""The stratified bootstrap on the device: `ggad_rank_bootstrap_f32` (csrc/rank_metrics.hip), `metrics.ap_ci`, `ResidentSweep.ap_ci`,
config key `ap_ci` and `run.py --ap_ci`, against tests/bootstrap_ref.py.  Every native call runs on a workspace full of -1 and outputs
full of -7 / -1.  B = 64 replicates unless a test says otherwise.

  1. every case: the three histograms of every replicate equal the reference's as integers (and are zero beyond entry P), the AUROC
     numerators are equal as integers, |AP* - reference| <= (P + 4) 2^-53 (P terms of which each is one division of exact integers,
     added in any order with partial sums of at most P, then one division by P: the summation bound of P terms, relative to a sum
     <= P, over P), out16[0:8] holds the bits of `ggad_rank_wide_f32`'s out8, out16[8..15] = reps, P, Nn, four zeros, status 0.
     The cases: those of tests/rank_wide_ref.py with at most ggad_rank_bootstrap_max_pos() positives and two of each class
     (`dgraph_like`, 1.7 M scores: all 64 replicates run, the reference makes four of them, 0, 1, 62 and 63, at a third of a second
     each), `heavy_ties` and `quantised` of the wide list cut to the cap, and the new ones of `_new_cases`;
  2. fewer than two of a class (status 8), the cap plus one (status 9, and the `ValueError` names the cap), the chain's own statuses;
  3. B = 1 and B = 4,096; the same seed twice, another seed;
  4. outputs and workspace carved out of dirty blocks (tests/dirty.py), one workspace reused; a captured graph replayed twice;
  5. `metrics.ap_ci`, `ResidentSweep.ap_ci`, the refused arguments;
  6. `ModelHandler` and `run.py` with the option on and off."""
import functools
import glob
import os
import random

import numpy as np
import pytest
import torch

from ggad_amd import synth
import bootstrap_ref as BR
import dirty as D
import rank_wide_ref as RW

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = -7.0
B = 64
SEED = 0x9E3779B97F4A7C15
CAP = BR.MAX_POS
SOME = (0, 1, 62, 63)                                   # the replicates the reference makes of `dgraph_like`


def _lib():
    from ggad_amd import _lib
    return _lib, _lib.load()


def _rand(rng, n, p):
    y = np.zeros(n, dtype=np.uint8)
    y[rng.choice(n, p, replace=False)] = 1
    return rng.random(n).astype(np.float32), y


def _cut(s, y, p):
    """The list without its positives beyond the p-th (in position order)."""
    keep = np.ones(len(y), dtype=bool)
    keep[np.flatnonzero(y == 1)[p:]] = False
    return np.ascontiguousarray(s[keep]), np.ascontiguousarray(y[keep])


@functools.lru_cache(maxsize=None)
def _new_cases():
    rng = np.random.default_rng(77)
    wide = {c[0]: c for c in RW.cases()}
    out = [("p2n2", np.array([0.1, 0.9, 0.4, 0.6], dtype=np.float32), np.array([1, 0, 1, 0], dtype=np.uint8))]
    out.append(("odd_odd", *_rand(rng, 1504, 501)))                              # 501 and 1,003 draws: both last calls half used
    out.append(("heavy_ties_cut", *_cut(*wide["heavy_ties_wide"][1:3], CAP)))
    out.append(("quantised_cut", *_cut(*wide["quantised"][1:3], CAP)))
    out.append(("all_equal", np.full(700, 0.5, dtype=np.float32), _rand(rng, 700, 123)[1]))
    s, y = _rand(rng, 1800, 300)
    out.append(("separated", (s + y).astype(np.float32), y))                     # every negative below every positive: bin 0 only
    out.append(("negatives_above", (s - y).astype(np.float32), y))               # every negative above every positive: bin P only
    s, y = _rand(rng, 400, 40)
    s = s.copy()
    s[np.flatnonzero(y == 1)[7]] = np.float32(2.0)                               # the top positive alone above every negative
    out.append(("top_alone", s, y))
    out.append(("at_boot_cap", *_rand(rng, CAP + 2500, CAP)))
    out.append(("n200k", *_rand(rng, 200000, 1000)))                             # every thread loops over the negatives' draws
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _all_cases():
    out = {}
    for name, s, y, _ in RW.cases():
        p = int(y.sum())
        if 2 <= p <= CAP and len(y) - p >= 2:
            out[name] = (s, y)
    for name, s, y in _new_cases():
        out[name] = (s, y)
    return out


NAMES = list(_all_cases())


@functools.lru_cache(maxsize=None)
def _ref(name, seed=SEED, reps=B):
    """The reference's replicates of a case, made once per process: dict of tests/bootstrap_ref.py's `bootstrap` (for `dgraph_like`
    only the replicates of SOME, at their places)."""
    s, y = _all_cases()[name]
    if name != "dgraph_like":
        return BR.bootstrap(s, y, seed, reps)
    pos, hist_u, hist_e = BR.bins(s, y)[:3]
    P, Nn = len(pos), int(hist_u.sum())
    ap, num = np.full(reps, np.nan), np.zeros(reps, dtype=np.int64)
    hist = np.zeros((reps, 3, P + 1), dtype=np.int64)
    for r in SOME:
        h = BR.replicate(seed, r, hist_u, hist_e)
        ap[r], num[r] = BR.terms(pos, *h)
        hist[r] = h
    return dict(P=P, Nn=Nn, pos=pos, ap=ap, num=num, hist=hist, auc=num / float(2 * P * Nn))


class Device:
    """One input on the device, uploaded once."""

    def __init__(self, s, y):
        self.n = len(s)
        self.s, self.y = torch.tensor(np.asarray(s)).to(DEV), torch.tensor(np.asarray(y)).to(DEV)

    def wide(self, pos_cap, thres=0.5):
        L, lib = _lib()
        ws = torch.full((int(lib.ggad_rank_wide_workspace_elems(self.n, pos_cap)),), -1, dtype=torch.int32, device=DEV)
        out8 = torch.full((8,), FILL, dtype=torch.float64, device=DEV)
        L.call("ggad_rank_wide_f32", L.ptr(self.s), L.ptr(self.y), self.n, pos_cap, float(thres), L.ptr(out8), L.ptr(ws))
        return out8.cpu().numpy()

    def boot(self, pos_cap, seed=SEED, reps=B, thres=0.5, hist=True, ws=None):
        """(out16, rep_ap, rep_num, hist int32[reps, 3, pos_cap + 1] or None) as host arrays."""
        L, lib = _lib()
        need = int(lib.ggad_rank_bootstrap_workspace_elems(self.n, pos_cap))
        assert need > 0
        if ws is None:
            ws = torch.full((need,), -1, dtype=torch.int32, device=DEV)            # (dirty on purpose)
        assert ws.numel() >= need
        out16 = torch.full((16,), FILL, dtype=torch.float64, device=DEV)
        ap = torch.full((reps,), FILL, dtype=torch.float64, device=DEV)
        num = torch.full((reps,), -1, dtype=torch.int64, device=DEV)
        h = torch.full((reps, 3, pos_cap + 1), -1, dtype=torch.int32, device=DEV) if hist else None
        L.call("ggad_rank_bootstrap_f32", L.ptr(self.s), L.ptr(self.y), self.n, pos_cap, float(thres), seed, reps, L.ptr(out16),
               L.ptr(ap), L.ptr(num), L.ptr(h), L.ptr(ws))
        return out16.cpu().numpy(), ap.cpu().numpy(), num.cpu().numpy(), None if h is None else h.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _device(name):
    return Device(*_all_cases()[name])


def _bits(*arrays):
    return np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.int64) if a.dtype.itemsize == 8 else
                           np.ascontiguousarray(a).reshape(-1).astype(np.int64) for a in arrays if a is not None])


def _check(tag, got, ref, out8, reps=B, which=None):
    o, ap, num, hist = got
    P, Nn = ref["P"], ref["Nn"]
    which = list(range(reps)) if which is None else list(which)
    worst = float(np.abs(ap[which] - ref["ap"][which]).max())
    print(f"[{tag}] P {P} Nn {Nn} status {o[15]:.0f}; worst |AP* - reference| {worst:.3e} against the bound {(P + 4) * 2.0 ** -53:.3e}; "
          f"AP* in [{ap.min()!r}, {ap.max()!r}]")
    np.testing.assert_array_equal(o[:8].view(np.int64), out8.view(np.int64), err_msg=tag)
    assert o[8:].tolist() == [float(reps), float(P), float(Nn), 0.0, 0.0, 0.0, 0.0, 0.0], (tag, o[8:].tolist())
    if hist is not None:
        np.testing.assert_array_equal(hist[which][:, :, :P + 1], ref["hist"][which], err_msg=tag)
        assert (hist[:, :, P + 1:] == 0).all(), tag
        assert (hist[:, 0].sum(axis=1) == P).all() and (hist[:, 1].sum(axis=1) == Nn).all(), tag     # every replicate, also of dgraph_like
    np.testing.assert_array_equal(num[which], ref["num"][which], err_msg=tag)
    assert worst <= (P + 4) * 2.0 ** -53, tag
    assert np.isfinite(ap).all() and (num >= 0).all() and (num <= 2 * P * Nn).all(), tag


# ------------------------------------------------------------------ 1: every case
@pytest.mark.parametrize("name", NAMES)
def test_every_case(name):
    s, y = _all_cases()[name]
    P = int(y.sum())
    d = _device(name)
    ref = _ref(name)
    got = d.boot(P)
    _check(name, got, ref, d.wide(P), which=SOME if name == "dgraph_like" else None)
    o, ap, num, hist = got
    Nn = len(y) - P
    if name in ("all_equal", "all_tied", "all_tied_wide"):
        assert (num == P * Nn).all() and np.abs(ap - P / (P + Nn)).max() <= 4 * 2.0 ** -53
    if name == "separated":
        assert (ap == 1.0).all() and (num == 2 * P * Nn).all() and (hist[:, 1, 0] == Nn).all()
    if name == "negatives_above":
        assert (num == 0).all() and (hist[:, 1, P] == Nn).all()
    if name == "top_alone":
        undrawn = ref["hist"][:, 0, P - 1] == 0
        assert undrawn.any() and (ref["hist"][:, 1, P] == 0).all()                  # 0 / 0 in the reference's replicates: the select
        print(f"[top_alone] {int(undrawn.sum())} of {B} replicates leave the top positive undrawn")
    if name == "odd_odd":
        assert P % 2 == 1 and Nn % 2 == 1
    if name in ("p8193", "at_boot_cap", "n200k"):                                  # a looser cap: other grids and LDS, the same bits
        again = d.boot(min(len(s), P + 700), hist=False)
        np.testing.assert_array_equal(_bits(*again[:3]), _bits(*got[:3]))


# ------------------------------------------------------------------ 2: statuses
def test_statuses():
    cases = {c[0]: c for c in RW.cases()}
    nan = float("nan")
    for name in ("tiny", "lone_positive", "lone_negative", "pad_p1"):              # both classes, fewer than two of one
        _, s, y, thres = cases[name]
        P = int(y.sum())
        d = Device(s, y)
        o, ap, num, hist = d.boot(max(1, P), thres=thres)
        np.testing.assert_array_equal(o[:8].view(np.int64), d.wide(max(1, P), thres).view(np.int64))
        assert o[7] == 0.0 and o[15] == float(BR.TOO_FEW) == 8.0 and o[8:11].tolist() == [float(B), float(P), float(len(y) - P)]
        assert np.isnan(ap).all() and (num == 0).all() and (hist == 0).all()
    rng = np.random.default_rng(9)
    s, y = _rand(rng, CAP + 1 + 2500, CAP + 1)                                     # the cap plus one
    d = Device(s, y)
    o, ap, num, _ = d.boot(CAP + 1, hist=False)
    np.testing.assert_array_equal(o[:8].view(np.int64), d.wide(CAP + 1).view(np.int64))
    assert o[7] == 0.0 and o[15] == float(BR.TOO_MANY) == 9.0 and o[9] == CAP + 1 and np.isnan(ap).all() and (num == 0).all()
    from ggad_amd.metrics import ap_ci
    for kw in ({}, {"pos_cap": CAP + 1}, {"pos_cap": CAP + 500}):
        with pytest.raises(ValueError, match=rf"{CAP + 1} positives are more than ggad_rank_bootstrap_max_pos\(\) = {CAP}"):
            ap_ci(d.s, d.y, reps=8, **kw)
    with pytest.raises(ValueError, match="pos_cap = 100"):
        ap_ci(d.s, d.y, reps=8, pos_cap=100)
    o, ap, num, _ = d.boot(CAP, hist=False)                                        # the chain's own status 2
    assert o[7] == o[15] == 2.0 and np.isnan(ap).all() and (num == 0).all()
    bad = s.copy()
    bad[11] = nan
    y2 = y.copy()
    y2[5] = 2
    for dd, status in ((Device(bad, y), 3), (Device(s, y2), 4), (Device(s, np.zeros_like(y)), 1), (Device(s, np.ones_like(y)), 1)):
        o, ap, num, _ = dd.boot(len(s), hist=False)
        assert o[7] == o[15] == float(status) and np.isnan(ap).all() and (num == 0).all()


def test_refused_without_a_launch():
    L, lib = _lib()
    d = _device("p2047")
    p = L.ptr
    out = torch.full((16,), FILL, dtype=torch.float64, device=DEV)
    ap = torch.full((B,), FILL, dtype=torch.float64, device=DEV)
    num = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    ws = torch.full((int(lib.ggad_rank_bootstrap_workspace_elems(d.n, 2047)) + 4,), -1, dtype=torch.int32, device=DEV)
    assert lib.ggad_rank_bootstrap_max_pos() == CAP and lib.ggad_rank_bootstrap_max_reps() == BR.MAX_REPS == 4096
    assert lib.ggad_rank_bootstrap_workspace_elems(d.n, 0) == 0 and lib.ggad_rank_bootstrap_workspace_elems(-1, 5) == 0
    call = lib.ggad_rank_bootstrap_f32
    for pos_cap, reps, o_, a_, n_, w in ((0, B, p(out), p(ap), p(num), p(ws)), (int(lib.ggad_rank_wide_max_pos()) + 1, B, p(out), p(ap), p(num), p(ws)),
                                         (2047, 0, p(out), p(ap), p(num), p(ws)), (2047, -3, p(out), p(ap), p(num), p(ws)),
                                         (2047, 4097, p(out), p(ap), p(num), p(ws)), (2047, B, 0, p(ap), p(num), p(ws)),
                                         (2047, B, p(out), 0, p(num), p(ws)), (2047, B, p(out), p(ap), 0, p(ws)),
                                         (2047, B, p(out), p(ap), p(num), 0), (2047, B, p(out), p(ap), p(num), p(ws) + 4)):
        assert call(p(d.s), p(d.y), d.n, pos_cap, 0.5, SEED, reps, o_, a_, n_, None, w, None) == -1
    assert call(0, p(d.y), d.n, 2047, 0.5, SEED, B, p(out), p(ap), p(num), None, p(ws), None) == -1
    assert call(p(d.s), p(d.y), 2 ** 31, 2047, 0.5, SEED, B, p(out), p(ap), p(num), None, p(ws), None) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all() and (ap.cpu().numpy() == FILL).all() and bool((num == -1).all()) and bool((ws == -1).all())


# ------------------------------------------------------------------ 3: replicate counts and seeds
def test_one_replicate_and_the_most():
    d = _device("n63")
    s, y = _all_cases()["n63"]
    P = int(y.sum())
    out8 = d.wide(P)
    _check("n63/B=1", d.boot(P, reps=1), BR.bootstrap(s, y, SEED, 1), out8, reps=1)
    most = d.boot(P, reps=4096)
    ref = BR.bootstrap(s, y, SEED, 4096)
    _check("n63/B=4096", most, ref, out8, reps=4096)
    np.testing.assert_array_equal(_bits(*d.boot(P)[1:]), _bits(most[1][:B], most[2][:B], most[3][:B]))     # a replicate depends on r alone


def test_seeds():
    d = _device("odd_odd")
    P = int(_all_cases()["odd_odd"][1].sum())
    a, b = d.boot(P), d.boot(P)
    np.testing.assert_array_equal(_bits(*a), _bits(*b))
    for seed in (SEED + 1, SEED ^ (1 << 32), 0, (1 << 64) - 1):                     # the low word, the high word, the ends
        c = d.boot(P, seed=seed)
        np.testing.assert_array_equal(c[0].view(np.int64), a[0].view(np.int64))     # the point estimates do not depend on it
        assert not np.array_equal(c[3][:, 0], a[3][:, 0]) and not np.array_equal(c[3][:, 1], a[3][:, 1]) and not np.array_equal(c[1], a[1])
        _check(f"odd_odd/seed {seed:#x}", c, _ref("odd_odd", seed), d.wide(P))


# ------------------------------------------------------------------ 4: dirty memory, reuse, capture
def _carve(n, fill, dtype):
    """dtype[n] inside an int32 block of `fill` with guards (tests/dirty.py)."""
    words = n * torch.empty((), dtype=dtype).element_size() // 4
    block, t = D.int_like(words, fill)
    return block, t.view(dtype)


def _guards_hold(block, fill):
    assert bool((block[:D.GUARD] == fill).all()) and bool((block[-D.GUARD:] == fill).all())


def test_dirty_outputs_and_a_reused_workspace_change_nothing():
    L, lib = _lib()
    order = ("at_boot_cap", "odd_odd", "p2n2")
    caps = {n: int(_all_cases()[n][1].sum()) for n in order}
    need = max(int(lib.ggad_rank_bootstrap_workspace_elems(_device(n).n, caps[n])) for n in order)
    wblock, shared = D.int_like(need, D.NAN_BITS)
    for k in range(2):
        for name in order:
            d, cap = _device(name), caps[name]
            clean = d.boot(cap)
            blocks = [_carve(16, D.NAN_BITS, torch.float64), _carve(B, D.NAN_BITS, torch.float64), _carve(B, D.NAN_BITS, torch.int64),
                      _carve(B * 3 * (cap + 1), D.NAN_BITS, torch.int32)]
            o, ap, num, h = (t for _, t in blocks)
            L.call("ggad_rank_bootstrap_f32", L.ptr(d.s), L.ptr(d.y), d.n, cap, 0.5, SEED, B, L.ptr(o), L.ptr(ap), L.ptr(num), L.ptr(h),
                   L.ptr(shared))
            D.dirty_lines()
            got = (o.cpu().numpy(), ap.cpu().numpy(), num.cpu().numpy(), h.cpu().numpy().reshape(B, 3, cap + 1))
            np.testing.assert_array_equal(_bits(*got), _bits(*clean), err_msg=f"{name} round {k}")
            for block, _ in blocks:
                _guards_hold(block, D.NAN_BITS)
            _guards_hold(wblock, D.NAN_BITS)


def test_captured_and_replayed_twice():
    L, lib = _lib()
    name = "heavy_ties_cut"
    d = _device(name)
    cap = int(_all_cases()[name][1].sum())
    eager = d.boot(cap)
    ws = torch.empty(int(lib.ggad_rank_bootstrap_workspace_elems(d.n, cap)), dtype=torch.int32, device=DEV)
    out16 = torch.zeros(16, dtype=torch.float64, device=DEV)
    ap, num = torch.zeros(B, dtype=torch.float64, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
    hist = torch.zeros((B, 3, cap + 1), dtype=torch.int32, device=DEV)
    scores = d.s.clone()

    def call():
        L.call("ggad_rank_bootstrap_f32", L.ptr(scores), L.ptr(d.y), d.n, cap, 0.5, SEED, B, L.ptr(out16), L.ptr(ap), L.ptr(num), L.ptr(hist),
               L.ptr(ws))
    call()                                                                         # (the LDS opt-in happens outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        for t in (out16, ap):
            t.fill_(FILL)
        num.fill_(-1), hist.fill_(-1), ws.fill_(-1)
        graph.replay()
        got = (out16.cpu().numpy(), ap.cpu().numpy(), num.cpu().numpy(), hist.cpu().numpy())
        np.testing.assert_array_equal(_bits(*got), _bits(*eager))
    scores.copy_(-d.s)                                                             # the replay reads the new scores
    graph.replay()
    other = Device(-_all_cases()[name][0], _all_cases()[name][1]).boot(cap)
    got = (out16.cpu().numpy(), ap.cpu().numpy(), num.cpu().numpy(), hist.cpu().numpy())
    np.testing.assert_array_equal(_bits(*got), _bits(*other))
    assert not np.array_equal(got[2], eager[2])


# ------------------------------------------------------------------ 5: the public calls
def _agrees(ci, ref, point_ap, point_auc, level, tag):
    lo, hi, se, bias = BR.summary(point_ap, ref["ap"], level)
    alo, ahi, ase, _ = BR.summary(point_auc, ref["auc"], level)
    for got, want, what in ((ci.ap_lo, lo, "ap_lo"), (ci.ap_hi, hi, "ap_hi"), (ci.ap_se, se, "ap_se"), (ci.ap_bias, bias, "ap_bias"),
                            (ci.auc_lo, alo, "auc_lo"), (ci.auc_hi, ahi, "auc_hi"), (ci.auc_se, ase, "auc_se")):
        assert abs(got - want) <= 1e-12, (tag, what, got, want)


@pytest.mark.parametrize("name", ["quantised_cut", "n63"])
def test_ap_ci_against_the_reference(name):
    from ggad_amd.metrics import BootstrapInterval, ap_ci, binary_report, format_ap_ci, rank_report_wide
    s, y = _all_cases()[name]
    d = _device(name)
    P = int(y.sum())
    ref = _ref(name)
    point = rank_report_wide(d.s, d.y, 0.5, pos_cap=P)
    for pos_cap in (None, P):
        for level in (0.95, 0.5):
            ci = ap_ci(d.s, d.y, level, reps=B, seed=SEED, pos_cap=pos_cap)
            assert isinstance(ci, BootstrapInterval) and (ci.n_pos, ci.n_neg, ci.level, ci.reps, ci.seed) == (P, len(y) - P, level, B, SEED)
            assert ci.ap == point["ap"] and ci.auc == point["auc"] and ci.ap_lo <= ci.ap_hi and ci.auc_lo <= ci.auc_hi
            assert np.abs(ci.ap_reps - ref["ap"]).max() <= (P + 4) * 2.0 ** -53 and np.array_equal(ci.auc_reps, ref["auc"])
            _agrees(ci, ref, ci.ap, ci.auc, level, name)
            assert ci.ap_reps.dtype == ci.auc_reps.dtype == np.float64 and len(ci.ap_reps) == len(ci.auc_reps) == B
    b = binary_report(d.s, d.y, 0.5)
    assert list(ci.report) == list(b) and all(ci.report[k] == b[k] for k in ("tp", "fp", "fn", "tn", "f1_macro", "gmean"))
    assert ci == ap_ci(d.s, d.y, 0.5, reps=B, seed=SEED, pos_cap=P) and ci != ap_ci(d.s, d.y, 0.5, reps=B, seed=SEED + 1, pos_cap=P)
    assert format_ap_ci(ci) == (f"[ap_ci] AP {ci.ap!r} ± {ci.ap_se!r} (50%: [{ci.ap_lo!r}, {ci.ap_hi!r}], bias {ci.ap_bias!r}) AUROC {ci.auc!r} "
                                f"(50%: [{ci.auc_lo!r}, {ci.auc_hi!r}]) from {B} stratified replicates, seed {SEED}, on {P} positives, "
                                f"{len(y) - P} negatives")
    one = ap_ci(d.s, d.y, reps=1, seed=SEED, pos_cap=P)                            # one replicate: no spread to speak of
    assert np.isnan(one.ap_se) and one.ap_lo == one.ap_hi == one.ap_reps[0]
    default = ap_ci(d.s, d.y)
    assert (default.reps, default.seed, default.level) == (1000, 0, 0.95) and default.ap_lo < default.ap < default.ap_hi


def test_ap_ci_refuses():
    from ggad_amd.metrics import ap_ci
    d = _device("p2047")
    s, y = _all_cases()["p2047"]
    bad = s.copy()
    bad[5] = np.nan
    y2 = y.copy()
    y2[5] = 3
    for args, text in (((torch.tensor(bad).to(DEV), d.y), "NaN"), ((d.s, torch.tensor(y2).to(DEV)), "neither 0 nor 1"),
                       ((d.s, torch.zeros_like(d.y)), "Only one class"), ((d.s, torch.ones_like(d.y)), "Only one class")):
        with pytest.raises(ValueError, match=text):
            ap_ci(*args, reps=4)
    for args in ((d.s.cpu(), d.y.cpu()), (d.s, d.y.cpu()), (d.s.double(), d.y), (d.s, d.y.int()), (d.s[:-1], d.y), (d.s.view(-1, 1), d.y.view(-1, 1))):
        with pytest.raises(ValueError, match="ap_ci takes"):
            ap_ci(*args, reps=4)
    for level in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="level"):
            ap_ci(d.s, d.y, level, reps=4)
    for reps in (0, -1, 4097, 2.5):
        with pytest.raises(ValueError, match=r"reps = .* is outside 1..ggad_rank_bootstrap_max_reps\(\) = 4096"):
            ap_ci(d.s, d.y, reps=reps)
    for seed in (-1, 1 << 64, 0.5):
        with pytest.raises(ValueError, match="seed"):
            ap_ci(d.s, d.y, reps=4, seed=seed)
    with pytest.raises(ValueError, match="pos_cap = 2046"):
        ap_ci(d.s, d.y, reps=4, pos_cap=2046)
    with pytest.raises(ValueError, match="pos_cap"):
        ap_ci(d.s, d.y, reps=4, pos_cap=0)
    cases = {c[0]: c for c in RW.cases()}
    for name in ("lone_positive", "lone_negative"):
        _, s1, y1, _ = cases[name]
        d1 = Device(s1, y1)
        with pytest.raises(ValueError, match="needs at least two positives and two negatives"):
            ap_ci(d1.s, d1.y, reps=4)


N_NODES = 3000


def test_resident_sweep_ap_ci():
    from ggad_amd import metrics
    from ggad_amd.dgraph import normalize_features
    from ggad_amd.eval_cache import ResidentSweep
    from ggad_amd.graph import DeviceGraph
    from ggad_amd.graphsage import GCN, FeatureTable, GCNAggregator, GCNEncoder
    rowptr, col = synth.make_graph(N_NODES, 30000, 3, kind="powerlaw", max_degree=200)
    rng = np.random.default_rng(8)
    cases = rng.integers(0, N_NODES, 6000).astype(np.int64)
    lab = np.zeros(len(cases), dtype=np.int64)
    lab[rng.choice(len(cases), 700, replace=False)] = 1
    torch.manual_seed(0)
    graph = DeviceGraph(rowptr, col, DEV)
    features = FeatureTable(torch.from_numpy(normalize_features(synth.make_features(N_NODES, 17, 3)).astype(np.float32)))
    enc = GCNEncoder(features, 17, 64, graph, GCNAggregator(features, cuda=True), gcn=True, cuda=True)
    model = GCN(2, enc)
    enc.engine.sync_params()
    sweep = ResidentSweep(model, cases, lab, 150)
    scores = sweep.scores()
    ci = sweep.ap_ci(0.9, B, 11)
    assert sweep.n_pos == 700 and (ci.n_pos, ci.n_neg, ci.reps, ci.seed, ci.level) == (700, 5300, B, 11, 0.9)
    assert ci == metrics.ap_ci(scores, sweep.labels, 0.9, B, 11, pos_cap=700) == sweep.ap_ci(0.9, B, 11, scores=scores)
    ref = BR.bootstrap(scores.cpu().numpy(), lab, 11, B, keep_hist=False)
    assert np.array_equal(ci.auc_reps, ref["auc"]) and np.abs(ci.ap_reps - ref["ap"]).max() <= 704 * 2.0 ** -53
    _agrees(ci, ref, ci.ap, ci.auc, 0.9, "sweep")
    with pytest.raises(ValueError, match="without labels"):
        ResidentSweep(model, cases, None, 150).ap_ci()


# ------------------------------------------------------------------ 6: the handler and run.py
def _masked(out):
    """A handler run's stdout without what differs between two identical runs: wall-clock times and the time-stamped checkpoint path."""
    import re
    keep = []
    for ln in out.splitlines():
        if ln.startswith(("total_time is", "Model path:")):
            continue
        keep.append(re.sub(r"time: [-+0-9.e]+s", "time: *", ln))
    return keep


def test_model_handler_with_ap_ci_on_and_off(tmp_path, capsys):
    from ggad_amd import metrics
    from ggad_amd.model_handler import ModelHandler
    n = 30000
    rowptr, col = synth.make_graph(n, 300000, 3, kind="powerlaw", max_degree=200)
    feat = synth.make_features(n, 17, 3)
    lab = synth.make_labels(n, 0.05, 3)
    rowptr, col, feat = synth.plant_anomalies(rowptr, col, feat, lab, 3, scale=0.25, rewire=0.5)
    runs = {}
    for tag, extra, cache in (("without", {}, True), ("without_plain", {}, False), ("off", {"ap_ci": 0, "boot_reps": 64, "boot_seed": 5}, True),
                              ("on", {"ap_ci": 0.9, "boot_reps": 64, "boot_seed": 5}, True),
                              ("on_plain", {"ap_ci": 0.9, "boot_reps": 64, "boot_seed": 5}, False)):
        cfg = dict(data_name="synthetic", data_dir="", data=((rowptr, col), feat, lab), seed=72, model="GCN", multi_relation="GNN",
                   emb_size=64, thres=0.4, lr=0.005, weight_decay=0.007, batch_size=60, num_epochs=2, valid_epochs=1, num_batches=6,
                   n_pseudo=20, save_dir=str(tmp_path / tag) + "/", test_ratio=0.67, device=0, eval_cache=cache, **extra)
        random.seed(72)
        np.random.seed(72)
        torch.manual_seed(72)
        capsys.readouterr()
        h = ModelHandler(cfg)
        res = h.train()
        out = capsys.readouterr().out
        files = sorted(glob.glob(str(tmp_path / tag / "*" / "*")))
        runs[tag] = dict(h=h, cfg=cfg, res=res, out=out, files=files, ckpt=[f for f in files if f.endswith(".pkl")][0])
    without, off, on, plain = (runs[k] for k in ("without", "off", "on", "on_plain"))
    assert "[ap_ci]" not in without["out"] and without["h"].ap_interval is None
    assert _masked(off["out"]) == _masked(without["out"]) and off["h"].ap_interval is None      # the key at 0: a run without it
    assert [os.path.basename(f) for f in off["files"]] == [os.path.basename(f) for f in without["files"]]
    for fa, fb in zip(off["files"], without["files"]):
        assert open(fa, "rb").read() == open(fb, "rb").read(), os.path.basename(fa)
    for r, base in ((on, without), (plain, runs["without_plain"])):                # (the plain sweep's metrics come from another route)
        assert r["res"] == base["res"] and r["out"].count("[ap_ci]") == 1 and r["out"].splitlines()[-1].startswith("[ap_ci] AP ")
        assert [ln for ln in _masked(r["out"]) if not ln.startswith("[ap_ci]")] == _masked(base["out"])
        assert open(r["ckpt"], "rb").read() == open(base["ckpt"], "rb").read()
    h = on["h"]
    sweep = h.eval_sweeps[1]
    scores = sweep.scores()
    ci = metrics.ap_ci(scores, sweep.labels, 0.9, 64, 5, pos_cap=sweep.n_pos)
    assert h.ap_interval == ci == plain["h"].ap_interval
    assert on["out"].splitlines()[-1] == metrics.format_ap_ci(ci) and "(90%: [" in on["out"].splitlines()[-1]
    ref = BR.bootstrap(scores.cpu().numpy(), np.asarray(h.dataset["y_test"]), 5, 64, keep_hist=False)
    assert np.array_equal(ci.auc_reps, ref["auc"]) and np.abs(ci.ap_reps - ref["ap"]).max() <= (ci.n_pos + 4) * 2.0 ** -53
    _agrees(ci, ref, ci.ap, ci.auc, 0.9, "handler")
    capsys.readouterr()
    h2 = ModelHandler(on["cfg"])                                                   # score(): the line again
    got_scores, _ = h2.score(on["ckpt"])
    out2 = capsys.readouterr().out
    assert torch.equal(got_scores, scores) and h2.ap_interval == ci and out2.count("[ap_ci]") == 1
    h3 = ModelHandler(without["cfg"])
    h3.score(on["ckpt"])
    assert "[ap_ci]" not in capsys.readouterr().out and h3.ap_interval is None
    with pytest.raises(ValueError, match="needs `model: 'GCN'`"):
        ModelHandler(dict(plain["cfg"], model="SAGE"))
    with pytest.raises(ValueError, match="confidence level"):
        ModelHandler(dict(on["cfg"], ap_ci=1.5))


def test_run_py_ap_ci(tmp_path, capsys):
    import contextlib
    import io
    import run
    a_pt, b_pt = str(tmp_path / "a.pt"), str(tmp_path / "b.pt")
    base = ["--synthetic", "--dataset", "reddit", "--quiet"]
    capsys.readouterr()
    assert run.main(base + ["--num_epoch", "4", "--save", a_pt]) is None
    out_a = capsys.readouterr().out
    assert run.main(base + ["--num_epoch", "4", "--save", b_pt, "--ap_ci", "--boot_reps", "64"]) is None
    out_b = capsys.readouterr().out
    assert "[ap_ci]" not in out_a and out_b.count("[ap_ci]") == 1
    sa, sb = (torch.load(f, map_location="cpu", weights_only=True)["state_dict"] for f in (a_pt, b_pt))
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)     # the option does not touch the training
    scores = run.main(base + ["--score", a_pt, "--ap_ci", "0.9", "--boot_reps", "64", "--boot_seed", "3"])
    out = capsys.readouterr().out
    plain = run.main(base + ["--score", a_pt])
    out_plain = capsys.readouterr().out
    assert "[ap_ci]" not in out_plain and np.array_equal(scores, plain)
    lines = [ln for ln in out.splitlines() if ln.startswith("[ap_ci]")]
    assert len(lines) == 1 and [ln for ln in out.splitlines() if not ln.startswith("[ap_ci]")] == out_plain.splitlines()
    args = run.parse(base)
    random.seed(args.seed), np.random.seed(args.seed), torch.manual_seed(args.seed)
    with contextlib.redirect_stdout(io.StringIO()):
        g = run.load_graph(args)
    y = np.asarray(g.ano_label).reshape(-1)
    idx = np.asarray(g.idx_test, dtype=np.int64)
    from ggad_amd.metrics import ap_ci, format_ap_ci
    y8 = torch.from_numpy(y[idx].astype(np.uint8)).to(DEV)
    ci = ap_ci(torch.from_numpy(scores[idx]).to(DEV), y8, 0.9, 64, 3, pos_cap=int(y[idx].sum()))
    assert lines[0] == format_ap_ci(ci) and f"from 64 stratified replicates, seed 3, on {int(y[idx].sum())} positives" in lines[0]
    ref = BR.bootstrap(scores[idx], y[idx], 3, 64, keep_hist=False)
    assert np.array_equal(ci.auc_reps, ref["auc"])
    _agrees(ci, ref, ci.ap, ci.auc, 0.9, "run.py")
    for argv in (["--boot_reps", "10"], ["--ap_ci", "1.5"], ["--ap_ci", "--boot_reps", "0"], ["--ap_ci", "--boot_seed", "-1"]):
        with pytest.raises(SystemExit):
            run.parse(base + argv)
    capsys.readouterr()
