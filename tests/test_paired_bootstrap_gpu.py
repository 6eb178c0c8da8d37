"""The paired stratified bootstrap on the device: `ggad_rank_bootstrap_pair_f32` (csrc/rank_metrics.hip), `metrics.compare_ap`,
`ResidentSweep.compare_ap`, config key `compare_ap` and `run.py --compare_ap`, against tests/paired_bootstrap_ref.py.  Every native
call runs on a workspace full of -1 and outputs full of -7 / -1.  B = 64 replicates unless a test says otherwise.

  1. every case: all six histograms of every replicate (w, cU, cE of A, then of B) equal the reference's as integers and are zero
     beyond entry P, both AUROC numerators are equal as integers, |AP* - reference| <= (P + 4) 2^-53 per model (the bound derived in
     tests/test_bootstrap_gpu.py: the formulas and the summation order are `ggad_rank_bootstrap_f32`'s), out24[0:8] and [8:16] hold
     the bits of `ggad_rank_wide_f32`'s out8 for each list, out24[16..23] = reps, P, Nn, four zeros, status 0.  `dgraph_like`: all
     64 replicates run, the reference makes four of them (0, 1, 62, 63) for both models;
  2. the statuses and the calls refused without a launch;
  3. B = 1 and B = 4,096; the same seed twice, another seed;
  4. outputs and workspace carved out of dirty blocks (tests/dirty.py), one workspace reused; a captured graph replayed twice;
  5. `metrics.compare_ap`, `ResidentSweep.compare_ap`, the refused arguments;
  6. `ModelHandler.score(compare=)` and `run.py --score --compare` with `compare_ap` on and off."""
import contextlib
import functools
import glob
import io
import random

import numpy as np
import pytest
import torch

from ggad_amd import synth
import dirty as D
import paired_bootstrap_ref as PR
import rank_wide_ref as RW

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL = -7.0
B = 64
SEED = 0x9E3779B97F4A7C15
CAP = PR.MAX_POS
SOME = (0, 1, 62, 63)                                   # the replicates the reference makes of `dgraph_like`


def _lib():
    from ggad_amd import _lib
    return _lib, _lib.load()


def _rand(rng, n, p):
    y = np.zeros(n, dtype=np.uint8)
    y[rng.choice(n, p, replace=False)] = 1
    return rng.random(n).astype(np.float32), y


def _signed_zeros(s):
    s = s.copy()
    s[::5] = np.float32(-0.0)
    s[1::5] = np.float32(0.0)
    return s


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (scores of A, scores of B, labels)."""
    rng = np.random.default_rng(78)
    f32 = np.float32
    out = {"p2n2": (np.array([0.1, 0.9, 0.4, 0.6], dtype=f32), np.array([0.8, 0.2, 0.3, 0.7], dtype=f32), np.array([1, 0, 1, 0], dtype=np.uint8))}
    s, y = _rand(rng, 1504, 501)                                                  # 501 and 1,003 draws: both last calls half used
    out["odd_odd"] = (s, rng.random(1504).astype(f32), y)
    s, y = _rand(rng, 1800, 300)
    out["identical"] = (s, s.copy(), y)
    out["reversed"] = (s, -s, y)
    out["separated_vs_above"] = ((s + y).astype(f32), (s - y).astype(f32), y)     # A: bin 0 only; B: bin P only
    s, y = _rand(rng, 700, 123)
    out["ties_all_equal"] = (np.full(700, 0.5, dtype=f32), s, y)
    s, y = _rand(rng, 2900, 400)
    t = rng.random(2900)
    out["ties_quantised"] = (_signed_zeros((np.floor(s * 64) / 64 - 0.5).astype(f32)), _signed_zeros((np.floor(t * 16) / 16 - 0.25).astype(f32)), y)
    s, y = _rand(rng, 400, 40)
    s = s.copy()
    s[np.flatnonzero(y == 1)[7]] = f32(2.0)                                       # under A the top positive alone above every negative
    out["top_alone"] = (s, rng.random(400).astype(f32), y)
    s, y = _rand(rng, CAP + 2500, CAP)
    out["at_boot_cap"] = (s, rng.random(len(s)).astype(f32), y)
    s, y = _rand(rng, 200000, 1000)                                               # threads loop over the draws; 256 blocks of several chunks
    out["n200k"] = (s, (0.5 * s + 0.5 * rng.random(200000)).astype(f32), y)
    y = np.zeros(200000, dtype=np.uint8)
    y[:1000] = 1                                                                  # the first block holds no negative, the second is mixed
    out["clustered"] = (out["n200k"][0], out["n200k"][1], y)
    _, s, y, _ = next(c for c in RW.cases() if c[0] == "dgraph_like")
    out["dgraph_like"] = (s, (s + 0.3 * rng.standard_normal(len(s))).astype(f32), y)
    return out


NAMES = list(_cases())


@functools.lru_cache(maxsize=None)
def _ref(name, seed=SEED, reps=B):
    sa, sb, y = _cases()[name]
    return PR.bootstrap(sa, sb, y, seed, reps, which=SOME if name == "dgraph_like" else None)


class Device:
    """One pair of lists on the device, uploaded once."""

    def __init__(self, sa, sb, y):
        self.n = len(y)
        self.a, self.b, self.y = (torch.tensor(np.asarray(v)).to(DEV) for v in (sa, sb, y))

    def wide(self, pos_cap, thres=0.5):
        """out8 of `ggad_rank_wide_f32` for either list, float64[2, 8]."""
        L, lib = _lib()
        got = []
        for s in (self.a, self.b):
            ws = torch.full((int(lib.ggad_rank_wide_workspace_elems(self.n, pos_cap)),), -1, dtype=torch.int32, device=DEV)
            out8 = torch.full((8,), FILL, dtype=torch.float64, device=DEV)
            L.call("ggad_rank_wide_f32", L.ptr(s), L.ptr(self.y), self.n, pos_cap, float(thres), L.ptr(out8), L.ptr(ws))
            got.append(out8.cpu().numpy())
        return np.stack(got)

    def pair(self, pos_cap, seed=SEED, reps=B, thres=0.5, hist=True, ws=None):
        """(out24, rep_ap[2, reps], rep_num[2, reps], hist int32[reps, 2, 3, pos_cap + 1] or None) as host arrays."""
        L, lib = _lib()
        need = int(lib.ggad_rank_bootstrap_pair_workspace_elems(self.n, pos_cap))
        assert need > 0
        if ws is None:
            ws = torch.full((need,), -1, dtype=torch.int32, device=DEV)            # (dirty on purpose)
        assert ws.numel() >= need
        out24 = torch.full((24,), FILL, dtype=torch.float64, device=DEV)
        ap = torch.full((2, reps), FILL, dtype=torch.float64, device=DEV)
        num = torch.full((2, reps), -1, dtype=torch.int64, device=DEV)
        h = torch.full((reps, 2, 3, pos_cap + 1), -1, dtype=torch.int32, device=DEV) if hist else None
        L.call("ggad_rank_bootstrap_pair_f32", L.ptr(self.a), L.ptr(self.b), L.ptr(self.y), self.n, pos_cap, float(thres), seed, reps,
               L.ptr(out24), L.ptr(ap), L.ptr(num), L.ptr(h), L.ptr(ws))
        return out24.cpu().numpy(), ap.cpu().numpy(), num.cpu().numpy(), None if h is None else h.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _device(name):
    return Device(*_cases()[name])


def _bits(*arrays):
    return np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.int64) if a.dtype.itemsize == 8 else
                           np.ascontiguousarray(a).reshape(-1).astype(np.int64) for a in arrays if a is not None])


def _check(tag, got, ref, out8, reps=B, which=None):
    o, ap, num, hist = got
    P, Nn = ref["P"], ref["Nn"]
    which = list(range(reps)) if which is None else list(which)
    worst = float(np.abs(ap[:, which] - ref["ap"][:, which]).max())
    print(f"[{tag}] P {P} Nn {Nn} status {o[23]:.0f}; worst |AP* - reference| {worst:.3e} against the bound {(P + 4) * 2.0 ** -53:.3e}; "
          f"AP*_A - AP*_B in [{(ap[0] - ap[1]).min()!r}, {(ap[0] - ap[1]).max()!r}]")
    np.testing.assert_array_equal(o[:16].view(np.int64), out8.reshape(-1).view(np.int64), err_msg=tag)
    assert o[16:].tolist() == [float(reps), float(P), float(Nn), 0.0, 0.0, 0.0, 0.0, 0.0], (tag, o[16:].tolist())
    if hist is not None:
        np.testing.assert_array_equal(hist[which][..., :P + 1], ref["hist"][which], err_msg=tag)
        assert (hist[..., P + 1:] == 0).all(), tag
        assert (hist[:, :, 0].sum(axis=-1) == P).all() and (hist[:, :, 1].sum(axis=-1) == Nn).all(), tag      # every replicate
    np.testing.assert_array_equal(num[:, which], ref["num"][:, which], err_msg=tag)
    assert worst <= (P + 4) * 2.0 ** -53, tag
    assert np.isfinite(ap).all() and (num >= 0).all() and (num <= 2 * P * Nn).all(), tag


# ------------------------------------------------------------------ 1: every case
@pytest.mark.parametrize("name", NAMES)
def test_every_case(name):
    sa, sb, y = _cases()[name]
    P = int(y.sum())
    Nn = len(y) - P
    d = _device(name)
    ref = _ref(name)
    got = d.pair(P)
    _check(name, got, ref, d.wide(P), which=SOME if name == "dgraph_like" else None)
    o, ap, num, hist = got
    if name == "p2n2":
        assert o[0] != o[8]                                                        # the two models order the four elements differently
    if name == "identical":
        assert (ap[0] == ap[1]).all() and (num[0] == num[1]).all() and (hist[:, 0] == hist[:, 1]).all()
    if name == "reversed":
        assert (num[0] + num[1] == 2 * P * Nn).all() and not (hist[:, 0] == hist[:, 1]).all()
    if name == "ties_all_equal":
        assert (num[0] == P * Nn).all() and np.abs(ap[0] - P / (P + Nn)).max() <= 4 * 2.0 ** -53
        assert (hist[:, 0, 0, 0] == P).all()                                       # the one run of equal positives is counted at its first rank
    if name == "ties_quantised":
        assert (hist[:, :, 2].sum(axis=-1) > 0).all() and (sa == 0).any() and np.signbit(sa[sa == 0]).any() and np.signbit(sb[sb == 0]).any()
    if name == "separated_vs_above":
        assert (ap[0] == 1.0).all() and (num[0] == 2 * P * Nn).all() and (hist[:, 0, 1, 0] == Nn).all()
        assert (num[1] == 0).all() and (hist[:, 1, 1, P] == Nn).all()
    if name == "top_alone":
        undrawn = ref["hist"][:, 0, 0, P - 1] == 0
        assert undrawn.any() and (ref["hist"][:, 0, 1, P] == 0).all()                # 0 / 0 in A's replicates: the select
    if name == "odd_odd":
        assert P % 2 == 1 and Nn % 2 == 1
    if name == "clustered":
        assert y[:1000].all() and not y[1000:].any()
    if name in ("at_boot_cap", "n200k", "clustered"):                              # a looser cap: other grids and LDS, the same bits
        again = d.pair(P + 700, hist=False)
        np.testing.assert_array_equal(_bits(*again[:3]), _bits(*got[:3]))


# ------------------------------------------------------------------ 2: statuses and refusals
def test_statuses():
    rng = np.random.default_rng(10)
    nan = float("nan")
    s, y = _rand(rng, 3000, 500)
    t = rng.random(3000).astype(np.float32)
    bad = t.copy()
    bad[11] = nan
    y2 = y.copy()
    y2[5] = 2
    one = np.zeros_like(y)
    one[77] = 1
    for dd, cap, status in ((Device(s, bad, y), 500, 3), (Device(bad, t, y), 500, 3), (Device(s, t, y2), 3000, 4),
                            (Device(s, t, np.zeros_like(y)), 3000, 1), (Device(s, t, np.ones_like(y)), 3000, 1), (Device(s, t, y), 499, 2),
                            (Device(s, t, one), 1, 8), (Device(s, t, 1 - one), 3000, 8)):
        o, ap, num, hist = dd.pair(cap)
        assert o[23] == float(status) == float(PR.status_of(dd.a.cpu().numpy(), dd.b.cpu().numpy(), dd.y.cpu().numpy(), cap)), (status, o)
        assert np.isnan(ap).all() and ap.shape == (2, B) and (num == 0).all() and (hist == 0).all()
        assert o[16:19].tolist() == [float(B), o[6], o[3] + o[5]] and o[19:23].tolist() == [0.0] * 4
        np.testing.assert_array_equal(o[:16].view(np.int64), dd.wide(cap).reshape(-1).view(np.int64))
    d = Device(s, bad, y)                                                          # NaN in B only: A's report stands, B's carries the status
    o = d.pair(500, hist=False)[0]
    assert o[7] == 0.0 and o[15] == 3.0 and o[23] == 3.0
    s, y = _rand(rng, CAP + 1 + 2500, CAP + 1)                                     # the cap plus one
    d = Device(s, rng.random(len(s)).astype(np.float32), y)
    o, ap, num, _ = d.pair(CAP + 1, hist=False)
    np.testing.assert_array_equal(o[:16].view(np.int64), d.wide(CAP + 1).reshape(-1).view(np.int64))
    assert o[7] == o[15] == 0.0 and o[23] == float(PR.TOO_MANY) == 9.0 and o[17] == CAP + 1 and np.isnan(ap).all() and (num == 0).all()
    from ggad_amd.metrics import compare_ap
    for kw in ({}, {"pos_cap": CAP + 1}, {"pos_cap": CAP + 500}):
        with pytest.raises(ValueError, match=rf"{CAP + 1} positives are more than ggad_rank_bootstrap_max_pos\(\) = {CAP}"):
            compare_ap(d.a, d.b, d.y, reps=8, **kw)
    with pytest.raises(ValueError, match="pos_cap = 100"):
        compare_ap(d.a, d.b, d.y, reps=8, pos_cap=100)


def test_refused_without_a_launch():
    L, lib = _lib()
    d = _device("odd_odd")
    p = L.ptr
    out = torch.full((24,), FILL, dtype=torch.float64, device=DEV)
    ap = torch.full((2 * B,), FILL, dtype=torch.float64, device=DEV)
    num = torch.full((2 * B,), -1, dtype=torch.int64, device=DEV)
    ws = torch.full((int(lib.ggad_rank_bootstrap_pair_workspace_elems(d.n, 501)) + 4,), -1, dtype=torch.int32, device=DEV)
    assert lib.ggad_rank_bootstrap_pair_workspace_elems(d.n, 0) == 0 and lib.ggad_rank_bootstrap_pair_workspace_elems(-1, 5) == 0
    assert lib.ggad_rank_bootstrap_pair_workspace_elems(2 ** 31, 5) == 0
    assert lib.ggad_rank_bootstrap_pair_workspace_elems(d.n, int(lib.ggad_rank_wide_max_pos()) + 1) == 0
    call = lib.ggad_rank_bootstrap_pair_f32
    good = dict(a=p(d.a), b=p(d.b), y=p(d.y), n=d.n, cap=501, reps=B, o=p(out), ap=p(ap), num=p(num), ws=p(ws))
    for change in (dict(cap=0), dict(cap=int(lib.ggad_rank_wide_max_pos()) + 1), dict(reps=0), dict(reps=-3), dict(reps=4097), dict(o=0),
                   dict(ap=0), dict(num=0), dict(ws=0), dict(ws=p(ws) + 4), dict(a=0), dict(b=0), dict(y=0), dict(n=2 ** 31), dict(n=-1)):
        g = dict(good, **change)
        assert call(g["a"], g["b"], g["y"], g["n"], g["cap"], 0.5, SEED, g["reps"], g["o"], g["ap"], g["num"], None, g["ws"], None) == -1, change
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all() and (ap.cpu().numpy() == FILL).all() and bool((num == -1).all()) and bool((ws == -1).all())


# ------------------------------------------------------------------ 3: replicate counts and seeds
def test_one_replicate_and_the_most():
    name = "top_alone"
    sa, sb, y = _cases()[name]
    d = _device(name)
    P = int(y.sum())
    out8 = d.wide(P)
    _check(f"{name}/B=1", d.pair(P, reps=1), PR.bootstrap(sa, sb, y, SEED, 1), out8, reps=1)
    most = d.pair(P, reps=4096)
    _check(f"{name}/B=4096", most, PR.bootstrap(sa, sb, y, SEED, 4096), out8, reps=4096)
    few = d.pair(P)
    np.testing.assert_array_equal(_bits(*few[1:]), _bits(most[1][:, :B], most[2][:, :B], most[3][:B]))       # a replicate depends on r alone


def test_seeds():
    d = _device("odd_odd")
    P = int(_cases()["odd_odd"][2].sum())
    a, b = d.pair(P), d.pair(P)
    np.testing.assert_array_equal(_bits(*a), _bits(*b))
    for seed in (SEED + 1, SEED ^ (1 << 32), 0, (1 << 64) - 1):                     # the low word, the high word, the ends
        c = d.pair(P, seed=seed)
        np.testing.assert_array_equal(c[0].view(np.int64), a[0].view(np.int64))     # the point estimates do not depend on it
        assert not np.array_equal(c[3][:, :, 0], a[3][:, :, 0]) and not np.array_equal(c[3][:, :, 1], a[3][:, :, 1]) and not np.array_equal(c[1], a[1])
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
    order = ("at_boot_cap", "ties_quantised", "p2n2")
    caps = {n: int(_cases()[n][2].sum()) for n in order}
    need = max(int(lib.ggad_rank_bootstrap_pair_workspace_elems(_device(n).n, caps[n])) for n in order)
    wblock, shared = D.int_like(need, D.NAN_BITS)
    for k in range(2):
        for name in order:
            d, cap = _device(name), caps[name]
            clean = d.pair(cap)
            blocks = [_carve(24, D.NAN_BITS, torch.float64), _carve(2 * B, D.NAN_BITS, torch.float64), _carve(2 * B, D.NAN_BITS, torch.int64),
                      _carve(B * 6 * (cap + 1), D.NAN_BITS, torch.int32)]
            o, ap, num, h = (t for _, t in blocks)
            L.call("ggad_rank_bootstrap_pair_f32", L.ptr(d.a), L.ptr(d.b), L.ptr(d.y), d.n, cap, 0.5, SEED, B, L.ptr(o), L.ptr(ap), L.ptr(num),
                   L.ptr(h), L.ptr(shared))
            D.dirty_lines()
            got = (o.cpu().numpy(), ap.cpu().numpy(), num.cpu().numpy(), h.cpu().numpy())
            np.testing.assert_array_equal(_bits(*got), _bits(*clean), err_msg=f"{name} round {k}")
            for block, _ in blocks:
                _guards_hold(block, D.NAN_BITS)
            _guards_hold(wblock, D.NAN_BITS)


def test_captured_and_replayed_twice():
    L, lib = _lib()
    name = "ties_quantised"
    d = _device(name)
    cap = int(_cases()[name][2].sum())
    eager = d.pair(cap)
    ws = torch.empty(int(lib.ggad_rank_bootstrap_pair_workspace_elems(d.n, cap)), dtype=torch.int32, device=DEV)
    out24 = torch.zeros(24, dtype=torch.float64, device=DEV)
    ap, num = torch.zeros((2, B), dtype=torch.float64, device=DEV), torch.zeros((2, B), dtype=torch.int64, device=DEV)
    hist = torch.zeros((B, 2, 3, cap + 1), dtype=torch.int32, device=DEV)
    sa, sb = d.a.clone(), d.b.clone()

    def call():
        L.call("ggad_rank_bootstrap_pair_f32", L.ptr(sa), L.ptr(sb), L.ptr(d.y), d.n, cap, 0.5, SEED, B, L.ptr(out24), L.ptr(ap), L.ptr(num),
               L.ptr(hist), L.ptr(ws))
    call()                                                                         # (the LDS opt-in happens outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        for t in (out24, ap):
            t.fill_(FILL)
        num.fill_(-1), hist.fill_(-1), ws.fill_(-1)
        graph.replay()
        got = (out24.cpu().numpy(), ap.cpu().numpy(), num.cpu().numpy(), hist.cpu().numpy())
        np.testing.assert_array_equal(_bits(*got), _bits(*eager))
    sa.copy_(d.b), sb.copy_(d.a)                                                   # the replay reads the new scores: the models swapped
    graph.replay()
    got = (out24.cpu().numpy(), ap.cpu().numpy(), num.cpu().numpy(), hist.cpu().numpy())
    np.testing.assert_array_equal(_bits(got[0][8:16], got[0][:8], got[0][16:], got[1][::-1], got[2][::-1], got[3][:, ::-1]), _bits(*eager))
    assert not np.array_equal(got[2], eager[2])


# ------------------------------------------------------------------ 5: the public calls
def _agrees(c, ref, level, tag):
    d_ap, d_auc = ref["ap"][0] - ref["ap"][1], ref["auc"][0] - ref["auc"][1]
    lo, hi, se = PR.summary(d_ap, level)
    alo, ahi, ase = PR.summary(d_auc, level)
    for got, want, what in ((c.diff_lo, lo, "diff_lo"), (c.diff_hi, hi, "diff_hi"), (c.diff_se, se, "diff_se"), (c.p, PR.p_value(d_ap), "p"),
                            (c.auc_diff_lo, alo, "auc_diff_lo"), (c.auc_diff_hi, ahi, "auc_diff_hi"), (c.auc_diff_se, ase, "auc_diff_se")):
        assert abs(got - want) <= 1e-12, (tag, what, got, want)


@pytest.mark.parametrize("name", ["ties_quantised", "n200k"])
def test_compare_ap_against_the_reference(name):
    from ggad_amd.metrics import ApComparison, compare_ap, format_compare_ap, rank_report_wide
    sa, sb, y = _cases()[name]
    d = _device(name)
    P = int(y.sum())
    ref = _ref(name)
    pa, pb = rank_report_wide(d.a, d.y, 0.5, pos_cap=P), rank_report_wide(d.b, d.y, 0.5, pos_cap=P)
    for pos_cap in (None, P):
        for level in (0.95, 0.5):
            c = compare_ap(d.a, d.b, d.y, level, reps=B, seed=SEED, pos_cap=pos_cap)
            assert isinstance(c, ApComparison) and (c.n_pos, c.n_neg, c.level, c.reps, c.seed) == (P, len(y) - P, level, B, SEED)
            assert (c.ap_a, c.ap_b, c.auc_a, c.auc_b) == (pa["ap"], pb["ap"], pa["auc"], pb["auc"]) and not c.identical
            assert c.diff == pa["ap"] - pb["ap"] and c.auc_diff == pa["auc"] - pb["auc"] and c.diff_lo <= c.diff_hi and 0.0 < c.p <= 1.0
            assert np.abs(c.diff_reps - (ref["ap"][0] - ref["ap"][1])).max() <= 2 * (P + 4) * 2.0 ** -53
            assert np.array_equal(c.auc_diff_reps, (ref["num"][0] - ref["num"][1]) / float(2 * P * (len(y) - P)))
            _agrees(c, ref, level, name)
            assert c.diff_reps.dtype == c.auc_diff_reps.dtype == np.float64 and len(c.diff_reps) == len(c.auc_diff_reps) == B
    assert c == compare_ap(d.a, d.b, d.y, 0.5, reps=B, seed=SEED, pos_cap=P) and c != compare_ap(d.a, d.b, d.y, 0.5, reps=B, seed=SEED + 1, pos_cap=P)
    assert format_compare_ap(c) == (f"[compare_ap] AP A {c.ap_a!r} B {c.ap_b!r} diff {c.diff!r} ± {c.diff_se!r} (50%: [{c.diff_lo!r}, {c.diff_hi!r}]) "
                                    f"p {c.p!r} AUROC diff {c.auc_diff!r} (50%: [{c.auc_diff_lo!r}, {c.auc_diff_hi!r}]) from {B} paired stratified "
                                    f"replicates, seed {SEED}, on {P} positives, {len(y) - P} negatives")
    same = compare_ap(d.a, d.a.clone(), d.y, reps=B, seed=SEED)
    assert same.identical and same.p == 1.0 and same.diff == same.auc_diff == same.diff_lo == same.diff_hi == same.diff_se == 0.0
    assert not same.diff_reps.any() and not same.auc_diff_reps.any()
    one = compare_ap(d.a, d.b, d.y, reps=1, seed=SEED, pos_cap=P)                  # one replicate: no spread to speak of
    assert np.isnan(one.diff_se) and one.diff_lo == one.diff_hi == one.diff_reps[0]
    default = compare_ap(d.a, d.b, d.y)
    assert (default.reps, default.seed, default.level) == (1000, 0, 0.95) and default.diff_lo < default.diff_hi


def test_compare_ap_refuses():
    from ggad_amd.metrics import compare_ap
    d = _device("odd_odd")
    sa, sb, y = _cases()["odd_odd"]
    bad = sb.copy()
    bad[5] = np.nan
    y2 = y.copy()
    y2[5] = 3
    for args, text in (((d.a, torch.tensor(bad).to(DEV), d.y), "NaN"), ((torch.tensor(bad).to(DEV), d.b, d.y), "NaN"),
                       ((d.a, d.b, torch.tensor(y2).to(DEV)), "neither 0 nor 1"), ((d.a, d.b, torch.zeros_like(d.y)), "Only one class"),
                       ((d.a, d.b, torch.ones_like(d.y)), "Only one class")):
        with pytest.raises(ValueError, match=text):
            compare_ap(*args, reps=4)
    for args in ((d.a.cpu(), d.b, d.y), (d.a, d.b.cpu(), d.y), (d.a, d.b, d.y.cpu()), (d.a.double(), d.b, d.y), (d.a, d.b.double(), d.y),
                 (d.a, d.b, d.y.int()), (d.a, d.b[:-1], d.y), (d.a[:-1], d.b, d.y), (d.a.view(-1, 1), d.b.view(-1, 1), d.y.view(-1, 1))):
        with pytest.raises(ValueError, match="compare_ap takes"):
            compare_ap(*args, reps=4)
    for level in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="level"):
            compare_ap(d.a, d.b, d.y, level, reps=4)
    for reps in (0, -1, 4097, 2.5):
        with pytest.raises(ValueError, match=r"reps = .* is outside 1..ggad_rank_bootstrap_max_reps\(\) = 4096"):
            compare_ap(d.a, d.b, d.y, reps=reps)
    for seed in (-1, 1 << 64, 0.5):
        with pytest.raises(ValueError, match="seed"):
            compare_ap(d.a, d.b, d.y, reps=4, seed=seed)
    with pytest.raises(ValueError, match="pos_cap = 500"):
        compare_ap(d.a, d.b, d.y, reps=4, pos_cap=500)
    with pytest.raises(ValueError, match="pos_cap"):
        compare_ap(d.a, d.b, d.y, reps=4, pos_cap=0)
    one = np.zeros_like(y)
    one[3] = 1
    for lab in (one, 1 - one):
        with pytest.raises(ValueError, match="needs at least two positives and two negatives"):
            compare_ap(d.a, d.b, torch.tensor(lab).to(DEV), reps=4)


N_NODES = 3000


def test_resident_sweep_compare_ap():
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
    scores = sweep.scores().clone()
    other = torch.from_numpy(rng.random(len(cases)).astype(np.float32)).to(DEV)
    c = sweep.compare_ap(other, level=0.9, reps=B, seed=11)
    assert sweep.n_pos == 700 and (c.n_pos, c.n_neg, c.reps, c.seed, c.level) == (700, 5300, B, 11, 0.9)
    assert c == metrics.compare_ap(scores, other, sweep.labels, 0.9, B, 11, pos_cap=700) == sweep.compare_ap(other, scores, 0.9, B, 11)
    ref = PR.bootstrap(scores.cpu().numpy(), other.cpu().numpy(), lab, 11, B, keep_hist=False)
    assert np.array_equal(c.auc_diff_reps, (ref["num"][0] - ref["num"][1]) / float(2 * 700 * 5300))
    assert np.abs(c.diff_reps - (ref["ap"][0] - ref["ap"][1])).max() <= 2 * 704 * 2.0 ** -53
    _agrees(c, ref, 0.9, "sweep")
    assert sweep.compare_ap(scores, scores).identical
    with pytest.raises(ValueError, match="without labels"):
        ResidentSweep(model, cases, None, 150).compare_ap(other)


# ------------------------------------------------------------------ 6: the handler and run.py
def _masked(out):
    """A handler run's stdout without what differs between two identical runs: wall-clock times and the time-stamped checkpoint path."""
    import re
    return [re.sub(r"time: [-+0-9.e]+s", "time: *", ln) for ln in out.splitlines() if not ln.startswith(("total_time is", "Model path:"))]


def test_model_handler_compare_ap_on_and_off(tmp_path, capsys):
    from ggad_amd import metrics
    from ggad_amd.model_handler import ModelHandler
    n = 30000
    rowptr, col = synth.make_graph(n, 300000, 3, kind="powerlaw", max_degree=200)
    feat = synth.make_features(n, 17, 3)
    lab = synth.make_labels(n, 0.05, 3)
    rowptr, col, feat = synth.plant_anomalies(rowptr, col, feat, lab, 3, scale=0.25, rewire=0.5)

    def config(tag, cache=True, **extra):
        return dict(data_name="synthetic", data_dir="", data=((rowptr, col), feat, lab), seed=72, model="GCN", multi_relation="GNN",
                    emb_size=64, thres=0.4, lr=0.005, weight_decay=0.007, batch_size=60, num_epochs=2, valid_epochs=1, num_batches=6,
                    n_pseudo=20, save_dir=str(tmp_path / tag) + "/", test_ratio=0.67, device=0, eval_cache=cache, **extra)
    ckpt = {}
    for tag, seed in (("a", 72), ("b", 73)):                                       # (`b`: the same split, other initial weights)
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        ModelHandler(config(tag)).train()
        ckpt[tag] = glob.glob(str(tmp_path / tag / "*" / "*.pkl"))[0]
    on = dict(compare_ap=0.9, boot_reps=64, boot_seed=5)
    outs = {}
    for tag, cfg in (("without", config("s")), ("off", config("s", compare_ap=0, boot_reps=64, boot_seed=5)), ("on", config("s", **on)),
                     ("on_plain", config("s", cache=False, **on)), ("without_plain", config("s", cache=False))):
        capsys.readouterr()
        h = ModelHandler(cfg)
        scores, _ = h.score(ckpt["a"], compare=ckpt["b"])
        outs[tag] = dict(h=h, out=capsys.readouterr().out, scores=scores.clone())
    for tag in ("without", "off", "without_plain"):
        assert "[compare_ap]" not in outs[tag]["out"] and outs[tag]["h"].ap_comparison is None
    assert _masked(outs["off"]["out"]) == _masked(outs["without"]["out"])         # the key at 0: a run without it
    scores_b, _ = ModelHandler(config("s")).score(ckpt["b"])
    capsys.readouterr()
    y = np.asarray(outs["on"]["h"].dataset["y_test"]).reshape(-1)
    y8 = torch.from_numpy(y.astype(np.uint8)).to(DEV)
    c = metrics.compare_ap(outs["on"]["scores"], scores_b, y8, 0.9, 64, 5, pos_cap=int(y.sum()))
    for tag, base in (("on", "without"), ("on_plain", "without_plain")):
        lines, plain = _masked(outs[tag]["out"]), _masked(outs[base]["out"])
        assert outs[tag]["out"].count("[compare_ap]") == 1 and lines[-1] == metrics.format_compare_ap(c) and "(90%: [" in lines[-1]
        assert lines[-2].startswith("[compare] AUROC A ") and lines[:-1] == plain      # behind `[compare]`, which is byte-equal
        assert outs[tag]["h"].ap_comparison == c and not c.identical and outs[tag]["h"].auc_comparison == outs[base]["h"].auc_comparison
    ref = PR.bootstrap(outs["on"]["scores"].cpu().numpy(), scores_b.cpu().numpy(), y, 5, 64, keep_hist=False)
    assert np.array_equal(c.auc_diff_reps, (ref["num"][0] - ref["num"][1]) / float(2 * c.n_pos * c.n_neg))
    _agrees(c, ref, 0.9, "handler")
    h = ModelHandler(config("s", **on))
    h.score(ckpt["a"], compare=ckpt["a"])                                          # a checkpoint with itself
    assert h.ap_comparison.identical and " diff 0.0 ± 0.0 (90%: [0.0, 0.0]) p 1.0 AUROC diff 0.0 " in capsys.readouterr().out.splitlines()[-1]
    h.score(ckpt["a"])                                                             # no compare: no line
    assert "[compare_ap]" not in capsys.readouterr().out
    with pytest.raises(ValueError, match="needs `model: 'GCN'`"):
        ModelHandler(dict(config("s", cache=False, **on), model="SAGE"))
    with pytest.raises(ValueError, match="confidence level"):
        ModelHandler(config("s", compare_ap=1.5))


def test_run_py_compare_ap(tmp_path, capsys):
    import run
    a_pt, b_pt = str(tmp_path / "a.pt"), str(tmp_path / "b.pt")
    base = ["--synthetic", "--dataset", "reddit", "--quiet"]
    assert run.main(base + ["--num_epoch", "4", "--save", a_pt]) is None
    assert run.main(base + ["--num_epoch", "4", "--seed", "1", "--save", b_pt]) is None
    capsys.readouterr()
    scores_a = run.main(base + ["--score", a_pt, "--compare", b_pt, "--compare_ap", "0.9", "--boot_reps", "64", "--boot_seed", "3"])
    out = capsys.readouterr().out
    scores_off = run.main(base + ["--score", a_pt, "--compare", b_pt])
    out_off = capsys.readouterr().out
    assert np.array_equal(scores_a, scores_off) and "[compare_ap]" not in out_off
    lines = out.splitlines()
    assert out.count("[compare_ap]") == 1 and lines[-1].startswith("[compare_ap] AP A ") and lines[-2].startswith("[compare] AUROC A ")
    assert lines[:-1] == out_off.splitlines()                                      # the `[compare]` line byte-equal, nothing else moved
    args = run.parse(base)
    random.seed(args.seed), np.random.seed(args.seed), torch.manual_seed(args.seed)
    with contextlib.redirect_stdout(io.StringIO()):
        g = run.load_graph(args)
    y = np.asarray(g.ano_label).reshape(-1)
    idx = np.asarray(g.idx_test, dtype=np.int64)
    from ggad_amd.fullgraph_script import load_checkpoint, prepare
    from ggad_amd.metrics import compare_ap, format_compare_ap
    from ggad_amd.model import Model
    dev = torch.device("cuda", 0)
    full, feats, ft_size = prepare(args, g.adj, g.feat, dev)
    model = Model(ft_size, args.embedding_dim, "prelu", args.negsamp_ratio, args.readout).to(dev)
    model.load_state_dict(load_checkpoint(b_pt, ft_size, args.embedding_dim)["state_dict"], strict=True)
    model.eval()
    scores_b = model.score(feats, full).detach().float().cpu().numpy()
    P = int(y[idx].sum())
    c = compare_ap(torch.from_numpy(scores_a[idx]).to(DEV), torch.from_numpy(scores_b[idx]).to(DEV),
                   torch.from_numpy(y[idx].astype(np.uint8)).to(DEV), 0.9, 64, 3, pos_cap=P)
    assert lines[-1] == format_compare_ap(c) and f"from 64 paired stratified replicates, seed 3, on {P} positives" in lines[-1]
    ref = PR.bootstrap(scores_a[idx], scores_b[idx], y[idx], 3, 64, keep_hist=False)
    assert np.array_equal(c.auc_diff_reps, (ref["num"][0] - ref["num"][1]) / float(2 * c.n_pos * c.n_neg))
    _agrees(c, ref, 0.9, "run.py")
    for argv in (["--compare_ap"], ["--score", a_pt, "--compare_ap"], ["--score", a_pt, "--compare", b_pt, "--compare_ap", "1.5"],
                 ["--score", a_pt, "--compare", b_pt, "--boot_reps", "10"], ["--score", a_pt, "--compare", b_pt, "--compare_ap", "--boot_reps", "0"]):
        with pytest.raises(SystemExit):
            run.parse(base + argv)
    capsys.readouterr()
