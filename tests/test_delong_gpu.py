"""DeLong's variance and the paired test on the device: `ggad_rank_delong_f32` / `ggad_rank_delong_pair_f32` (csrc/rank_metrics.hip),
`metrics.auc_ci` / `compare_auc`, `ResidentSweep.auc_ci` / `.compare`, config key `auc_ci`, `score(compare=)` and `run.py --auc_ci
--compare`.  Every native call runs on a workspace full of -1 and outputs full of -7.

  1. every case of tests/rank_wide_ref.py, single call, against tests/delong_ref.py: out16[0:8] holds the bits of `ggad_rank_wide_f32`'s
     out8; all ten limb words equal the reference's integers; the status is equal (`lone_negative`: 6; `all_tied`: 0 with a variance of
     exactly 0.0); out16[8..11] are within 1e-14 relative of the float of the exact Fraction (each term is one exactly-integer numerator
     converted once over a denominator of at most five float64 multiplications, one division, then one addition of non-negatives: fewer
     than ten roundings of 1.1e-16 and no cancellation).  `dgraph_like` is where m S2 passes 64 bits;
  2. `beyond_64`: 2^20 positives and 2^22 negatives, where S2 alone is 66 bits: both limbs of every sum;
  3. pairs on p8193, p16385, five_tiles, heavy_ties, quantised, signed_zero, infinity (and the wide lists of the same names) and
     dgraph_like, with B = A + noise, -A, A quantised to 1/8, A itself (status 7) and `near` (A with the values of one positive and one
     negative exchanged): all twenty limb words, out24[0:16] against two wide calls, [16..21] within 1e-14 (the signed `cov` and `diff`
     relative to the larger of their two terms).  For `near` the float64 composition var_a + var_b - 2 cov of the REFERENCE's own
     values misses var_diff by more than 1e-14: what the numerators ND10 / ND01 are for;
  4. one workspace reused across five_tiles -> p8193 -> tiny, twice, for both calls: bit-equal to fresh workspaces; both calls captured
     behind `ResidentSweep.scores()` and replayed after the weights changed;
  5. the status codes and the refused arguments;
  6. `metrics.auc_ci` / `compare_auc` and the `ResidentSweep` methods;
  7. `ModelHandler.train()` with `auc_ci` on and off, `score(compare=)`;
  8. `run.py --score a.pt --auc_ci 0.9 --compare b.pt`."""
import contextlib
import functools
import glob
import io
import math
import random
from statistics import NormalDist

import numpy as np
import pytest
import torch

from ggad_amd import synth
import delong_ref as DL
import operating_point_ref as OP
import rank_wide_ref as RW

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = [c[0] for c in RW.cases()]
FILL = -7.0
REL = 1e-14


def _lib():
    from ggad_amd import _lib
    return _lib, _lib.load()


def _case(name):
    return next(c for c in RW.cases() if c[0] == name)


class Device:
    """Labels and one or two score lists of one input on the device, uploaded once."""

    def __init__(self, s, y, sb=None):
        self.n = len(s)
        self.s, self.y = torch.tensor(np.asarray(s)).to(DEV), torch.tensor(np.asarray(y)).to(DEV)
        self.sb = None if sb is None else torch.tensor(np.asarray(sb)).to(DEV)

    def wide(self, pos_cap, thres, b=False):
        L, lib = _lib()
        ws = torch.full((int(lib.ggad_rank_wide_workspace_elems(self.n, pos_cap)),), -1, dtype=torch.int32, device=DEV)
        out8 = torch.full((8,), FILL, dtype=torch.float64, device=DEV)
        L.call("ggad_rank_wide_f32", L.ptr(self.sb if b else self.s), L.ptr(self.y), self.n, pos_cap, float(thres), L.ptr(out8), L.ptr(ws))
        return out8.cpu().numpy()

    def single(self, pos_cap, thres=0.5, ws=None):
        """(out16, sums) as host arrays."""
        L, lib = _lib()
        need = int(lib.ggad_rank_delong_workspace_elems(self.n, pos_cap))
        assert need > 0
        if ws is None:
            ws = torch.full((need,), -1, dtype=torch.int32, device=DEV)            # (dirty on purpose)
        assert ws.numel() >= need
        out16 = torch.full((16,), FILL, dtype=torch.float64, device=DEV)
        sums = torch.full((12,), -1, dtype=torch.int64, device=DEV)
        L.call("ggad_rank_delong_f32", L.ptr(self.s), L.ptr(self.y), self.n, pos_cap, float(thres), L.ptr(out16), L.ptr(sums), L.ptr(ws))
        return out16.cpu().numpy(), sums.cpu().numpy()

    def pair(self, pos_cap, thres=0.5, ws=None):
        """(out24, sums) as host arrays."""
        L, lib = _lib()
        need = int(lib.ggad_rank_delong_pair_workspace_elems(self.n, pos_cap))
        assert need > 0
        if ws is None:
            ws = torch.full((need,), -1, dtype=torch.int32, device=DEV)
        assert ws.numel() >= need
        out24 = torch.full((24,), FILL, dtype=torch.float64, device=DEV)
        sums = torch.full((24,), -1, dtype=torch.int64, device=DEV)
        L.call("ggad_rank_delong_pair_f32", L.ptr(self.s), L.ptr(self.sb), L.ptr(self.y), self.n, pos_cap, float(thres), L.ptr(out24),
               L.ptr(sums), L.ptr(ws))
        return out24.cpu().numpy(), sums.cpu().numpy()


def _close(got, want, scale=None):
    """|got - want| <= 1e-14 of `scale` (default: the wanted value's own magnitude)."""
    want = float(want)
    return abs(float(got) - want) <= REL * abs(want if scale is None else float(scale))


def _check_single(tag, o, sums, ref, out8):
    print(f"[{tag}] status {o[15]:.0f} (reference {ref['status']}) var {o[8]!r} = {o[9]!r} + {o[10]!r} se {o[11]!r} "
          f"(reference var {None if ref['var'] is None else float(ref['var'])!r}) sums {sums.tolist()}")
    np.testing.assert_array_equal(o[:8].view(np.int64), out8.view(np.int64), err_msg=tag)
    assert int(o[15]) == ref["status"] and float(o[15]).is_integer(), tag
    assert sums.tolist() == ref["sums"], tag
    if ref["status"] in (1, 2, 3, 4):
        assert o[7] == o[15] and np.isnan(o[8:15]).all(), tag
        return
    assert o[7] == 0.0 and (o[12:15] == 0.0).all(), tag
    if ref["status"] == 6:
        assert np.isnan(o[8:12]).all(), tag
        return
    want = [float(ref["var"]), float(ref["v10"]), float(ref["v01"]), math.sqrt(float(ref["var"]))]
    for j, w in enumerate(want):
        assert _close(o[8 + j], w), (tag, j, o[8 + j], w)
    if ref["var"] == 0:
        assert (o[8:12] == 0.0).all(), tag


# ------------------------------------------------------------------ 1: every case of the wide chain
@functools.lru_cache(maxsize=None)
def _single_ref(name):
    _, s, y, _ = _case(name)
    return DL.single(s, y)


@pytest.mark.parametrize("name", NAMES)
def test_every_case_single(name):
    _, s, y, thres = _case(name)
    P = int(y.sum())
    d = Device(s, y)
    o, sums = d.single(P, thres)
    ref = _single_ref(name)
    _check_single(name, o, sums, ref, d.wide(P, thres))
    if name.startswith("lone_negative"):
        assert o[15] == 6.0
    if name.startswith("all_tied"):
        assert o[15] == 0.0 and o[8] == 0.0 and o[11] == 0.0 and ref["N10"] == ref["N01"] == 0
    if name == "dgraph_like":
        assert (ref["m"] * ref["S2"]).bit_length() > 64 and ref["N10"].bit_length() > 64   # a 64-bit accumulator fails here
        assert sums[7] != 0                                                        # the high limb of N10
    if P > 1:                                                                      # a looser cap: other grids, the same integers
        o2, sums2 = d.single(min(len(s), P + 5000, 1 << 20), thres)
        assert sums2.tolist() == sums.tolist() and np.array_equal(o2[8:].view(np.int64), o[8:].view(np.int64))


# ------------------------------------------------------------------ 2: sums beyond 64 bits
def test_beyond_64_bits():
    import time
    rng = np.random.default_rng(64)
    y = np.zeros((1 << 20) + (1 << 22), dtype=np.uint8)
    y[rng.choice(len(y), 1 << 20, replace=False)] = 1
    s = (rng.standard_normal(len(y)) + y).astype(np.float32)
    t0 = time.time()
    ref = DL.single(s, y)
    took = time.time() - t0
    print(f"[beyond_64] the reference took {took:.2f} s; S2 has {ref['S2'].bit_length()} bits, m S2 {(ref['m'] * ref['S2']).bit_length()}")
    assert took < 5.0
    assert ref["S2"].bit_length() > 64 and ref["status"] == 0
    d = Device(s, y)
    o, sums = d.single(1 << 20)
    _check_single("beyond_64", o, sums, ref, d.wide(1 << 20, 0.5))
    assert sums[3] != 0 and sums[7] != 0 and sums[9] != 0                           # the high limbs of S2, N10, N01 (T2 ends at 64 bits)


# ------------------------------------------------------------------ 3: pairs
PAIR_CASES = ("p8193", "p16385", "five_tiles", "heavy_ties", "quantised", "signed_zero", "infinity", "dgraph_like",
              "heavy_ties_wide", "signed_zero_wide", "infinity_wide")
VARIANTS = ("noise", "negated", "eighths", "itself", "near")
# `near`: the seed that picks the positive and the negative whose values are exchanged, chosen on the CPU (the first of 0, 1, 2, ...
# at which the reference shows var_diff > 0 and the float64 composition more than 1e-14 off; the test asserts both)
NEAR_SEED = {"p8193": 0, "p16385": 0, "five_tiles": 0, "heavy_ties": 0, "quantised": 0, "signed_zero": 2, "infinity": 2, "dgraph_like": 0,
             "heavy_ties_wide": 0, "signed_zero_wide": 0, "infinity_wide": 0}


def second_list(name, variant, s, y, seed=None):
    if variant == "noise":
        with np.errstate(invalid="ignore"):
            return (s + np.float32(0.5) * np.random.default_rng(31).standard_normal(len(s)).astype(np.float32)).astype(np.float32)
    if variant == "negated":
        return -s
    if variant == "eighths":
        return (np.floor(s.astype(np.float64) * 8) / 8).astype(np.float32)
    if variant == "itself":
        return s.copy()
    rng = np.random.default_rng(NEAR_SEED[name] if seed is None else seed)
    i, j = int(rng.choice(np.flatnonzero(y == 1))), int(rng.choice(np.flatnonzero(y == 0)))
    b = s.copy()
    b[i], b[j] = s[j], s[i]
    return b


def composition_error(ref):
    """How far the float64 composition var_a + var_b - 2 cov of the reference's own values is from var_diff, relative."""
    composed = float(ref["var_a"]) + float(ref["var_b"]) - 2.0 * float(ref["cov"])
    return abs(composed - float(ref["var_diff"])) / float(ref["var_diff"])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", PAIR_CASES)
def test_pairs(name, variant):
    _, s, y, thres = _case(name)
    sb = second_list(name, variant, s, y)
    assert not np.isnan(sb).any()
    P = int(y.sum())
    ref = DL.pair(s, sb, y)
    d = Device(s, y, sb)
    o, sums = d.pair(P, thres)
    print(f"[{name}/{variant}] status {o[23]:.0f} (reference {ref['status']}) out24[16:22] {o[16:22].tolist()} sums {sums.tolist()}")
    np.testing.assert_array_equal(o[:8].view(np.int64), d.wide(P, thres).view(np.int64))
    np.testing.assert_array_equal(o[8:16].view(np.int64), d.wide(P, thres, b=True).view(np.int64))
    assert sums.tolist() == ref["sums"]
    assert int(o[23]) == ref["status"] and o[22] == 0.0
    same = variant == "itself" or (variant == "eighths" and name.startswith("heavy_ties"))     # (fifths stay distinct in eighths: the same
    assert ref["status"] == (7 if same else 0)                                               # placements, found from the integers)
    va, vb, vd = float(ref["var_a"]), float(ref["var_b"]), float(ref["var_diff"])
    assert _close(o[16], va) and _close(o[17], vb) and _close(o[19], vd)
    assert _close(o[18], ref["cov"], max(abs(ref["cov10"]), abs(ref["cov01"])))
    theta_a, theta_b = o[0], o[8]
    assert _close(o[20], ref["diff"], max(abs(theta_a), abs(theta_b)))
    if same:
        assert np.isnan(o[21]) and o[19] == 0.0 and o[20] == 0.0 and o[18] == o[16] == o[17]
        return
    assert vd > 0 and _close(o[21], float(ref["diff"]) / math.sqrt(vd))
    if variant == "near":
        err = composition_error(ref)
        print(f"[{name}/near] var_diff {vd!r}; var_a + var_b - 2 cov in float64 is {err:.3e} relative off")
        assert err > REL                                                            # the case has not gone soft


# ------------------------------------------------------------------ 4: a reused workspace, a captured graph
def test_one_workspace_reused_shows_nothing_stale():
    _, lib = _lib()
    order = ("five_tiles", "p8193", "tiny")
    devs, caps, thres = {}, {}, {}
    for name in order:
        _, s, y, thres[name] = _case(name)
        devs[name], caps[name] = Device(s, y, second_list(name, "noise", s, y)), int(y.sum())
    need = max(int(lib.ggad_rank_delong_pair_workspace_elems(devs[n].n, caps[n])) for n in order)
    shared = torch.full((need,), -1, dtype=torch.int32, device=DEV)
    for _ in range(2):
        for name in order:
            for call in (devs[name].single, devs[name].pair):
                fresh = call(caps[name], thres[name])
                again = call(caps[name], thres[name], ws=shared)
                np.testing.assert_array_equal(again[0].view(np.int64), fresh[0].view(np.int64), err_msg=name)
                np.testing.assert_array_equal(again[1], fresh[1], err_msg=name)
            assert fresh[0][23] == (6.0 if name == "tiny" else 0.0)


N_NODES = 3000


@pytest.fixture(scope="module")
def small_graph():
    rowptr, col = synth.make_graph(N_NODES, 30000, 3, kind="powerlaw", max_degree=200)
    rng = np.random.default_rng(8)
    cases = rng.integers(0, N_NODES, 12000).astype(np.int64)
    lab = np.zeros(len(cases), dtype=np.int64)
    lab[rng.choice(len(cases), 9000, replace=False)] = 1                           # two tiles of positives
    return rowptr, col, cases, lab


def _model(small_graph, f, d, seed=0):
    from ggad_amd.dgraph import normalize_features
    from ggad_amd.graph import DeviceGraph
    from ggad_amd.graphsage import GCN, FeatureTable, GCNAggregator, GCNEncoder
    rowptr, col = small_graph[:2]
    torch.manual_seed(seed)
    graph = DeviceGraph(rowptr, col, DEV)
    feat = normalize_features(synth.make_features(N_NODES, f, 3)).astype(np.float32)
    features = FeatureTable(torch.from_numpy(feat))
    enc = GCNEncoder(features, f, d, graph, GCNAggregator(features, cuda=True), gcn=True, cuda=True)
    model = GCN(2, enc)
    enc.engine.sync_params()
    return model


def _perturb(eng, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        eng.params[:eng.n_train] += 0.05 * torch.randn(eng.n_train, generator=g).to(eng.params.device)
    eng.sync_params()


def test_resident_sweep_methods_and_replay(small_graph):
    from ggad_amd import metrics
    from ggad_amd.eval_cache import ResidentSweep
    L, lib = _lib()
    _, _, cases, lab = small_graph
    model = _model(small_graph, 17, 64)
    eng = model.enc.engine
    _perturb(eng, 2)
    sweep = ResidentSweep(model, cases, lab, 150)
    other = sweep.scores().clone()                                                 # a second model's scores of the same list
    _perturb(eng, 5)
    scores = sweep.scores()
    ci = sweep.auc_ci(0.9)
    assert sweep.n_pos == 9000
    assert ci == metrics.auc_ci(scores, sweep.labels, 0.9, pos_cap=9000) == sweep.auc_ci(0.9, scores=scores)
    cmp = sweep.compare(other)
    assert cmp == metrics.compare_auc(scores, other, sweep.labels, pos_cap=9000) == sweep.compare(other, scores=scores)
    ref = DL.pair(scores.cpu().numpy(), other.cpu().numpy(), lab)
    assert ref["status"] == 0 and _close(ci.var, ref["var_a"]) and _close(cmp.var_diff, ref["var_diff"]) and not cmp.identical
    assert (ci.n_pos, ci.n_neg, cmp.n_pos, cmp.n_neg) == (9000, 3000, 9000, 3000)
    for method in ("auc_ci", "compare"):
        with pytest.raises(ValueError, match="without labels"):
            getattr(ResidentSweep(model, cases, None, 150), method)(*(() if method == "auc_ci" else (other,)))
    # scores() plus both calls as one graph, replayed after the weights changed
    pos_cap = 9000
    ws1 = torch.empty(int(lib.ggad_rank_delong_workspace_elems(sweep.n, pos_cap)), dtype=torch.int32, device=DEV)
    ws2 = torch.empty(int(lib.ggad_rank_delong_pair_workspace_elems(sweep.n, pos_cap)), dtype=torch.int32, device=DEV)
    out16, out24 = torch.zeros(16, dtype=torch.float64, device=DEV), torch.zeros(24, dtype=torch.float64, device=DEV)
    sums1, sums2 = torch.zeros(12, dtype=torch.int64, device=DEV), torch.zeros(24, dtype=torch.int64, device=DEV)

    def both(probs, o16, s12, w1, o24, s24, w2):
        L.call("ggad_rank_delong_f32", L.ptr(probs), L.ptr(sweep.labels), sweep.n, pos_cap, 0.5, L.ptr(o16), L.ptr(s12), L.ptr(w1))
        L.call("ggad_rank_delong_pair_f32", L.ptr(probs), L.ptr(other), L.ptr(sweep.labels), sweep.n, pos_cap, 0.5, L.ptr(o24), L.ptr(s24),
               L.ptr(w2))

    def eager():
        o16, o24 = torch.full_like(out16, FILL), torch.full_like(out24, FILL)
        s12, s24 = torch.full_like(sums1, -1), torch.full_like(sums2, -1)
        both(sweep.scores(), o16, s12, torch.full_like(ws1, -1), o24, s24, torch.full_like(ws2, -1))
        return np.concatenate([o16.cpu().numpy().view(np.int64), s12.cpu().numpy(), o24.cpu().numpy().view(np.int64), s24.cpu().numpy()])

    def replayed():
        return np.concatenate([out16.cpu().numpy().view(np.int64), sums1.cpu().numpy(), out24.cpu().numpy().view(np.int64), sums2.cpu().numpy()])
    first = eager()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both(sweep.scores(), out16, sums1, ws1, out24, sums2, ws2)
    graph.replay()
    np.testing.assert_array_equal(replayed(), first)
    assert out16[15].item() == 0.0 and out16[6].item() == 9000.0 and out24[23].item() == 0.0
    seen = [first]
    for seed in (3, 4):
        _perturb(eng, seed)
        graph.replay()
        got = replayed()
        np.testing.assert_array_equal(got, eager())
        assert not any(np.array_equal(got, s) for s in seen)                       # the replay saw the new weights
        seen.append(got)


# ------------------------------------------------------------------ 5: status
def test_status_codes_and_refused_arguments():
    L, lib = _lib()
    _, s, y, thres = _case("p8193")
    nan_s = s.copy()
    nan_s[333] = np.nan
    y2 = y.copy()
    y2[77] = 2

    def refused_single(d, pos_cap, status):
        o, sums = d.single(pos_cap, thres)
        assert o[15] == o[7] == float(status) and np.isnan(o[8:15]).all() and (sums == 0).all()
        np.testing.assert_array_equal(o[:8].view(np.int64), d.wide(pos_cap, thres).view(np.int64))

    def refused_pair(d, pos_cap, status):
        o, sums = d.pair(pos_cap, thres)
        assert o[23] == float(status) and np.isnan(o[16:23]).all() and (sums == 0).all()
        np.testing.assert_array_equal(o[:8].view(np.int64), d.wide(pos_cap, thres).view(np.int64))
        np.testing.assert_array_equal(o[8:16].view(np.int64), d.wide(pos_cap, thres, b=True).view(np.int64))
        return o
    refused_single(Device(nan_s, y), 8193, 3)
    o = refused_pair(Device(nan_s, y, s), 8193, 3)                                  # NaN in A only
    assert o[7] == 3.0 and o[15] == 0.0
    o = refused_pair(Device(s, y, nan_s), 8193, 3)                                  # NaN in B only
    assert o[7] == 0.0 and o[15] == 3.0
    refused_single(Device(s, y2), 8193, 4)
    refused_pair(Device(s, y2, -s), 8193, 4)
    for const in (0, 1):
        yc = np.full(len(s), const, dtype=np.uint8)
        refused_single(Device(s, yc), len(s), 1)
        refused_pair(Device(s, yc, -s), len(s), 1)
    refused_single(Device(s, y), 8192, 2)                                           # P = pos_cap + 1
    o = refused_pair(Device(s, y, -s), 8192, 2)
    assert int(o[6]) == int(o[14]) == 8193
    # fewer than two of a class: status 6, the AUROC words and the sums valid
    rng = np.random.default_rng(6)
    for p in (1, 4999):
        y6 = np.zeros(5000, dtype=np.uint8)
        y6[rng.choice(5000, p, replace=False)] = 1
        s6 = rng.random(5000).astype(np.float32)
        d = Device(s6, y6, -s6)
        o, sums = d.single(p)
        ref = DL.single(s6, y6)
        assert ref["status"] == 6
        _check_single(f"status6_p{p}", o, sums, ref, d.wide(p, 0.5))
        o, sums = d.pair(p)
        pref = DL.pair(s6, -s6, y6)
        assert o[23] == 6.0 == pref["status"] and np.isnan(o[16:22]).all() and o[22] == 0.0 and sums.tolist() == pref["sums"]
        assert o[7] == o[15] == 0.0 and o[0] == float(ref["auc"]) and o[8] == float(DL.single(-s6, y6)["auc"])
    # refused without a launch: nothing is touched
    d = Device(s, y, -s)
    out = torch.full((24,), FILL, dtype=torch.float64, device=DEV)
    sums = torch.full((24,), -1, dtype=torch.int64, device=DEV)
    ws = torch.full((int(lib.ggad_rank_delong_pair_workspace_elems(len(s), 8193)) + 4,), -1, dtype=torch.int32, device=DEV)
    p = L.ptr
    assert p(ws) % 16 == 0
    one, two = lib.ggad_rank_delong_f32, lib.ggad_rank_delong_pair_f32
    for pos_cap, o_, s_, w in ((0, p(out), p(sums), p(ws)), (int(lib.ggad_rank_wide_max_pos()) + 1, p(out), p(sums), p(ws)),
                               (8193, 0, p(sums), p(ws)), (8193, p(out), 0, p(ws)), (8193, p(out), p(sums), 0),
                               (8193, p(out), p(sums), p(ws) + 4)):
        assert one(p(d.s), p(d.y), len(s), pos_cap, 0.5, o_, s_, w, None) == -1
        assert two(p(d.s), p(d.sb), p(d.y), len(s), pos_cap, 0.5, o_, s_, w, None) == -1
    assert two(p(d.s), 0, p(d.y), len(s), 8193, 0.5, p(out), p(sums), p(ws), None) == -1
    assert one(p(d.s), p(d.y), 2 ** 31, 8193, 0.5, p(out), p(sums), p(ws), None) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all() and bool((sums == -1).all()) and bool((ws == -1).all())


# ------------------------------------------------------------------ 6: the public calls
SEPARABLE = OP.separable_cases()


@pytest.mark.parametrize("name", ["sep_p8193", "sep_q64_p600"])
def test_public_calls_against_the_reference(name):
    from ggad_amd.metrics import AucComparison, AucInterval, auc_ci, binary_report, compare_auc
    _, s, y = next(c for c in SEPARABLE if c[0] == name)
    sb = second_list(name, "noise", s, y)
    d = Device(s, y, sb)
    ref, pref = DL.single(s, y), DL.pair(s, sb, y)
    P = int(y.sum())
    for pos_cap in (None, P):
        for level in (0.95, 0.5):
            ci = auc_ci(d.s, d.y, level, pos_cap=pos_cap)
            assert isinstance(ci, AucInterval) and ci.status_ok and (ci.n_pos, ci.n_neg, ci.level) == (P, len(y) - P, level)
            assert ci.auc == float(ref["auc"]) and _close(ci.var, ref["var"]) and _close(ci.se, math.sqrt(float(ref["var"])))
            q = NormalDist().inv_cdf(0.5 + level / 2)
            assert ci.lo == max(0.0, ci.auc - q * ci.se) and ci.hi == min(1.0, ci.auc + q * ci.se) and ci.lo < ci.auc < ci.hi
        b = binary_report(d.s, d.y, 0.5)
        assert list(ci.report) == list(b) and all(ci.report[k] == b[k] for k in ("tp", "fp", "fn", "tn", "f1_macro", "gmean"))
        c = compare_auc(d.s, d.sb, d.y, pos_cap=pos_cap)
        assert isinstance(c, AucComparison) and not c.identical and (c.n_pos, c.n_neg) == (P, len(y) - P)
        assert c.auc_a == ci.auc and c.auc_b == float(DL.single(sb, y)["auc"])
        assert _close(c.var_a, pref["var_a"]) and _close(c.var_b, pref["var_b"]) and _close(c.var_diff, pref["var_diff"])
        assert _close(c.cov, pref["cov"], max(abs(pref["cov10"]), abs(pref["cov01"]))) and _close(c.diff, pref["diff"], max(c.auc_a, c.auc_b))
        assert _close(c.z, float(pref["diff"]) / math.sqrt(float(pref["var_diff"]))) and c.p == math.erfc(abs(c.z) / 2 ** 0.5)
        same = compare_auc(d.s, d.s, d.y, pos_cap=pos_cap)
        assert same.identical and same.z == 0.0 and same.p == 1.0 and same.diff == 0.0 and same.var_diff == 0.0 and same.var_a == ci.var


def test_public_calls_refuse():
    from ggad_amd.metrics import auc_ci, compare_auc
    _, s, y, _ = _case("p8193")
    d = Device(s, y)
    bad = s.copy()
    bad[5] = np.nan
    bad = torch.tensor(bad).to(DEV)
    y2 = y.copy()
    y2[5] = 3
    for args, text in (((bad, d.y), "NaN"), ((d.s, torch.tensor(y2).to(DEV)), "neither 0 nor 1"), ((d.s, torch.zeros_like(d.y)), "Only one class"),
                       ((d.s, torch.ones_like(d.y)), "Only one class")):
        with pytest.raises(ValueError, match=text):
            auc_ci(*args)
        with pytest.raises(ValueError, match=text):
            compare_auc(args[0], d.s, args[1])
    with pytest.raises(ValueError, match="NaN"):
        compare_auc(d.s, bad, d.y)
    for call in (lambda **kw: auc_ci(d.s, d.y, **kw), lambda **kw: compare_auc(d.s, d.s, d.y, **kw)):
        with pytest.raises(ValueError, match="pos_cap = 8192"):
            call(pos_cap=8192)
        with pytest.raises(ValueError, match="pos_cap"):
            call(pos_cap=0)
    for name in ("lone_positive", "lone_negative_wide"):
        _, s1, y1, _ = _case(name)
        d1 = Device(s1, y1)
        with pytest.raises(ValueError, match="needs at least two positives and two negatives"):
            auc_ci(d1.s, d1.y)
        with pytest.raises(ValueError, match="needs at least two positives and two negatives"):
            compare_auc(d1.s, d1.s, d1.y)
    with pytest.raises(ValueError, match="level"):
        auc_ci(d.s, d.y, 1.0)


# ------------------------------------------------------------------ 7: the handler
def test_model_handler_with_auc_ci_on_and_off(tmp_path, capsys):
    from ggad_amd import metrics
    from ggad_amd.model_handler import ModelHandler
    n = 30000
    rowptr, col = synth.make_graph(n, 300000, 3, kind="powerlaw", max_degree=200)
    feat = synth.make_features(n, 17, 3)
    lab = synth.make_labels(n, 0.05, 3)
    rowptr, col, feat = synth.plant_anomalies(rowptr, col, feat, lab, 3, scale=0.25, rewire=0.5)
    runs = {}
    for tag, level, cache, seed in (("off", 0, True, 72), ("on", 0.95, True, 72), ("on_plain", 0.95, False, 72), ("other", 0, True, 73)):
        cfg = dict(data_name="synthetic", data_dir="", data=((rowptr, col), feat, lab), seed=72, model="GCN", multi_relation="GNN",
                   emb_size=64, thres=0.4, lr=0.005, weight_decay=0.007, batch_size=60, num_epochs=2, valid_epochs=1, num_batches=6,
                   n_pseudo=20, save_dir=str(tmp_path / tag) + "/", test_ratio=0.67, device=0, eval_cache=cache)
        if level:
            cfg["auc_ci"] = level
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)                                                    # (`other`: the same split, other initial weights)
        capsys.readouterr()
        h = ModelHandler(cfg)
        res = h.train()
        out = capsys.readouterr().out
        ckpts = glob.glob(str(tmp_path / tag / "*" / "*.pkl"))
        assert len(ckpts) == 1
        runs[tag] = dict(h=h, cfg=cfg, res=res, out=out, ckpt=ckpts[0], losses=np.stack(h.epoch_losses), end=h.end_state)
    off, on, plain, other = runs["off"], runs["on"], runs["on_plain"], runs["other"]
    assert "[auc_ci]" not in off["out"] and "[compare]" not in off["out"] and off["h"].auc_interval is None
    for r in (on, plain):
        np.testing.assert_array_equal(off["losses"].view(np.int64), r["losses"].view(np.int64))
        assert list(off["end"]) == list(r["end"]) and all(torch.equal(off["end"][k], r["end"][k]) for k in off["end"])
        assert r["res"] == off["res"] and r["out"].count("[auc_ci]") == 1 and "[compare]" not in r["out"]
        assert r["out"].splitlines()[-1].startswith("[auc_ci]")                     # behind the closing sweep's report
        gnn = [ln for ln in off["out"].splitlines() if ln.startswith("   GNN ")]
        assert len(gnn) == 6 and [ln for ln in r["out"].splitlines() if ln.startswith("   GNN ")] == gnn
    h = on["h"]
    sweep = h.eval_sweeps[1]
    scores = sweep.scores()
    ci = metrics.auc_ci(scores, sweep.labels, 0.95, pos_cap=sweep.n_pos)
    assert h.auc_interval == ci == plain["h"].auc_interval
    line = next(ln for ln in on["out"].splitlines() if ln.startswith("[auc_ci]"))
    assert line == (f"[auc_ci] AUROC {ci.auc!r} ± {ci.se!r} (95%: [{ci.lo!r}, {ci.hi!r}]) on {ci.n_pos} positives, {ci.n_neg} negatives")
    ref = DL.single(scores.cpu().numpy(), np.asarray(h.dataset["y_test"]))
    assert ci.auc == float(ref["auc"]) and _close(ci.var, ref["var"]) and ci.n_pos == ref["m"]
    # score(): the line again; compare= a second checkpoint, and a checkpoint with itself
    for cfg in (on["cfg"], plain["cfg"]):
        capsys.readouterr()
        h2 = ModelHandler(cfg)
        got_scores, _ = h2.score(on["ckpt"], compare=other["ckpt"])
        out2 = capsys.readouterr().out
        assert torch.equal(got_scores, scores) and h2.metrics == on["res"] and h2.auc_interval == ci
        assert [ln for ln in out2.splitlines() if ln.startswith("[auc_ci]")] == [line]
        h3 = ModelHandler(off["cfg"])
        scores_b, _ = h3.score(other["ckpt"])
        capsys.readouterr()
        c = metrics.compare_auc(scores, scores_b, sweep.labels, pos_cap=sweep.n_pos)
        assert h2.auc_comparison == c and not c.identical
        assert [ln for ln in out2.splitlines() if ln.startswith("[compare]")] == [
            f"[compare] AUROC A {c.auc_a!r} B {c.auc_b!r} diff {c.diff!r} z {c.z!r} p {c.p!r}"]
    h4 = ModelHandler(off["cfg"])
    h4.score(on["ckpt"], compare=on["ckpt"])
    out4 = capsys.readouterr().out
    assert "[auc_ci]" not in out4 and h4.auc_comparison.identical
    assert next(ln for ln in out4.splitlines() if ln.startswith("[compare]")).endswith("diff 0.0 z 0.0 p 1.0")
    capsys.readouterr()
    h5 = ModelHandler(off["cfg"])                                                  # key off, no compare: score() is today's
    h5.score(on["ckpt"])
    out5 = capsys.readouterr().out
    assert "[auc_ci]" not in out5 and "[compare]" not in out5 and h5.metrics == off["res"]
    with pytest.raises(ValueError, match="needs labels"):
        ModelHandler(off["cfg"]).score(on["ckpt"], ids=np.arange(100, dtype=np.int64), compare=on["ckpt"])


# ------------------------------------------------------------------ 8: run.py
def test_run_py_auc_ci_and_compare(tmp_path, capsys):
    import run
    a_pt, b_pt = str(tmp_path / "a.pt"), str(tmp_path / "b.pt")
    base = ["--synthetic", "--dataset", "reddit", "--quiet"]
    capsys.readouterr()
    assert run.main(base + ["--num_epoch", "4", "--save", a_pt]) is None
    out_a = capsys.readouterr().out
    assert run.main(base + ["--num_epoch", "4", "--seed", "1", "--save", b_pt, "--auc_ci"]) is None
    out_b = capsys.readouterr().out
    assert "[auc_ci]" not in out_a and "[compare]" not in out_a
    assert sum(ln.startswith("[auc_ci] AUROC ") and "(95%: [" in ln for ln in out_b.splitlines()) == 1
    scores_a = run.main(base + ["--score", a_pt, "--auc_ci", "0.9", "--compare", b_pt])
    out = capsys.readouterr().out
    scores_plain = run.main(base + ["--score", a_pt])
    out_plain = capsys.readouterr().out
    assert "[auc_ci]" not in out_plain and "[compare]" not in out_plain and np.array_equal(scores_a, scores_plain)
    assert [ln for ln in out.splitlines() if not ln.startswith(("[auc_ci]", "[compare]"))] == out_plain.splitlines()
    # B's scores of the graph A was trained on: the graph follows from --seed, the weights from the file
    args = run.parse(base)
    random.seed(args.seed), np.random.seed(args.seed), torch.manual_seed(args.seed)
    with contextlib.redirect_stdout(io.StringIO()):
        g = run.load_graph(args)
    y = np.asarray(g.ano_label).reshape(-1)
    idx = np.asarray(g.idx_test, dtype=np.int64)
    ref = DL.single(scores_a[idx], y[idx])
    assert ref["status"] == 0
    auc, se = float(ref["auc"]), None
    line = next(ln for ln in out.splitlines() if ln.startswith("[auc_ci]"))
    head, _, tail = line.partition(" ± ")
    assert head == f"[auc_ci] AUROC {auc!r}" and tail.endswith(f") on {ref['m']} positives, {ref['n']} negatives")
    se = float(tail.split(" ")[0])
    assert _close(se, math.sqrt(float(ref["var"])))
    q = NormalDist().inv_cdf(0.95)
    assert tail == f"{se!r} (90%: [{max(0.0, auc - q * se)!r}, {min(1.0, auc + q * se)!r}]) on {ref['m']} positives, {ref['n']} negatives"
    # the [compare] line: B's scores are not returned, so the reference runs on what `metrics.compare_auc` is given by another route
    from ggad_amd.fullgraph_script import load_checkpoint, prepare
    from ggad_amd.model import Model
    dev = torch.device("cuda", 0)
    full, feats, ft_size = prepare(args, g.adj, g.feat, dev)
    model = Model(ft_size, args.embedding_dim, "prelu", args.negsamp_ratio, args.readout).to(dev)
    model.load_state_dict(load_checkpoint(b_pt, ft_size, args.embedding_dim)["state_dict"], strict=True)
    model.eval()
    scores_b = model.score(feats, full).detach().float().cpu().numpy()
    pref = DL.pair(scores_a[idx], scores_b[idx], y[idx])
    assert pref["status"] == 0
    words = next(ln for ln in out.splitlines() if ln.startswith("[compare]")).split(" ")
    assert words[:3] == ["[compare]", "AUROC", "A"] and [words[i] for i in (4, 6, 8, 10)] == ["B", "diff", "z", "p"]
    got = {k: float(words[i]) for k, i in (("a", 3), ("b", 5), ("diff", 7), ("z", 9), ("p", 11))}
    assert got["a"] == auc and got["b"] == float(DL.single(scores_b[idx], y[idx])["auc"])
    assert _close(got["diff"], pref["diff"], max(got["a"], got["b"]))
    assert _close(got["z"], float(pref["diff"]) / math.sqrt(float(pref["var_diff"]))) and got["p"] == math.erfc(abs(got["z"]) / 2 ** 0.5)
