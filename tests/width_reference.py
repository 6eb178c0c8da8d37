"""Shared inputs, float64 references and checks of tests/test_feature_widths_gpu.py and tests/test_feature_widths_cpu.py, and the
feature-width-generic step check of tests/test_wide_embed_gpu.py (not a test module itself).

Everything here is built once per session (`functools.lru_cache`) and must be left unchanged by its users.

  * `graph()`: power-law graph on 3,000 nodes plus three nodes added by hand (a pendant, a row of closed size exactly 16, one of
    exactly 17: one piece of 16 entries against two) and a few self-loops; no node of degree 0; one hub whose closed row has at
    least 480 entries = 30 pieces of 16: `k_combine1_reset` then runs its eight-in-flight loop (`c + 7 rpi < pieces`) at every
    F >= 16 (rpi = 64 / F <= 4).  Below F = 16 that loop needs up to 57 pieces (F = 1: rpi = 64, 7 * 64 + 1 = 449 pieces = 7,169
    entries) and what runs at those widths is its tail loop.
  * `feat(f)`: `synth.make_features`, column means removed (F > 1), rows scaled to unit L2 norm.  Row-sum scaling
    (`oracle.normalize_rows`) leaves a median |dW| of 3.7e-4 at F = 1, too close to the suite's 3e-6 absolute gradient term.
  * `batches()`: 48 rows (hub at label 0, second hub at label 1, pendant, the 16- and 17-entry rows, a self-loop row, one node
    twice with one label, one node once with each label, label-1 rows in the middle), 3 rows (1 + 2), 130 rows.
  * `aggs(f)`: per batch the float64 aggregate, the float32 one and the float64 aggregate of |feat| (the S of the error bounds).
"""
import functools

import numpy as np
import torch

from ggad_amd import synth
from oracle import ggad_oracle as O
import step_reference as R

U = 2.0 ** -24                       # unit round-off of fp32
N_BASE = 3000
PENDANT, ROW16, ROW17 = N_BASE, N_BASE + 1, N_BASE + 2
N_NODES = N_BASE + 3
SELF_LOOPS = (5, 77, 1234, 2999)
HUB_MIN = 480


# ------------------------------------------------------------------ the step check at any feature width
def split(x, d, f):
    return x[:d], x[d:d + d * f], x[d + d * f:d + d * f + d * d]


def check_step(eng, before, ref_g, what):
    """tests/step_reference.py::check_step with the engine's own feature width (the helper's is fixed at 17)."""
    p0, m0, v0, t0 = before
    d, f, nt = eng.D, eng.F, eng.n_train
    params = eng.params.cpu().numpy()
    R.check_moments(eng.exp_avg.cpu().numpy(), eng.exp_avg_sq.cpu().numpy(), *R.moment_bounds(ref_g, p0, m0, v0), what)
    p_ref, _, _ = O.adam_f64(p0, m0, v0, ref_g, t0 + 1, R.LR, R.WD)
    gp = ref_g + R.WD * p0
    for name, a, r, q, s in zip(("w", "W", "fc"), split(params[:nt].astype(np.float64), d, f), split(p_ref, d, f),
                                split(p0, d, f), split(gp, d, f)):
        diff = np.abs(a - r)
        sure = np.abs(s) > max(1e-6 * np.abs(s).max(), 1e-6)
        if sure.any():
            assert diff[sure].max() < 3e-6, f"{what}: {name} off by {diff[sure].max():.3e} after the Adam step"
        assert diff.max() <= 2.1 * np.abs(r - q).max() + 1e-12, f"{what}: {name} off by {diff.max():.3e} (more than one opposite step)"
    W = params[d:d + d * f].reshape(d, f)
    fc = params[d + d * f:nt].reshape(d, d)
    assert np.array_equal(params[nt:nt + f * d].reshape(f, d), W.T), f"{what}: Wt is not W^T"
    assert np.array_equal(params[nt + f * d:nt + f * d + d * d].reshape(d, d), fc.T), f"{what}: fcT is not fc^T"
    assert int(eng.step_counter.item()) == t0 + 1, what


# ------------------------------------------------------------------ shared inputs
@functools.lru_cache(maxsize=None)
def graph():
    import scipy.sparse as sp
    rowptr, col = synth.make_graph(N_BASE, 45000, 2, kind="powerlaw", max_degree=600)
    rng = np.random.default_rng(41)
    deg = np.diff(rowptr)
    quiet = np.flatnonzero(deg < 40)                                   # (keeps the hub and the second hub as they are)
    n16 = rng.choice(quiet, 15, replace=False)
    n17 = rng.choice(quiet, 16, replace=False)
    src = [np.repeat(np.arange(N_BASE), deg), [PENDANT], np.full(15, ROW16), np.full(16, ROW17), SELF_LOOPS]
    dst = [col, [0], n16, n17, SELF_LOOPS]
    r, c = np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)
    a = sp.csr_matrix((np.ones(2 * len(r), dtype=np.int8), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(N_NODES, N_NODES))
    a.sum_duplicates()
    a.sort_indices()
    rowptr, col = a.indptr.astype(np.int32), a.indices.astype(np.int32)
    deg = np.diff(rowptr)
    closed = closed_sizes(rowptr, col)
    assert deg.min() >= 1, "a node of degree 0"
    assert closed.max() >= HUB_MIN, f"largest closed row {closed.max()} < {HUB_MIN} entries"
    assert closed[PENDANT] == 2 and closed[ROW16] == 16 and closed[ROW17] == 17
    assert all(closed[v] == deg[v] for v in SELF_LOOPS)
    return rowptr, col


def closed_sizes(rowptr, col):
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    has_self = np.bincount(rows[col == rows], minlength=n) > 0
    return np.diff(rowptr) + 1 - has_self


@functools.lru_cache(maxsize=None)
def feat(f):
    x = synth.make_features(N_NODES, f, 9 + f).astype(np.float64)
    if f > 1:
        x = x - x.mean(0, keepdims=True)
    x = x / (np.sqrt((x * x).sum(1, keepdims=True)) + 1e-12)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def padded(x, fill=0.0, stride=32):
    """Rows of `stride` floats: the trainer's table for F <= 32."""
    out = np.full((x.shape[0], stride), fill, dtype=np.float32)
    out[:, :x.shape[1]] = x
    return out


@functools.lru_cache(maxsize=None)
def batches():
    rowptr, col = graph()
    closed = closed_sizes(rowptr, col)
    order = np.argsort(closed)
    hub, hub2 = int(order[-1]), int(order[-2])
    rng = np.random.default_rng(99)
    out = []
    nodes = rng.choice(N_BASE, 48, replace=False).astype(np.int64)
    lab = np.zeros(48, dtype=np.int64)
    lab[[5, 17, 18, 30]] = 1
    lab[40:] = 1
    nodes[2] = hub                                  # label 0
    nodes[18] = hub2                                # label 1: the second large row feeds the outlier generation
    nodes[9] = PENDANT
    nodes[10], nodes[41] = ROW16, ROW17             # one at each label
    nodes[11] = SELF_LOOPS[1]
    nodes[21] = nodes[20]                           # one node twice with the same label
    nodes[30] = nodes[12]                           # ... and one once with each label
    assert lab[20] == lab[21] and lab[30] != lab[12] and lab[2] == 0 and lab[18] == 1
    out.append(("mixed", nodes, lab))
    out.append(("three", rng.choice(N_BASE, 3, replace=False).astype(np.int64), np.array([0, 1, 1], dtype=np.int64)))
    nodes = rng.choice(N_NODES, 130, replace=False).astype(np.int64)
    lab = np.zeros(130, dtype=np.int64)
    lab[rng.choice(130, 30, replace=False)] = 1
    out.append(("big", nodes, lab))
    for _, nodes, lab in out:
        nodes.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def aggs(f):
    """Per batch: (float64 aggregate, float32 aggregate, float64 aggregate of |feat|)."""
    rowptr, col = graph()
    x = feat(f)
    return [(O.aggregate_batch(rowptr, col, x, nodes, True, dtype=np.float64), O.aggregate_batch(rowptr, col, x, nodes, True),
             O.aggregate_batch(rowptr, col, np.abs(x), nodes, True, dtype=np.float64)) for _, nodes, _ in batches()]


# ------------------------------------------------------------------ group 1: the plan's aggregates
def check_plan(ch, f, what):
    """Entries, counts and owners as tests/test_minibatch_gpu.py::_check_plan_against_oracle; x1 per row and x2 per owner element by
    element within the forward bound of an fp32 sum of products, |got - float64| <= (terms + 4) 2^-24 sum_j |w_j| |feat_j,f| (terms:
    entries of the row / degree of the owner; + 4: two square roots, the division, the final store).  Returns worst error / bound."""
    rowptr, col = graph()
    ent_ptr = ch.ent_ptr[:ch.n_rows + 1].cpu().numpy()
    etot = int(ent_ptr[-1])
    assert np.array_equal(ent_ptr, ch.ent_ptr_host)
    ent_col = ch.ent_col[:etot].cpu().numpy()
    ent_own = ch.ent_own[:etot].cpu().numpy()
    ent_c1 = ch.ent_c1[:etot].cpu().numpy()
    ent_row = ch.ent_row[:etot].cpu().numpy()
    assert np.array_equal(ent_row, np.repeat(np.arange(ch.n_rows), np.diff(ent_ptr)))
    x1 = ch.x1[:ch.n_rows * f].view(-1, f).cpu().numpy().astype(np.float64)
    x2 = ch.x2[:etot * f].view(-1, f).cpu().numpy().astype(np.float64)
    deg = np.diff(rowptr)
    worst = 0.0
    for b, ((shape, nodes, _), (a64, _, aabs)) in enumerate(zip(batches(), aggs(f))):
        r0, r1 = ch.batch_rows(b)
        assert np.array_equal(ent_ptr[r0:r1 + 1] - ent_ptr[r0], a64.ent_ptr), f"{what} {shape}: entry offsets"
        e0, e1 = ent_ptr[r0], ent_ptr[r1]
        assert np.array_equal(ent_col[e0:e1], a64.unique[a64.ent_pos]), f"{what} {shape}: entry columns"
        cnt = np.bincount(a64.ent_pos, minlength=len(a64.unique))
        assert np.array_equal(ent_c1[e0:e1], cnt[a64.ent_pos]), f"{what} {shape}: column counts"
        own = ent_own[e0:e1]
        assert (own >= e0).all() and (own < e1).all()
        assert np.array_equal(ent_col[own], ent_col[e0:e1])
        owners = np.unique(own)
        assert len(owners) == len(a64.unique) and (ent_own[owners] == owners).all(), f"{what} {shape}: owners"
        # x1: terms = entries of the row
        bound = (a64.r[:, None] + 4) * U * aabs.to_feats
        err = np.abs(x1[r0:r1] - a64.to_feats)
        assert np.isfinite(x1[r0:r1]).all(), f"{what} {shape}: x1 is not finite"
        ratio = (err / np.maximum(bound, 1e-300)).max()
        assert (err <= bound).all(), f"{what} {shape}: x1 off by {err.max():.3e}, {ratio:.2f} x bound"
        worst = max(worst, ratio)
        # x2: terms = degree of the owner's node; a node without neighbours gives NaN on both sides
        pos = np.searchsorted(a64.unique, ent_col[owners])
        ref, got = a64.to_feats_neigh[pos], x2[owners]
        assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what} {shape}: NaN rows of x2"
        ok = ~np.isnan(ref)
        bound = (deg[ent_col[owners]][:, None] + 4) * U * aabs.to_feats_neigh[pos]
        err = np.where(ok, np.abs(got - ref), 0.0)
        ratio = (err / np.maximum(np.where(ok, bound, 1.0), 1e-300)).max()
        assert (err <= np.where(ok, bound, 0.0)).all(), f"{what} {shape}: x2 off by {err.max():.3e}, {ratio:.2f} x bound"
        worst = max(worst, ratio)
    return worst


# ------------------------------------------------------------------ group 3: the step
# (F, D, chain): every narrow shape the module steps; (9, 32) and (25, 64) run on the 32-float padded table
STEP_CASES = [(65, 64, 0), (1, 64, 0), (16, 64, 0), (63, 64, 0), (64, 64, 0), (65, 64, 2), (128, 64, 0), (148, 64, 0), (296, 32, 0),
              (1024, 9, 0), (33, 33, 0), (70, 1, 0), (9, 32, 0), (9, 32, 2), (25, 64, 0)]
PADDED_STEP = {(9, 32), (25, 64)}


# (draw, gain) of the xavier_uniform parameters where draw 0 at gain 1 misses `check_step_conditions` on one of the batches (the
# inputs are chosen so that the conditions hold; the conditions are not fitted to the inputs).  At D = 1 fc is one scalar and a
# unit-gain draw leaves |dfc| below 5e-3 or the only channel dead: that case draws with gain 2.
PARAM_DRAW = {(1, 64): (4, 1.0), (63, 64): (2, 1.0), (128, 64): (2, 1.0), (1024, 9): (1, 1.0), (70, 1): (1, 2.0)}


def init_params(f, d):
    draw, gain = PARAM_DRAW.get((f, d), (0, 1.0))
    torch.manual_seed(500 + d + f + 1000 * draw)
    return (torch.nn.init.xavier_uniform_(torch.empty(1, d), gain=gain), torch.nn.init.xavier_uniform_(torch.empty(d, f), gain=gain),
            torch.nn.init.xavier_uniform_(torch.empty(d, d), gain=gain))


@functools.lru_cache(maxsize=None)
def step_reference(f, d):
    """Per batch: float64 losses and packed gradient, and the float32 oracle's (for the printed comparison)."""
    params = init_params(f, d)
    out = []
    for (_, _, lab), (a64, a32, _) in zip(batches(), aggs(f)):
        ref_loss, g = R.loss_and_grad64(a64, lab, params)
        p32 = O.MiniParams.leaves(*[np.asarray(t) for t in params])
        t32 = O.batch_loss(p32, a32, lab)
        t32[0].backward()
        l32 = np.array([t.item() for t in t32])
        g32 = np.concatenate([t.grad.numpy().reshape(-1) for t in p32.tensors()]).astype(np.float64)
        out.append((ref_loss, g, l32, g32))
    return out


def check_step_conditions(f, d):
    """What makes the step check of a case mean something, from the float64 reference alone: median |dW| >= 1e-3, max |g| of each
    tensor >= 5e-3, the share of every tensor the masked Adam rule holds to 3e-6 ("sure") >= 0.99 -- from fresh state and from the
    preloaded moments."""
    p0 = R.flat(*init_params(f, d))
    for (shape, _, _), (_, g, _, _) in zip(batches(), step_reference(f, d)):
        what = f"F={f} D={d} {shape}"
        gw, gW, gfc = split(g, d, f)
        assert np.median(np.abs(gW)) >= 1e-3, f"{what}: median |dW| {np.median(np.abs(gW)):.2e}"
        for name, t in (("w", gw), ("W", gW), ("fc", gfc)):
            assert np.abs(t).max() >= 5e-3, f"{what}: max |d{name}| {np.abs(t).max():.2e}"
        for name, s in zip(("w", "W", "fc"), split(g + R.WD * p0, d, f)):
            sure = np.abs(s) > max(1e-6 * np.abs(s).max(), 1e-6)
            assert sure.mean() >= 0.99, f"{what}: 'sure' share of {name} {sure.mean():.4f}"


# ------------------------------------------------------------------ group 2: ragged lists for ggad_seg_mean / ggad_seg_wsum
SEG_LENGTHS = (300, 0, 65, 1, 130, 64, 2, 128, 63)      # on the 64-entry block loop of gather_block and its four-way unroll


@functools.lru_cache(maxsize=None)
def seg_lists():
    """(seg_ptr, seg_col, seg_w) of one ragged list with rows of SEG_LENGTHS entries; ids repeat within a row; weights in [-1, 1]
    with exact zeros."""
    rng = np.random.default_rng(7)
    ptr = np.concatenate([[0], np.cumsum(SEG_LENGTHS)]).astype(np.int32)
    cols = []
    for n in SEG_LENGTHS:
        c = rng.integers(0, N_NODES, n)
        if n >= 2:
            c[n // 2] = c[0]                        # the same neighbour twice
        if n >= 64:
            c[rng.integers(0, n, n // 4)] = c[1]    # ... and many times
        cols.append(c)
    col = np.concatenate(cols).astype(np.int32)
    w = rng.uniform(-1.0, 1.0, len(col)).astype(np.float32)
    w[rng.random(len(col)) < 0.1] = 0.0
    for a in (ptr, col, w):
        a.setflags(write=False)
    return ptr, col, w


@functools.lru_cache(maxsize=None)
def seg_reference(f):
    """float64 mean and weighted sum per row with their bounds (r + 3) 2^-24 sum |w| |x|; the empty row is NaN with bound 0."""
    ptr, col, w = seg_lists()
    x = feat(f).astype(np.float64)
    n = len(SEG_LENGTHS)
    mean, wsum = np.zeros((n, f)), np.zeros((n, f))
    b_mean, b_wsum = np.zeros((n, f)), np.zeros((n, f))
    for i in range(n):
        e0, e1 = int(ptr[i]), int(ptr[i + 1])
        r = e1 - e0
        if r == 0:
            mean[i] = wsum[i] = np.nan
            continue
        rows = x[col[e0:e1]]
        ww = w[e0:e1].astype(np.float64)[:, None]
        mean[i] = rows.sum(0) / r
        wsum[i] = (ww * rows).sum(0)
        b_mean[i] = (r + 3) * U * np.abs(rows).sum(0) / r
        b_wsum[i] = (r + 3) * U * (np.abs(ww) * np.abs(rows)).sum(0)
    return mean, wsum, b_mean, b_wsum
