"""The XCD-resident chunk kernel (`k_train_chunk_xcd`, csrc/step_xcd.hip: every optimiser step of a chunk in one launch, the
default hot path) and the launch chain (csrc/step.hip) against a FLOAT64 reference -- the oracle with dtype=np.float64 plus
torch.optim.Adam's update restated in float64 (tests/step_reference.py) -- at the shapes where the kernels branch:

  run-time width (D not a multiple of 16, lanes >= D aliased)  D in {63, 48, 33, 17, 16, 8, 1}   test_teacher_forced_step[d*]
  odd D (scalar weight-load path)                               D in {63, 33, 17, 1}               test_teacher_forced_step[d*]
  hub rows (>= XHUB = 32 pieces, summed by the whole workgroup) a closed row of >= 600 entries      [*-hub-*]
  more than XPC pieces per virtual wave                         batches of > 10,000 entries       [*-large-*], nv 24 too
  more than XRA = 512 label-1 rows                              1,100 rows, 600 of label 1        [*-xra-*]
  rows not a multiple of 16, 3-row batch                        37 rows / 3 rows                  [*-ragged-*], [*-tiny-*]
  the same node twice, self-loops                               [*-dup-*]
  24 / 28 / 32 surviving workgroups (phase-E ownership)        test_teacher_forced_step[nv*]
  Adam bias correction from the step counter (k_xcd_prep)      every case: fresh, t = 1 and t = 10,000 with preloaded moments
  chunks of more than XBT = 256 batches                         test_trajectory_in_one_launch[260x12]

Teacher forcing: a chunk of ONE batch, so that the launch's step starts from known parameters and optimiser state; its loss-log
row, exp_avg / exp_avg_sq (through which the gradient is pinned: the kernel has no gradient output) and parameters are compared
with the float64 step.  Tolerances: tests/step_reference.py.  Trajectories: every step's losses (1e-5) and the final state.
A repeat of a launch at the same number of workgroups is bit-identical (the kernel's claim: no float atomics, fixed reduction
trees).  Across different numbers of workgroups it need not be: the dW partials are grouped by workgroup.
"""
import functools

import numpy as np
import pytest
import torch

from ggad_amd import synth
from oracle import ggad_oracle as O
import step_reference as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ggad_amd.graph import DeviceGraph
    from ggad_amd.minibatch import BatchChunk, MiniBatchEngine

DEV = "cuda:0"
F = R.F
XPC, XRA, XBT, XHUB = 2, 512, 256, 32          # csrc/step_xcd.hip
STATES = (0, 1, 10000)                          # step counter before the step; 0 = fresh optimiser state


@functools.lru_cache(maxsize=None)
def _graph(kind):
    """Power-law graphs from synth.make_graph: every node has degree >= 1 (ring); "main" has hubs of ~1,800 neighbours,
    "loops" self-loops on 5 % of its nodes."""
    if kind == "main":
        n, ne, seed, md, sl = 30000, 600000, 5, 2000, 0.0
    else:
        n, ne, seed, md, sl = 20000, 300000, 6, 300, 0.05
    rowptr, col = synth.make_graph(n, ne, seed, kind="powerlaw", max_degree=md, self_loop_frac=sl)
    feat = O.normalize_rows(synth.make_features(n, F, seed)).astype(np.float32)
    assert np.diff(rowptr).min() >= 1
    return rowptr, col, feat


@functools.lru_cache(maxsize=None)
def _device_graph(kind):
    rowptr, col, feat = _graph(kind)
    return DeviceGraph(rowptr, col, DEV), torch.from_numpy(feat).to(DEV)


def _labels(rng, n, n1):
    lab = np.zeros(n, dtype=np.int64)
    lab[rng.choice(n, n1, replace=False)] = 1
    return lab


def _batch(shape, seed):
    """(graph kind, nodes, labels) of one batch of the given shape; every batch holds both labels."""
    rng = np.random.default_rng(seed)
    kind = "loops" if shape == "dup" else "main"
    rowptr, col, _ = _graph(kind)
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    rows = dict(std=(200, 50), hub=(200, 50), large=(700, 175), xra=(1100, 600), ragged=(37, 9), tiny=(3, 1), dup=(200, 50))
    b, n1 = rows[shape]
    nodes = rng.choice(n, b, replace=False)
    lab = _labels(rng, b, n1)
    if shape == "hub":                                   # the two largest rows, one of each label
        top = np.argsort(deg)[-2:]
        i0, i1 = np.flatnonzero(lab == 0)[3], np.flatnonzero(lab == 1)[3]
        nodes[i0], nodes[i1] = top
        assert deg[top].min() + 1 >= 600
    if shape == "dup":                                   # a self-looped node twice with the same label, another with both labels
        loops = np.array([v for v in range(n) if v in set(col[rowptr[v]:rowptr[v + 1]].tolist())])
        assert len(loops) > 100
        a, c = rng.choice(loops, 2, replace=False)
        z, o = np.flatnonzero(lab == 0), np.flatnonzero(lab == 1)
        nodes[z[0]] = nodes[z[1]] = a
        nodes[z[2]] = nodes[o[0]] = c
    return kind, nodes.astype(np.int64), lab


@functools.lru_cache(maxsize=None)
def _agg64(shape, seed):
    kind, nodes, lab = _batch(shape, seed)
    rowptr, col, feat = _graph(kind)
    return O.aggregate_batch(rowptr, col, feat, nodes, True, dtype=np.float64)


def _chunk(kind, d, batches, labels):
    graph, feat = _device_graph(kind)
    ch = BatchChunk(graph, feat, d, max_batches=len(batches), rows_cap=256, ent_cap=8192, train=True, hop2="ldsw")
    ch.build(batches, labels)
    return ch


def _run_resident(eng, ch, nv):
    eng.xcd_wgs = nv
    eng.train_chunk(ch)
    st = eng.xcd_status()
    assert st["error"] == 0 and st["workgroups"] == nv, st


def _snapshot(eng, n_steps):
    torch.cuda.synchronize()
    return (eng.losses(n_steps).copy(), eng.params.cpu().numpy().copy(), eng.exp_avg.cpu().numpy().copy(),
            eng.exp_avg_sq.cpu().numpy().copy(), int(eng.step_counter.item()))


def _same(a, b, what):
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), f"{what}: a repeat of the launch is not bit-identical"
    assert a[4] == b[4]


# (D, nv, batch shape): every width at the trainer's nv = 28; every nv at D = 64 and 33; every batch shape at D = 64 and 33
CASES = sorted({(d, 28, "std") for d in (64, 63, 48, 33, 17, 16, 8, 1)}
               | {(d, nv, "std") for d in (64, 33) for nv in (24, 28, 32)}
               | {(d, 28, s) for d in (64, 33) for s in ("hub", "large", "xra", "ragged", "tiny", "dup")}
               | {(d, 24, "large") for d in (64, 33)}, key=lambda c: (c[2], -c[0], c[1]))


@pytest.mark.parametrize("d,nv,shape", CASES, ids=[f"{s}-d{d}-nv{nv}" for d, nv, s in CASES])
def test_teacher_forced_step(d, nv, shape):
    """One batch, one launch of the resident kernel, from fresh state and from preloaded moments at step counters 1 and 10,000:
    loss row, moments, parameters (transposed copies included) and step counter against the float64 step; every launch
    repeated once, bit-identical.  Tolerances: tests/step_reference.py."""
    seed = 1000 + {"std": 0, "hub": 1, "large": 2, "xra": 3, "ragged": 4, "tiny": 5, "dup": 6}[shape]
    kind, nodes, lab = _batch(shape, seed)
    agg = _agg64(shape, seed)
    ch = _chunk(kind, d, [nodes], [lab])
    n_ent, n_pieces = ch.n_ents, ch.n_chunks
    # the branch this shape is here for is really taken
    if shape == "hub":
        assert int(ch.batch_max_row[0]) >= 600 and (np.diff(ch.row_ck_ptr[:ch.n_rows + 1].cpu().numpy()) > XHUB).sum() >= 2
    if shape in ("large", "xra"):
        assert n_ent > 10000 and n_pieces > XPC * 8 * nv
    if shape == "xra":
        assert int(lab.sum()) > XRA
    if shape in ("ragged", "tiny"):
        assert len(nodes) % 16 != 0
    params = R.init_params(d, seed + d)
    p0 = R.flat(*params)
    ref_loss, g = R.loss_and_grad64(agg, lab, params)
    eng = MiniBatchEngine(F, d, DEV, lr=R.LR, weight_decay=R.WD, resident=True)
    for t0 in STATES:
        m0, v0 = R.preload_state(g, p0, t0, seed + t0)
        what = f"{shape} D={d} nv={nv} t0={t0}"
        runs = []
        for _ in range(2):
            R.load_state(eng, params, m0, v0, t0)
            _run_resident(eng, ch, nv)
            runs.append(_snapshot(eng, 1))
            if len(runs) == 1:
                R.check_losses(runs[0][0][0], ref_loss, what)
                R.check_step(eng, (p0, m0, v0, t0), g, what)
        _same(runs[0], runs[1], what)


CHAIN_D = (63, 33, 17, 8, 1)


@pytest.mark.parametrize("d", CHAIN_D)
def test_launch_chain_at_the_same_widths(d):
    """The launch chain (`resident=False`: `loss_and_grads` exposes the gradient, then `adam_step`) at the widths the resident
    kernel is checked at: losses, gradient, moments and parameters against the float64 step, fresh and preloaded state."""
    seed = 2000 + d
    kind, nodes, lab = _batch("std", seed)
    agg = _agg64("std", seed)
    ch = _chunk(kind, d, [nodes], [lab])
    params = R.init_params(d, seed)
    p0 = R.flat(*params)
    ref_loss, g = R.loss_and_grad64(agg, lab, params)
    eng = MiniBatchEngine(F, d, DEV, lr=R.LR, weight_decay=R.WD, resident=False)
    for t0 in (0, 10000):
        m0, v0 = R.preload_state(g, p0, t0, seed + t0)
        what = f"chain D={d} t0={t0}"
        R.load_state(eng, params, m0, v0, t0)
        eng.loss_and_grads(ch, 0, 0)
        R.check_losses(eng.losses(1)[0], ref_loss, what)
        R.check_grads(eng.grads.cpu().numpy(), g, what)
        eng.adam_step()
        R.check_step(eng, (p0, m0, v0, t0), g, what)


def _trajectory_batches(nb, rows, n1, seed):
    rng = np.random.default_rng(seed)
    rowptr, col, feat = _graph("main")
    n = len(rowptr) - 1
    batches = [rng.choice(n, rows, replace=False).astype(np.int64) for _ in range(nb)]
    labels = [_labels(rng, rows, n1) for _ in range(nb)]
    aggs = [O.aggregate_batch(rowptr, col, feat, b, True, dtype=np.float64) for b in batches]
    return batches, labels, aggs


@functools.lru_cache(maxsize=None)
def _trajectory_case(nb, rows, n1):
    return _trajectory_batches(nb, rows, n1, 3000 + nb)


@pytest.mark.parametrize("nb,rows,n1", [(20, 200, 50), (260, 12, 3)], ids=["20x200", "260x12"])
@pytest.mark.parametrize("t0", [0, 10000])
def test_trajectory_in_one_launch(nb, rows, n1, t0):
    """A whole chunk in one launch at nv = 28: bench's 20-batch chunk, and 260 small batches (more than XBT = 256: the later
    batches' offsets are read from global memory), from fresh state and from step counter 10,000 with preloaded moments.  The
    float64 reference runs the same steps on its own trajectory.  Every step's loss row: 1e-5 (as the suite's other trajectory
    checks).  Final moments: the single-step bounds of tests/step_reference.py carried through every step (each step adds its
    gradient tolerance and rounding, earlier contributions decay by beta1 / beta2).  Final parameters: the masked rule of a
    single step, 3e-6, where the gradient Adam saw stayed clear of 0 (as defined there) in every step -- the drift of 20 or 260
    steps measured 3e-7 at most -- and at most one opposite step elsewhere.  A repeat of the launch is bit-identical."""
    batches, labels, aggs = _trajectory_case(nb, rows, n1)
    d, nv = 64, 28
    params = R.init_params(d, 77)
    p = R.flat(*params)
    _, g_first = R.loss_and_grad64(aggs[0], labels[0], params)
    m, v = R.preload_state(g_first, p, t0, 5 + t0)
    eng = MiniBatchEngine(F, d, DEV, lr=R.LR, weight_decay=R.WD, resident=True)
    ch = _chunk("main", d, batches, labels)
    runs = []
    for _ in range(2):
        R.load_state(eng, params, m, v, t0)
        _run_resident(eng, ch, nv)
        runs.append(_snapshot(eng, nb))
    what = f"trajectory {nb}x{rows} t0={t0}"
    _same(runs[0], runs[1], what)
    losses, got_p, got_m, got_v, counter = runs[0]
    assert counter == t0 + nb
    # the float64 trajectory
    ref_losses = []
    gmin = np.full_like(p, np.inf)
    gmax = np.zeros(3)
    bm = bv = 0.0
    for b in range(nb):
        w_, W_, fc_ = R.split(p, d)
        loss, g = R.loss_and_grad64(aggs[b], labels[b], (w_.reshape(1, d), W_.reshape(d, F), fc_.reshape(d, d)))
        ref_losses.append(loss)
        gp = g + R.WD * p
        for k, s in enumerate(R.split(gp, d)):
            gmax[k] = max(gmax[k], np.abs(s).max())
        gmin = np.minimum(gmin, np.abs(gp))
        _, _, bm, bv = R.moment_bounds(g, p, m, v, bm, bv)
        p, m, v = O.adam_f64(p, m, v, g, t0 + b + 1, R.LR, R.WD)
    err = np.abs(losses - np.array(ref_losses)).max(axis=1)
    assert err.max() <= 1e-5, f"{what}: loss rows off by up to {err.max():.3e} (first bad step {int(np.argmax(err > 1e-5))})"
    R.check_moments(got_m, got_v, m, v, bm, bv, what)
    nt = eng.n_train
    for k, (name, a, r, lo) in enumerate(zip(("w", "W", "fc"), R.split(got_p[:nt].astype(np.float64), d), R.split(p, d),
                                             R.split(gmin, d))):
        diff = np.abs(a - r)
        sure = lo > max(1e-6 * gmax[k], 1e-6)
        assert sure.any() and diff[sure].max() < 3e-6, f"{what}: final {name} off by {diff[sure].max():.3e}"
        assert diff.max() < 2.1e-3, f"{what}: final {name} off by {diff.max():.3e}"
