"""The hand-over between steps of the XCD-resident chunk kernel (`k_train_chunk_xcd`, csrc/step_xcd.hip): the records and the
matrix-core operands of step b + 1 are loaded RAW during phase C of step b and masked at the bottom of the step with the piece
lengths of step b + 1's own records.  The other resident-kernel tests run chunks of one batch or of equal batches; here ONE launch
walks consecutive batches of different shapes (the builders of tests/test_resident_step_gpu.py):

  large   700 rows, > 10,000 entries: more than XPC = 2 pieces per wave (the pieces beyond are loaded inside the step)
  tiny    3 rows: most waves own no piece and no position
  hub     a row of >= 600 entries (summed by the whole workgroup)
  ragged  37 rows, pieces shorter than 16

in the orders [large, tiny, hub, ragged, large] and its reverse, at 24 and 32 workgroups and D = 64 (compile-time width) and 33
(run-time width, odd: scalar weight loads).  That covers the first step (nothing was prefetched), the last (nothing to prefetch)
and every change of piece count and piece length between neighbouring steps.

Checked: every step's loss row (1e-5) and the final moments and parameters against the float64 trajectory, with the bounds of
tests/step_reference.py carried from step to step exactly as tests/test_resident_step_gpu.py::test_trajectory_in_one_launch
carries them; a repeat of the launch is bit-identical; and the launch equals the same five batches run as five one-batch
launches in sequence BITWISE (loss rows, parameters, moments): a one-batch launch prefetches nothing, so every operand of its
step comes through the in-step loaders, and both ways must hand the matrix cores the same bits.  (On the parent of the commit
that introduced this test the equality was bitwise as well.)
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ggad_oracle as O
import step_reference as R
import test_resident_step_gpu as T

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ggad_amd.minibatch import MiniBatchEngine

F = R.F
ORDER = (("large", 1002), ("tiny", 1005), ("hub", 1001), ("ragged", 1004), ("large", 1012))
ORDERS = {"fwd": ORDER, "rev": ORDER[::-1]}
T0 = 10000                                                  # step counter before the launch, moments preloaded


@functools.lru_cache(maxsize=None)
def _reference(d, order):
    """float64 trajectory over the five batches: start state, per-step loss rows, final (p, m, v), carried moment bounds, and the
    smallest / largest gradient Adam saw per parameter / per tensor (for the masked parameter rule)."""
    batches = [T._batch(s, seed) for s, seed in ORDERS[order]]
    aggs = [T._agg64(s, seed) for s, seed in ORDERS[order]]
    params = R.init_params(d, 91)
    p = R.flat(*params)
    _, g_first = R.loss_and_grad64(aggs[0], batches[0][2], params)
    m, v = R.preload_state(g_first, p, T0, 17)
    start = (params, m.copy(), v.copy())
    ref_losses = []
    gmin = np.full_like(p, np.inf)
    gmax = np.zeros(3)
    bm = bv = 0.0
    for b, (_, _, lab) in enumerate(batches):
        w_, W_, fc_ = R.split(p, d)
        loss, g = R.loss_and_grad64(aggs[b], lab, (w_.reshape(1, d), W_.reshape(d, F), fc_.reshape(d, d)))
        ref_losses.append(loss)
        gp = g + R.WD * p
        for k, s in enumerate(R.split(gp, d)):
            gmax[k] = max(gmax[k], np.abs(s).max())
        gmin = np.minimum(gmin, np.abs(gp))
        _, _, bm, bv = R.moment_bounds(g, p, m, v, bm, bv)
        p, m, v = O.adam_f64(p, m, v, g, T0 + b + 1, R.LR, R.WD)
    return start, np.array(ref_losses), (p, m, v), (bm, bv), gmin, gmax


@pytest.mark.parametrize("order", ["fwd", "rev"])
@pytest.mark.parametrize("nv", [24, 32])
@pytest.mark.parametrize("d", [64, 33])
def test_steps_of_different_shapes_in_one_launch(d, nv, order):
    shapes = ORDERS[order]
    nb = len(shapes)
    batches = [T._batch(s, seed) for s, seed in shapes]
    assert {k for k, _, _ in batches} == {"main"}
    nodes, labels = [b[1] for b in batches], [b[2] for b in batches]
    (params, m0, v0), ref_losses, (p_ref, m_ref, v_ref), (bm, bv), gmin, gmax = _reference(d, order)
    what = f"hand-over {order} D={d} nv={nv}"
    eng = MiniBatchEngine(F, d, T.DEV, lr=R.LR, weight_decay=R.WD, resident=True)

    # the same five batches as five one-batch launches in sequence (nothing is prefetched in any of them)
    singles = [T._chunk("main", d, [n], [l]) for n, l in zip(nodes, labels)]
    for (s, _), c in zip(shapes, singles):                  # the branches these shapes are here for are really taken
        pieces = np.diff(c.row_ck_ptr[:c.n_rows + 1].cpu().numpy())
        if s == "large":
            assert c.n_chunks > T.XPC * 8 * nv
        if s == "tiny":
            assert c.n_rows == 3
        if s == "hub":
            assert int(c.batch_max_row[0]) >= 600 and (pieces > T.XHUB).sum() >= 2
        if s == "ragged":
            assert c.n_rows == 37 and c.n_ents < 16 * c.n_chunks
    R.load_state(eng, params, m0, v0, T0)
    for b, c in enumerate(singles):
        eng.xcd_wgs = nv
        eng.train_chunk(c, log_base=b)
        st = eng.xcd_status()
        assert st["error"] == 0 and st["workgroups"] == nv, st
    seq = T._snapshot(eng, nb)

    ch = T._chunk("main", d, nodes, labels)
    runs = []
    for _ in range(2):
        R.load_state(eng, params, m0, v0, T0)
        T._run_resident(eng, ch, nv)
        runs.append(T._snapshot(eng, nb))
    T._same(runs[0], runs[1], what)
    losses, got_p, got_m, got_v, counter = runs[0]
    assert counter == T0 + nb

    err = np.abs(losses - ref_losses).max(axis=1)
    print(f"{what}: loss rows off by {err.max():.3e}; one launch == five launches bitwise: "
          f"{[bool(np.array_equal(x.view(np.int32), y.view(np.int32))) for x, y in zip(runs[0][:4], seq[:4])]}")
    assert err.max() <= 1e-5, f"{what}: loss rows off by up to {err.max():.3e} (first bad step {int(np.argmax(err > 1e-5))})"
    R.check_moments(got_m, got_v, m_ref, v_ref, bm, bv, what)
    nt = eng.n_train
    for k, (name, a, r, lo) in enumerate(zip(("w", "W", "fc"), R.split(got_p[:nt].astype(np.float64), d), R.split(p_ref, d),
                                             R.split(gmin, d))):
        diff = np.abs(a - r)
        sure = lo > max(1e-6 * gmax[k], 1e-6)
        assert sure.any() and diff[sure].max() < 3e-6, f"{what}: final {name} off by {diff[sure].max():.3e}"
        assert diff.max() < 2.1e-3, f"{what}: final {name} off by {diff.max():.3e}"

    for x, y, name in zip(runs[0][:4], seq[:4], ("loss rows", "parameters", "exp_avg", "exp_avg_sq")):
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), f"{what}: {name} of one launch differ from five one-batch launches"
    assert seq[4] == counter
