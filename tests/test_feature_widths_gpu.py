"""The mini-batch path at every feature width it promises (F up to 1,024; D <= 64 on the one-lane-per-channel step chain), against
float64 (inputs, references and bounds: tests/width_reference.py).

  1. the plan's aggregates x1 / x2 at F in {1, 9, 16, 17, 21, 22, 32, 33, 63, 64, 65, 128, 129, 1024} on the three 2-hop paths
     (`k_gather2_items<0>` / `k_gather2_w` / `k_count2` + `k_gather2`), and on the 32-float padded table (zeros and NaN behind the
     row), element by element within (terms + 4) 2^-24 sum |w| |feat|;
  2. `ggad_seg_mean` / `ggad_seg_wsum` called directly: rows of 0 .. 300 entries around the 64-entry block loop, 1 / 4 / 5 / 9 rows;
  3. the narrow step chain (`k_project<0>`, `k_fwd_rows<0>`, `k_bwd_flat<0>`, `k_grad_reduce`) teacher-forced against the float64
     step up to F * D = 9,472 (148 KB of dynamic LDS in `k_bwd_flat<0>`), `k_score` and `k_encode` at the same shapes;
  4. shapes the narrow chain cannot take are refused at construction.

The first test of the module is the first launch of `k_bwd_flat<0>` with more than 64 KB of dynamic LDS, (F, D) = (65, 64).
"""
import functools

import numpy as np
import pytest
import torch

import step_reference as R
import width_reference as WR

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from ggad_amd._lib import call, ptr
    from ggad_amd.graph import DeviceGraph
    from ggad_amd.minibatch import BatchChunk, MiniBatchEngine

DEV = "cuda:0"
WIDTHS = [1, 9, 16, 17, 21, 22, 32, 33, 63, 64, 65, 128, 129, 1024]


@functools.lru_cache(maxsize=None)
def _device_graph():
    return DeviceGraph(*WR.graph(), DEV)


@functools.lru_cache(maxsize=None)
def _device_feat(f, pad=None):
    x = WR.feat(f)
    if pad is not None:
        x = WR.padded(x, fill=float("nan") if pad == "nan" else 0.0)
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _chunk(f, d, pad=None, **kw):
    cases = WR.batches()
    ch = BatchChunk(_device_graph(), _device_feat(f, pad), d, max_batches=len(cases), rows_cap=256, ent_cap=8192, train=True,
                    feat_dim=f if pad is not None else None, **kw)
    ch.build([c[1] for c in cases], [c[2] for c in cases])
    torch.cuda.synchronize()
    sizes = np.diff(ch.ent_ptr_host)
    assert int(ch.batch_max_row[0]) >= WR.HUB_MIN and sizes.min() == 2 and (sizes == 16).any() and (sizes == 17).any()
    return ch


# ------------------------------------------------------------------ 3a: the first launch above 64 KB
def _step_case(f, d, chain):
    """Teacher-forced steps (`loss_and_grads`, then `adam_step`) of every batch, from fresh state and from preloaded moments at step
    counter 10,000: losses, packed gradient, moments, parameters, transposed copies and step counter against the float64 step with
    the tolerances of tests/step_reference.py.  Prints |device - float64|, |float32 oracle - float64| and their ratio."""
    WR.check_step_conditions(f, d)                       # from the float64 reference alone, before the device is looked at
    ref = WR.step_reference(f, d)
    params = WR.init_params(f, d)
    p0 = R.flat(*params)
    ch = _chunk(f, d, pad="zero" if (f, d) in WR.PADDED_STEP else None, hop2="ldsw")
    eng = MiniBatchEngine(f, d, DEV, lr=R.LR, weight_decay=R.WD, chain=chain)
    assert not eng.wide and not eng.resident
    failures = []
    worst_l = worst_g = 0.0
    for b, ((shape, _, _), (ref_loss, g, l32, g32)) in enumerate(zip(WR.batches(), ref)):
        for t0 in (0, 10000):
            what = f"F={f} D={d} chain {chain} {shape} t0={t0}"
            m0, v0 = R.preload_state(g, p0, t0, 7 + t0)
            R.load_state(eng, params, m0, v0, t0)
            eng.loss_and_grads(ch, b, 0)
            got_l = eng.losses(1)[0].astype(np.float64)
            got_g = eng.grads.cpu().numpy().astype(np.float64)
            if t0 == 0:
                el, el32 = np.abs(got_l - ref_loss).max(), np.abs(l32 - ref_loss).max()
                rg, rg32 = (np.abs(got_g - g) / R.grad_bound(g)).max(), (np.abs(g32 - g) / R.grad_bound(g)).max()
                worst_l, worst_g = max(worst_l, el), max(worst_g, rg)
                print(f"{what}: loss err device {el:.2e} f32-oracle {el32:.2e} ratio {el / max(el32, 1e-30):.1f} | "
                      f"grad err/bound device {rg:.3f} f32-oracle {rg32:.3f} ratio {rg / max(rg32, 1e-30):.1f} "
                      f"(|g|max {np.abs(g).max():.2e})")
            try:
                R.check_losses(got_l, ref_loss, what)
                R.check_grads(got_g, g, what)
                eng.adam_step()
                WR.check_step(eng, (p0, m0, v0, t0), g, what)
            except AssertionError as exc:
                failures.append(str(exc))
    print(f"WORST step F={f} D={d} chain {chain}: loss err {worst_l:.2e} (bound 1e-5), grad err/bound {worst_g:.3f}")
    assert not failures, "\n".join(failures)


def test_first_bwd_flat_launch_above_64_kb():
    """(F, D) = (65, 64): `k_bwd_flat<0>` asks for 4 * 65 * 64 * 4 = 66,560 bytes of dynamic LDS.  A runtime that refuses the launch
    makes `loss_and_grads` raise (an error code through `_lib.check`)."""
    _step_case(65, 64, 0)


# ------------------------------------------------------------------ 1: plan aggregates
PATHS = {"items": dict(hop2="ldsw", node_major=True),          # k_gather2_items<0> at F <= 64, k_gather2_w above
         "wave": dict(hop2="ldsw", node_major=False),          # k_gather2_w at every F
         "global": dict(hop2="global")}                        # k_count2 / k_gather2


def _plan_case(f, path, pad=None):
    ch = _chunk(f, 8, pad, **PATHS[path])
    assert ch.last_hop2 == PATHS[path]["hop2"]
    what = f"F={f} {path}" + (f" padded({pad})" if pad else "")
    worst = WR.check_plan(ch, f, what)
    print(f"WORST plan {what}: error / bound {worst:.3f}")
    torch.cuda.synchronize()
    assert int(ch.cnt1.abs().sum()) == 0, "cnt1 is not clean after the build"
    assert ch.cnt2 is None or int(ch.cnt2.abs().sum()) == 0, "cnt2 is not clean after the build"
    if ch.hop2 == "ldsw":
        assert int(ch.node_head.abs().sum()) == 0, "node_head is not clean after the build"


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("f", WIDTHS)
def test_plan_aggregates_against_float64(f, path):
    _plan_case(f, path)


@pytest.mark.parametrize("path", ["items", "wave"])
@pytest.mark.parametrize("f,pad", [(1, "zero"), (9, "zero"), (25, "zero"), (17, "zero"), (9, "nan")])
def test_plan_aggregates_on_padded_rows(f, pad, path):
    """Rows of 32 floats with `feat_dim=F`, as the trainer pads every F <= 32; NaN behind the row: the padding is never read."""
    _plan_case(f, path, pad)


# ------------------------------------------------------------------ 2: ggad_seg_mean / ggad_seg_wsum
def _seg(name, feat_t, f, sp, sc, sw, n_rows, out):
    if name == "ggad_seg_mean":
        call(name, ptr(feat_t), f, ptr(sp), ptr(sc), n_rows, ptr(out))
    else:
        call(name, ptr(feat_t), f, ptr(sp), ptr(sc), ptr(sw), n_rows, ptr(out))


@pytest.mark.parametrize("f", WIDTHS)
def test_seg_mean_and_wsum_against_float64(f):
    """Both entry points on the first 1, 4, 5 and 9 rows of the ragged list (lengths 300, 0, 65, 1, 130, 64, 2, 128, 63): within
    (r + 3) 2^-24 sum |w| |x| of float64 per element; the empty row is NaN in every column; the row behind the last is not written;
    equal inputs give equal bits; n_rows = 0 returns OK and writes nothing."""
    sp_h, sc_h, sw_h = WR.seg_lists()
    mean, wsum, b_mean, b_wsum = WR.seg_reference(f)
    feat_t = _device_feat(f)
    sp, sc, sw = (torch.from_numpy(np.array(a)).to(DEV) for a in (sp_h, sc_h, sw_h))
    empty = [i for i, n in enumerate(WR.SEG_LENGTHS) if n == 0]
    assert empty == [1]
    worst = {}
    for name, ref, bound in (("ggad_seg_mean", mean, b_mean), ("ggad_seg_wsum", wsum, b_wsum)):
        for n_rows in (1, 4, 5, 9):
            out = torch.full(((n_rows + 1) * f,), float("nan"), dtype=torch.float32, device=DEV)
            _seg(name, feat_t, f, sp, sc, sw, n_rows, out)
            torch.cuda.synchronize()
            got = out.cpu().numpy().reshape(n_rows + 1, f)
            assert np.isnan(got[n_rows]).all(), f"{name} F={f} n_rows={n_rows}: wrote behind the last row"
            got = got[:n_rows].astype(np.float64)
            r, bd = ref[:n_rows], bound[:n_rows]
            assert np.array_equal(np.isnan(got), np.isnan(r)), f"{name} F={f} n_rows={n_rows}: NaN rows {np.flatnonzero(np.isnan(got).any(1))}"
            if n_rows > 1:
                assert np.isnan(got[1]).all()
            ok = ~np.isnan(r)
            err = np.where(ok, np.abs(got - r), 0.0)
            ratio = (err / np.maximum(np.where(ok, bd, 1.0), 1e-300)).max()
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert (err <= bd).all(), f"{name} F={f} n_rows={n_rows}: off by {err.max():.3e}, {ratio:.2f} x bound (row {int((err / np.maximum(bd, 1e-300)).max(1).argmax())})"
            again = torch.full_like(out, float("nan"))
            _seg(name, feat_t, f, sp, sc, sw, n_rows, again)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.int32), again.cpu().numpy().view(np.int32)), f"{name} F={f}: second call differs"
        out = torch.full((2 * f,), float("nan"), dtype=torch.float32, device=DEV)
        before = out.cpu().numpy().view(np.int32).copy()
        _seg(name, feat_t, f, sp, sc, sw, 0, out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.int32), before), f"{name} F={f}: n_rows = 0 wrote to out"
    print(f"WORST seg F={f}: error / bound mean {worst['ggad_seg_mean']:.3f} wsum {worst['ggad_seg_wsum']:.3f}")


# ------------------------------------------------------------------ 3b: the narrow step chain
@pytest.mark.parametrize("f,d,chain", WR.STEP_CASES[1:], ids=[f"f{f}-d{d}-chain{c}" for f, d, c in WR.STEP_CASES[1:]])
def test_narrow_step_against_float64(f, d, chain):
    _step_case(f, d, chain)


INFER_CASES = sorted({(f, d) for f, d, _ in WR.STEP_CASES})


@pytest.mark.parametrize("f,d", INFER_CASES, ids=[f"f{f}-d{d}" for f, d in INFER_CASES])
def test_score_and_encode_against_float64(f, d):
    """`k_score` against the float64 sigmoid at 3e-6 and `k_encode` within (F + 2) 2^-24 sum_f |W_df| |x_f| per element, on the
    181 aggregated rows of the three batches (not a multiple of 4) and on 4 * 4096 + 3 rows (more rows than the 4,096 workgroups
    of four waves take in one pass)."""
    params = WR.init_params(f, d)
    w, W = params[0].numpy().astype(np.float64), params[1].numpy().astype(np.float64)
    eng = MiniBatchEngine(f, d, DEV)
    assert not eng.wide
    eng.load_params(*params)
    x_small = np.concatenate([a64.to_feats for a64, _, _ in WR.aggs(f)]).astype(np.float32)
    assert x_small.shape[0] % 4 != 0
    rng = np.random.default_rng(f + d)
    x_big = x_small[rng.integers(0, len(x_small), 4 * 4096 + 3)] * rng.uniform(0.5, 2.0, (4 * 4096 + 3, 1)).astype(np.float32)
    for x in (x_small, x_big):
        n = x.shape[0]
        x64 = x.astype(np.float64)
        pre = x64 @ W.T
        h_ref = np.maximum(pre, 0.0)
        prob_ref = 1.0 / (1.0 + np.exp(-(h_ref @ w.reshape(-1))))
        h_bound = (f + 2) * WR.U * (np.abs(x64) @ np.abs(W).T)
        xt = torch.from_numpy(x).to(DEV)
        prob = torch.full((n + 1,), float("nan"), dtype=torch.float32, device=DEV)
        h = torch.full(((n + 1) * d,), float("nan"), dtype=torch.float32, device=DEV)
        call("ggad_mb_score", ptr(eng.params), d, f, ptr(xt), n, ptr(prob))
        call("ggad_mb_encode", ptr(eng.params), d, f, ptr(xt), n, ptr(h))
        torch.cuda.synchronize()
        prob, h = prob.cpu().numpy().astype(np.float64), h.cpu().numpy().astype(np.float64).reshape(n + 1, d)
        assert np.isnan(prob[n]) and np.isnan(h[n]).all(), "wrote behind the last row"
        e_p = np.abs(prob[:n] - prob_ref).max()
        e_h = np.abs(h[:n] - h_ref)
        ratio = (e_h / np.maximum(h_bound, 1e-300)).max()
        print(f"WORST infer F={f} D={d} rows {n}: score err {e_p:.2e} (bound 3e-6), encode err / bound {ratio:.3f}")
        assert e_p <= 3e-6, f"F={f} D={d} rows {n}: score off by {e_p:.3e}"
        assert (e_h <= h_bound).all(), f"F={f} D={d} rows {n}: encode off by {e_h.max():.3e}, {ratio:.2f} x bound"


# ------------------------------------------------------------------ 4: refusal up front
@pytest.mark.parametrize("chain", [0, 2])
@pytest.mark.parametrize("f,d", [(149, 64), (297, 32), (1025, 1)])
def test_unsupported_narrow_shape_is_refused_at_construction(f, d, chain):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="features <= ") as exc:
        MiniBatchEngine(f, d, DEV, chain=chain)
    assert "chain=3" in str(exc.value)
    assert torch.cuda.memory_allocated() == before


@pytest.mark.parametrize("f,d", [(148, 64), (296, 32), (1024, 9)])
def test_largest_narrow_shapes_construct(f, d):
    for chain in (0, 2):
        eng = MiniBatchEngine(f, d, DEV, chain=chain)
        assert not eng.wide and not eng.resident


def test_refused_narrow_shape_steps_on_chain_3():
    """(F, D) = (745, 64): refused by chains 0 and 2, taken by `chain=3`; one teacher-forced step within the float64 bounds."""
    f, d = 745, 64
    with pytest.raises(ValueError, match="chain=3"):
        MiniBatchEngine(f, d, DEV)
    eng = MiniBatchEngine(f, d, DEV, lr=R.LR, weight_decay=R.WD, chain=3)
    assert eng.wide and not eng.resident
    params = WR.init_params(f, d)
    p0 = R.flat(*params)
    (shape, _, lab), (a64, _, _) = WR.batches()[0], WR.aggs(f)[0]
    ref_loss, g = R.loss_and_grad64(a64, lab, params)
    ch = _chunk(f, d, hop2="ldsw")
    what = f"F={f} D={d} chain 3 {shape}"
    m0, v0 = R.preload_state(g, p0, 0, 7)
    R.load_state(eng, params, m0, v0, 0)
    eng.loss_and_grads(ch, 0, 0)
    got_l = eng.losses(1)[0].astype(np.float64)
    got_g = eng.grads.cpu().numpy().astype(np.float64)
    print(f"WORST step {what}: loss err {np.abs(got_l - ref_loss).max():.2e}, grad err/bound {(np.abs(got_g - g) / R.grad_bound(g)).max():.3f}")
    R.check_losses(got_l, ref_loss, what)
    R.check_grads(got_g, g, what)
    eng.adam_step()
    WR.check_step(eng, (p0, m0, v0, 0), g, what)
