"""Float64 reference of one mini-batch optimiser step and the checks that compare a HIP step with it (shared by
tests/test_resident_step_gpu.py and tests/test_fullsize_gpu.py; not a test module itself).

The reference is the oracle in float64 (`aggregate_batch` / `batch_loss` with dtype=np.float64, torch autograd) followed by
`adam_f64`, torch.optim.Adam's update restated in float64: lr 1e-3, weight decay 0.007, betas (0.9, 0.999), eps 1e-8.

Tolerances (the kernels run in fp32; every bound is a bound on |HIP - float64|):
  * loss terms: 1e-5 absolute, as every other mini-batch loss check of the suite;
  * gradient g: 3e-6 absolute + 2e-5 relative to |g|, the suite's gradient tolerance.  The resident kernel exposes no
    gradient; its gradient is pinned through the moments after the step, the tolerance carried through Adam's moment updates:
      exp_avg    = m0 + 0.1 (g + wd p0 - m0)        -> 0.1 dg
      exp_avg_sq = 0.999 v0 + 0.001 (g + wd p0)^2   -> 0.001 (2 |g + wd p0| dg + dg^2)
    plus the fp32 rounding of those updates (a few ulps: 2.4e-7 relative, far below the gradient term);
  * parameters after one Adam step: 3e-6 absolute where |g + wd p0| (the gradient Adam sees) is above 1e-6 of its tensor's
    largest magnitude AND above 1e-6 = 100 eps; elsewhere at most one opposite step (2.1 x the largest step of that tensor:
    2.1e-3 from fresh state).  A fresh-state Adam step is lr g' / (|g'| + eps), +-lr whatever the gradient's size unless
    |g'| is within a few hundred eps of 0, where its slope lr eps / g'^2 is steep: at |g'| = 3.8e-8 (above 1e-6 of a 2.2e-2
    scale; it occurs in W at D = 63) a 2e-9 round-off of an fp32 gradient sum moves the parameter by 9e-6.  From 1e-6 on the
    slope is below 10, so the round-off (a few 1e-8 at most on these sums) stays far below 3e-6.
"""
import numpy as np
import torch

from oracle import ggad_oracle as O

LR, WD = 1e-3, 0.007
F = 17


def init_params(d, seed):
    """xavier_uniform w (1, D), W (D, F), fc (D, D) as the trainer draws them (fp32)."""
    torch.manual_seed(seed)
    w = torch.nn.init.xavier_uniform_(torch.empty(1, d))
    W = torch.nn.init.xavier_uniform_(torch.empty(d, F))
    fc = torch.nn.init.xavier_uniform_(torch.empty(d, d))
    return w, W, fc


def flat(w, W, fc):
    return np.concatenate([np.asarray(t, dtype=np.float64).reshape(-1) for t in (w, W, fc)])


def loss_and_grad64(agg64, lab, params):
    """Four loss terms and the packed (w | W | fc) gradient of one batch, all float64."""
    p = O.MiniParams.leaves(*[np.asarray(t) for t in params], dtype=torch.float64)
    terms = O.batch_loss(p, agg64, lab, dtype=torch.float64)
    terms[0].backward()
    g = np.concatenate([t.grad.numpy().reshape(-1) for t in p.tensors()])
    return np.array([t.item() for t in terms]), g


def preload_state(g, p0, t0, seed):
    """Optimiser state as after t0 steps: fresh (t0 = 0), or moments of the size of this gradient (exp_avg_sq > 0)."""
    if t0 == 0:
        return np.zeros_like(p0), np.zeros_like(p0)
    rng = np.random.default_rng(seed)
    s = np.sqrt(np.mean((g + WD * p0) ** 2)) + 1e-12
    m0 = (s * rng.standard_normal(len(p0))).astype(np.float32).astype(np.float64)
    v0 = (s * s * rng.uniform(0.25, 4.0, len(p0))).astype(np.float32).astype(np.float64)
    return m0, v0


def split(x, d):
    return x[:d], x[d:d + d * F], x[d + d * F:d + d * F + d * d]


def grad_bound(g):
    return 3e-6 + 2e-5 * np.abs(g)


def check_grads(got, g, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - g)
    ratio = err / grad_bound(g)
    assert ratio.max() <= 1.0, f"{what}: gradient off by {err.max():.3e} (worst at {int(ratio.argmax())}, {ratio.max():.2f} x bound)"


def check_losses(got, ref, what, tol=1e-5):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    assert err.max() <= tol, f"{what}: losses {np.asarray(got).tolist()} vs float64 {ref.tolist()} (max err {err.max():.3e})"


def moment_bounds(g, p0, m0, v0, bm0=0.0, bv0=0.0):
    """float64 moments after one Adam step from (m0, v0) with gradient g, and the bounds on |fp32 - float64| they carry: the
    gradient tolerance through the update, fp32 rounding of the update, plus bm0 / bv0 already carried by m0 / v0."""
    gp = g + WD * p0
    dg = grad_bound(g)
    m_ref = m0 + 0.1 * (gp - m0)
    v_ref = 0.999 * v0 + 0.001 * gp * gp
    bm = 0.9 * bm0 + 0.1 * dg + 2.4e-7 * (np.abs(m_ref) + np.abs(gp) + np.abs(m0))
    bv = 0.999 * bv0 + 0.001 * (2.0 * np.abs(gp) * dg + dg * dg) + 2.4e-7 * (v_ref + 0.001 * gp * gp)
    return m_ref, v_ref, bm, bv


def check_moments(m1, v1, m_ref, v_ref, bm, bv, what):
    em = np.abs(np.asarray(m1, dtype=np.float64) - m_ref)
    ev = np.abs(np.asarray(v1, dtype=np.float64) - v_ref)
    assert (em <= bm).all(), f"{what}: exp_avg off by {em.max():.3e} ({(em / bm).max():.2f} x bound, worst at {int((em / bm).argmax())})"
    assert (ev <= bv).all(), f"{what}: exp_avg_sq off by {ev.max():.3e} ({(ev / bv).max():.2f} x bound, worst at {int((ev / bv).argmax())})"


def check_params_masked(p1, p_ref, p0, gp, d, what):
    """The masked Adam-step rule, tensor by tensor (module docstring)."""
    for name, a, r, q, s in zip(("w", "W", "fc"), split(np.asarray(p1, dtype=np.float64), d), split(p_ref, d), split(p0, d),
                                split(gp, d)):
        diff = np.abs(a - r)
        sure = np.abs(s) > max(1e-6 * np.abs(s).max(), 1e-6)
        if sure.any():
            assert diff[sure].max() < 3e-6, f"{what}: {name} off by {diff[sure].max():.3e} after the Adam step"
        assert diff.max() <= 2.1 * np.abs(r - q).max() + 1e-12, f"{what}: {name} off by {diff.max():.3e} (more than one opposite step)"


def check_step(eng, before, ref_g, what):
    """Everything one optimiser step of `eng` left (losses of log slot 0 aside): moments, parameters, transposed copies, step
    counter, against the float64 step from `before` = (p0, m0, v0, t0) with float64 gradient ref_g."""
    p0, m0, v0, t0 = before
    d, nt = eng.D, eng.n_train
    params = eng.params.cpu().numpy()
    check_moments(eng.exp_avg.cpu().numpy(), eng.exp_avg_sq.cpu().numpy(), *moment_bounds(ref_g, p0, m0, v0), what)
    p_ref, _, _ = O.adam_f64(p0, m0, v0, ref_g, t0 + 1, LR, WD)
    check_params_masked(params[:nt], p_ref, p0, ref_g + WD * p0, d, what)
    W = params[d:d + d * F].reshape(d, F)
    fc = params[d + d * F:nt].reshape(d, d)
    assert np.array_equal(params[nt:nt + F * d].reshape(F, d), W.T), f"{what}: Wt is not W^T"
    assert np.array_equal(params[nt + F * d:nt + F * d + d * d].reshape(d, d), fc.T), f"{what}: fcT is not fc^T"
    assert int(eng.step_counter.item()) == t0 + 1, what


def load_state(eng, params, m0, v0, t0):
    eng.load_params(*params)
    eng.exp_avg.copy_(torch.from_numpy(m0.astype(np.float32)))
    eng.exp_avg_sq.copy_(torch.from_numpy(v0.astype(np.float32)))
    eng.step_counter.fill_(int(t0))
