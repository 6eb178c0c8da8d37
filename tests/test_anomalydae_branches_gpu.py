"""The loop branches of csrc/anomalydae.hip against the sparse float64 oracle (`oracle/ggad_oracle.py`: `adae_gat`, `adae_recon`,
computed by torch in float64 on the device: torch's kernels, not ours), at the shapes where they change course:

GAT layer (`k_gat_fwd`, `k_gat_bwd_tgt`, `k_gat_bwd_src`; lanes over edges, `k = lane; k <= deg; k += 64`):
  * targets with 62, 63, 64, 65, 127, 128, 129 stored in-entries, with and without a raw self loop among them: the added self
    loop (slot k == deg) moves from the first pass to the second (and third), and `k_gat_bwd_tgt` re-reads its own `dpre`
    slots across passes;
  * a target hub of 3,000 in-entries and (asymmetric graph, `tmap`) a source hub of 2,500 out-entries with in-degree 3;
  * stored zeros (`gat_edge`'s `tval <= 0`), in every graph; N = 1 and N = 2;
  * output widths F = 1, 63, 64, 65 (one and two 64-lane feature passes), 745, input widths 40 and 300.
Fused loss (`k_stru_fwd_dense` / `_rows`, `k_mean`, `k_stru_bwd_dense`, `k_stru_bwd_combine`):
  * N = 16,384 / 16,385 / 40,000 / 46,564: 64, 65, 157, 182 column blocks per row (the `part` loop of `k_stru_fwd_rows`);
  * |R| = 1, 1,023, 1,024, 1,025, N: `k_mean`'s `per > 1`; the row pass's split count `bwd_split(|R|, N)` reaches 625 and 728 at
    |R| = 1, while at |R| = N one split walks every node;
  * F = 1, 3, 4, 5, 16, 17, 745, 768 (768: the last output tile t = 11 of wave 3); F = 769 is refused;
  * unsorted rows holding a hub row (a column every 8th row touches: `k_stru_bwd_combine`'s long `tptr` walks), an isolated
    row, a self-loop-only row and a row with a stored zero; one case where most s are exactly 1.0f (and 0.0f).
Every case runs twice and the second run must be bit-identical (the kernels use no float atomics).

Tolerances (|HIP - float64|, relative to `scale` = the largest magnitude of the float64 tensor):
  * GAT z: 2e-5.  y = h W^T is an fp32 GEMM over K = 40 / 300; z_i = sum_r p_ri y_r is a convex combination of up to 3,001 rows,
    summed in a fixed order: the rounding walks as sqrt(K) eps |y| (3,001 terms: 55 x 6e-8 = 3.3e-6) -- x6 margin;
  * GAT gradients: 1e-4, the suite's full-size gradient tolerance (test_fullgraph_fullsize_gpu.py): dW and d att are sums over
    all N = 4,000 rows of products that already carry the sums above.  d att_src and d att_dst share one scale, the larger of
    the two: both are y-weighted sums of the same per-edge terms dpre_ri (grouped by source, by target), so they carry the
    same rounding, but d att_dst can cancel to exactly 0 -- a target whose incoming pre-activations share one leaky-ReLU slope
    has sum_r dpre_ri = sum_r p_ri (q_ri - S_i) = 0 (as in the N = 2 graph here) -- leaving only fp32 round-off;
  * loss and score: 4e-6 relative + 1e-6.  stru_i^2 sums N terms s^2 in at most 16 + 4 + 64 + 6 roundings (tile registers,
    16-column butterfly, 4 waves, column blocks over lanes, wave butterfly) plus the edge correction: 90 eps = 5.4e-6 worst
    case on stru^2, half of that on stru; the mean over |R| rows adds |R| / 1,024 + 16 roundings;
  * dz: 2e-4 relative + 2e-5 of scale, the bound of test_recon_loss_forward_backward_vs_float64 (relative 2e-4, absolute 1e-5
    of scale) with the absolute part doubled: the split partials of the longest sums here (N = 46,564 walked rows against 301)
    add up to 2 x 46,564 / 64 block products of 64 terms each in fp32; dx_hat: 1e-5 relative + 1e-8, as there.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _full(m):
    from ggad_amd.fullgraph import FullGraphAdj
    return FullGraphAdj(m, m, DEV)


def _csr(r, c, v, n):
    m = sp.csr_matrix((np.asarray(v, dtype=np.float64), (np.asarray(r), np.asarray(c))), shape=(n, n))
    m.sort_indices()
    return m


def _unique_pairs(r, c, n):
    key = np.unique(np.asarray(r, dtype=np.int64) * n + np.asarray(c, dtype=np.int64))
    return key // n, key % n


def _values(r, c, n, symmetric, zero_frac=0.02):
    """A_hat-like values in [0.05, 1.05), a stored zero at about 2 % of the off-diagonal entries; symmetric graphs get the same
    value (and the same zeros) at (r, c) and (c, r)."""
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    key = (lo * n + hi if symmetric else r * n + c).astype(np.uint64)
    h = ((key * np.uint64(2654435761) + np.uint64(97)) % np.uint64(1 << 32)) / float(1 << 32)    # a deterministic per-pair uniform
    v = 0.05 + h
    z = ((key * np.uint64(40503) + np.uint64(11)) % np.uint64(1000)) < 1000 * zero_frac
    v[z & (r != c)] = 0.0
    return v


DEGREES = [62, 63, 64, 65, 127, 128, 129]


def _gat_graph(kind, seed=0):
    """(csr, expected in-entry count of the designated targets).  `asym` / `sym`: 4,000 nodes, the 14 designated targets
    (DEGREES, without / with a raw self loop among the entries), a 3,000-entry target hub, in `asym` a source hub of 2,500 entries
    whose own column holds 3, background entries between the other nodes (8 per node, raw self loops on every 5th), an isolated
    node and a self-loop-only node.  `n1` / `n2`: the smallest graphs."""
    if kind == "n1":
        return _csr([0], [0], [1.0], 1), {}
    if kind == "n2":
        return _csr([0, 0, 1, 1], [0, 1, 0, 1], [1.0, 0.6, 0.0, 1.0], 2), {}
    sym = kind == "sym"
    n = 4000
    rng = np.random.default_rng(seed + sym)
    special = np.arange(len(DEGREES) * 2 + 4)                             # designated targets, target hub, source hub, isolated, loop-only
    t_hub, s_hub, iso, loop_only = special[-4:]
    pool = np.arange(len(special), n)
    R, C = [], []
    want = {}
    for k, d in enumerate(DEGREES * 2):
        t = int(special[k])
        with_loop = k >= len(DEGREES)
        src = rng.choice(pool, d - with_loop, replace=False)
        R += [src, [t] * with_loop]
        C += [np.full(len(src), t), [t] * with_loop]
        want[t] = d
    src = rng.choice(pool, 3000, replace=False)
    R.append(src)
    C.append(np.full(3000, t_hub))
    want[int(t_hub)] = 3000
    if not sym:
        dst = rng.choice(pool, 2500, replace=False)
        R += [np.full(2500, s_hub), rng.choice(pool, 3, replace=False)]
        C += [dst, np.full(3, s_hub)]
        want[int(s_hub)] = 3
    r = rng.choice(pool, 8 * len(pool))
    c = rng.choice(pool, 8 * len(pool))
    R += [r[r != c], pool[::5], [loop_only]]
    C += [c[r != c], pool[::5], [loop_only]]
    r, c = np.concatenate(R).astype(np.int64), np.concatenate(C).astype(np.int64)
    if sym:
        r, c = np.concatenate([r, c]), np.concatenate([c, r])
    r, c = _unique_pairs(r, c, n)
    m = _csr(r, c, _values(r, c, n, sym), n)
    return m, want


def _gat_run(conv, h, fa, g):
    for p in conv.parameters():
        p.grad = None
    hd = h.clone().requires_grad_(True)
    z = conv(hd, fa)
    z.backward(g)
    torch.cuda.synchronize()
    return [z.detach().clone(), hd.grad.clone(), conv.lin_src.weight.grad.clone(), conv.att_src.grad.clone(),
            conv.att_dst.grad.clone(), conv.bias.grad.clone()]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _close(got, ref, tol, what, scale=None):
    ref = ref.detach()
    scale = float(ref.abs().max()) + 1e-30 if scale is None else scale
    err = float((got.double() - ref).abs().max()) / scale
    print(f"  {what}: max |HIP - f64| / scale = {err:.2e} (scale {scale:.3e})")
    assert err <= tol, f"{what}: {err:.3e} of scale {scale:.3e} (bound {tol:.0e})"


@pytest.mark.parametrize("f,hd", [(1, 40), (63, 40), (64, 300), (65, 40), (745, 300)], ids=lambda v: str(v))
@pytest.mark.parametrize("kind", ["asym", "sym", "n1", "n2"])
def test_gat_branches_vs_float64(kind, f, hd):
    from ggad_amd.gat import GATConv
    from oracle import ggad_oracle as O
    m, want = _gat_graph(kind)
    n = m.shape[0]
    col_cnt = np.bincount(m.indices, minlength=n)
    for t, d in want.items():
        assert col_cnt[t] == d, (t, d, col_cnt[t])                        # the stored in-entries each branch needs
    if kind in ("asym", "sym"):
        assert (m.data == 0).sum() > 100 and np.diff(m.indptr).max() >= 2500
        if kind == "asym":
            assert np.diff(m.indptr)[len(DEGREES) * 2 + 1] == 2500              # the source hub's row
    fa = _full(m)
    assert fa.symmetric == (kind in ("sym", "n1"))
    torch.manual_seed(f + hd)
    conv = GATConv(hd, f)
    conv.bias.data.normal_()
    conv.to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(f * 7 + n)
    h = torch.randn(n, hd, device=DEV, generator=gen)
    g = torch.randn(n, f, device=DEV, generator=gen)
    got = _gat_run(conv, h, fa, g)
    again = _gat_run(conv, h, fa, g)
    for k, (a, b) in enumerate(zip(got, again)):
        assert _bits_equal(a, b), f"launch 2 differs from launch 1 in output {k}"
    h64 = h.double().requires_grad_(True)
    ps = [p.detach().double().requires_grad_(True) for p in (conv.lin_src.weight, conv.att_src, conv.att_dst, conv.bias)]
    ref = O.adae_gat(h64, *ps, m.indptr, m.indices, m.data.astype(np.float32))
    ref.backward(g.double())
    print(f"[gat {kind} F={f} in={hd}]")
    _close(got[0], ref, 2e-5, "z")
    att_scale = max(float(ps[1].grad.abs().max()), float(ps[2].grad.abs().max())) + 1e-30
    for name, a, b in zip(["dh", "dW", "d att_src", "d att_dst", "d bias"], got[1:], [h64.grad] + [p.grad for p in ps]):
        _close(a, b, 1e-4, name, att_scale if name.startswith("d att") else None)


def _loss_graph(n, seed):
    """Symmetric A_hat-like graph: 4 entries per node drawn at random (both directions), self loops on every node but the
    isolated one (n - 1), a hub node 0 linked to n / 8 nodes, a self-loop-only node (n - 2), stored zeros.
    Returns (csr, hub, isolated, loop-only, a row holding a stored zero)."""
    rng = np.random.default_rng(seed)
    body = np.arange(1, n - 2)
    r = rng.choice(body, 4 * len(body))
    c = rng.choice(body, 4 * len(body))
    hub_nb = rng.choice(body, max(1, n // 8), replace=False)
    r = np.concatenate([r, np.zeros(len(hub_nb), dtype=np.int64)])
    c = np.concatenate([c, hub_nb])
    r, c = np.concatenate([r, c]), np.concatenate([c, r])
    r, c = np.concatenate([r, np.arange(n - 1)]), np.concatenate([c, np.arange(n - 1)])
    r, c = _unique_pairs(r, c, n)
    v = _values(r, c, n, True)
    m = _csr(r, c, v, n)
    zr = np.repeat(np.arange(n), np.diff(m.indptr))[m.data == 0]
    zero_row = int(zr[(zr != 0)][0])
    return m, 0, n - 1, n - 2, zero_row


LOSS_CASES = [                      # (N, |R|, F, scale of z)
    (16384, 1025, 16, 0.3),
    (16385, 1024, 17, 0.3),
    (16385, 1023, 5, 0.5),
    (16385, 16385, 1, 1.0),
    (40000, 1, 3, 0.5),
    (46564, 1, 4, 0.5),
    (46564, 46564, 3, 0.4),
    (3000, 1025, 745, 0.05),
    (3000, 700, 768, 0.05),
    (3001, 1024, 1, 1.0),
    (3000, 1025, 16, 5.0),          # saturated: |z_i . z_j| mostly far above 17, s = 1.0f / 0.0f exactly
]


def _rows(n, n_rows, specials, seed):
    rng = np.random.default_rng(seed)
    rest = np.setdiff1d(np.arange(n), specials)
    rows = np.concatenate([specials, rng.choice(rest, max(0, n_rows - len(specials)), replace=False)])[:n_rows]
    return rng.permutation(rows).astype(np.int64) if n_rows > 1 else rows.astype(np.int64)


def _loss_run(z, xh, x, fa, rows):
    from ggad_amd.model_anomalydae import recon_loss, recon_score
    zd = z.clone().requires_grad_(True)
    xhd = xh.clone().requires_grad_(True)
    loss, score = recon_loss(zd, xhd, x, fa, rows)
    (2.5 * loss).backward()
    rsc = recon_score(z, xh, x, fa, rows)
    torch.cuda.synchronize()
    return [loss.detach().reshape(1).clone(), score.clone(), rsc, zd.grad.clone(), xhd.grad.clone()]


@pytest.mark.parametrize("n,n_rows,f,scale", LOSS_CASES, ids=lambda v: str(v))
def test_recon_loss_branches_vs_float64(n, n_rows, f, scale):
    from oracle import ggad_oracle as O
    m, hub, iso, loop_only, zero_row = _loss_graph(n, n + f)
    assert np.diff(m.indptr)[hub] >= n // 8 and np.diff(m.indptr)[iso] == 0 and np.diff(m.indptr)[loop_only] == 1
    rows = _rows(n, n_rows, np.array([hub, iso, loop_only, zero_row]), n_rows + f)
    fa = _full(m)
    gen = torch.Generator(device=DEV).manual_seed(n + n_rows + f)
    z = torch.randn(n, f, device=DEV, generator=gen) * scale
    x = torch.rand(n, f, device=DEV, generator=gen)
    xh = torch.randn(n, f, device=DEV, generator=gen)
    got = _loss_run(z, xh, x, fa, rows)
    again = _loss_run(z, xh, x, fa, rows)
    for k, (a, b) in enumerate(zip(got, again)):
        assert _bits_equal(a, b), f"launch 2 differs from launch 1 in output {k}"
    assert _bits_equal(got[1], got[2]), "recon_score differs from the training forward's score"
    z64 = z.double().requires_grad_(True)
    xh64 = xh.double().requires_grad_(True)
    A = (m.indptr, m.indices, m.data.astype(np.float32))
    loss, score, _, _ = O.adae_recon(z64, xh64, x.double(), A, rows)
    (2.5 * loss).backward()
    if scale >= 3.0:
        with torch.no_grad():
            s32 = torch.sigmoid(z[torch.from_numpy(rows[:64]).to(DEV)] @ z.T)
            assert float(((s32 == 1.0) | (s32 == 0.0)).float().mean()) > 0.5
    print(f"[loss N={n} R={n_rows} F={f} scale={scale}] loss {loss.item():.6f}")
    le = abs(float(got[0]) - loss.item())
    print(f"  loss: |HIP - f64| = {le:.2e}")
    assert le <= 4e-6 * abs(loss.item()) + 1e-6
    se = (got[1].double() - score.detach()).abs()
    print(f"  score: max |HIP - f64| = {float(se.max()):.2e}, relative {float((se / score.detach().abs()).max()):.2e}")
    assert bool((se <= 4e-6 * score.detach().abs() + 1e-6).all())
    gz = z64.grad
    dz_err = (got[3].double() - gz).abs()
    gscale = float(gz.abs().max())
    print(f"  dz: max |HIP - f64| / scale = {float(dz_err.max()) / gscale:.2e} (scale {gscale:.3e})")
    assert bool((dz_err <= 2e-4 * gz.abs() + 2e-5 * gscale).all())
    gx = xh64.grad
    assert bool(((got[4].double() - gx).abs() <= 1e-5 * gx.abs() + 1e-8).all())


def test_recon_loss_refuses_769_features():
    """F = 769 is past the backward's 12 output tiles: `recon_loss` raises before building anything, and the C ABI's backward
    refuses with GGAD_E_INVALID before launching (dz keeps its sentinel)."""
    from ggad_amd import _lib
    from ggad_amd._lib import call, ptr
    from ggad_amd.model_anomalydae import recon_loss, row_structs
    m, hub, iso, loop_only, zero_row = _loss_graph(200, 1)
    fa = _full(m)
    rows = np.array([hub, iso, 5, 9], dtype=np.int64)
    z = torch.zeros(200, 769, device=DEV)
    with pytest.raises(ValueError, match="768"):
        recon_loss(z, z, z, fa, rows)
    rs = row_structs(fa, rows)
    n, nr, F = 200, len(rows), 769
    ws = torch.zeros(int(_lib.load().ggad_adae_stru_bwd_workspace_elems(nr, n, F)), device=DEV)
    dz = torch.full((n, F), 7.0, device=DEV)
    s_edge = torch.zeros(max(rs["nnz"], 1), device=DEV)
    stru, g = torch.ones(nr, device=DEV), torch.ones(1, device=DEV)
    with pytest.raises(_lib.GgadKernelError, match="code -1"):
        call("ggad_adae_stru_bwd_f32", ptr(z), n, F, ptr(rs["rows"]), nr, ptr(rs["rptr"]), ptr(rs["rcol"]), ptr(rs["rval"]),
             ptr(s_edge), ptr(rs["pos"]), ptr(rs["tptr"]), ptr(rs["trow"]), ptr(rs["tedge"]), ptr(stru), ptr(g), ptr(ws), ptr(dz))
    torch.cuda.synchronize()
    assert bool((dz == 7.0).all())


def test_captured_row_list_survives_other_lists():
    """The captured epoch holds raw pointers to its row list's structures.  Capture recon_loss forward and backward, score 20
    other row lists (more than the 16 the cache keeps), check that the captured list's cached tensors are still the same
    allocations BEFORE replaying, then replay and compare with an eager run bit for bit."""
    from ggad_amd.model_anomalydae import recon_loss, recon_score
    n, f = 3000, 16
    m, hub, iso, loop_only, zero_row = _loss_graph(n, 5)
    fa = _full(m)
    rows = _rows(n, 300, np.array([hub, iso, loop_only, zero_row]), 3)
    gen = torch.Generator(device=DEV).manual_seed(11)
    z = (torch.randn(n, f, device=DEV, generator=gen) * 0.3).requires_grad_(True)
    xh = torch.randn(n, f, device=DEV, generator=gen).requires_grad_(True)
    x = torch.rand(n, f, device=DEV, generator=gen)

    def step():
        loss, score = recon_loss(z, xh, x, fa, rows)
        gz, gx = torch.autograd.grad(loss, [z, xh])
        return loss.detach(), score, gz, gx

    eager = [t.clone() for t in step()]                              # also the warm-up before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    torch.cuda.synchronize()
    ptrs = _cached_ptrs(fa, rows)
    assert ptrs is not None
    rng = np.random.default_rng(4)
    for k in range(20):
        other = rng.choice(n, 50 + k, replace=False)
        recon_score(z.detach(), xh.detach(), x, fa, other)
    torch.cuda.synchronize()
    assert _cached_ptrs(fa, rows) == ptrs, "the captured row list's structures were evicted"
    graph.replay()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(static, eager)):
        assert _bits_equal(a, b), f"replay differs from the eager run in output {k}"


def _cached_ptrs(fa, rows):
    arr = np.asarray(rows, dtype=np.int64)
    for k, s in fa.__dict__.get("_adae", {}).items():
        if isinstance(k, tuple) and k[0] == "rows" and np.array_equal(s["host"], arr):
            return {name: t.data_ptr() for name, t in s.items() if isinstance(t, torch.Tensor)}
    return None
