"""Shared inputs and the float64 reference of tests/test_explain_cpu.py and tests/test_explain_gpu.py (not a test module itself).

Everything here is built once per session (`functools.lru_cache`) and must be left unchanged by its users.

  * `graph()`: the 3,000-node power-law graph of tests/width_reference.py's recipe plus rows made by hand: an isolated node (closed
    row {i}), a pendant, a node with a self-loop among its columns (closed size = degree), closed rows of exactly 64 and 65 entries,
    one hub of exactly `ggad_explain_lds_rows()` entries and one of that plus 1 (both sizes are asked of the library: the two
    branches of csrc/explain.hip), and the filler nodes the hubs need as neighbours.  Symmetric.
  * `feat(f)`: `synth.make_features` (uniform in [0, 1)), rows scaled to unit L2 norm.  Non-negative on purpose: the aggregate of a
    12,288-entry hub over signed features cancels to about 1 / 110 of its sum of absolute values, and then every tenth ReLU unit of
    a hub row would be undecided (below).
  * `cases()`: the scored list, 457 ids (no multiple of 7 or 150): one id twice inside one slice (positions 2 and 5), one id in two
    slices (10 and 300) with a neighbour beside its first occurrence only, the hubs, the isolated node, a filler and a base neighbour
    of both hubs, the hand-made rows on slice boundaries of batch size 150.
  * `positions(bs)`: the explained positions: first and last position of a slice, the short last slice, both hubs, the isolated
    node, the repeated ids; `positions_twice(bs)`: the same with one position given twice.
  * `reference(d, f, bs, variant)`: per explained position the float64 quantities and the bounds of every float the kernel stores.

Bounds.  Every comparison is |got - float64| <= gamma_n 2^-24-style bounds, gamma_n = n u / (1 - n u), u = 2^-24, n the roundings
on the value's path through the KERNEL'S OWN operation chain (csrc/explain.hip), S the same expression over absolute values:
  omega_ij      4: sqrt(r), 1 / ., sqrt(c), the division
  x1[f]         G1 = 4 + ceil(r / NG) + (NG - 1): omega, the fma chain of one piece of the list, the adds of the NG pieces
                (NG = min(256 / GS, 1024 / F), GS = min(64, the power of two >= F): `x1_terms`)
  a[d]          G1 + F: the fma chain over f
  z             G1 + F + 1 + D: w_d * relu(a_d), D adds.  relu is 1-Lipschitz, so this holds whatever the masks are.
  g[f]          D: the fma chain over d (given equal masks: see `undecided`)
  feature[f]    D + G1 + 1
  t_j           D + F + 4 + 1: g, the fma chain over f, omega, the product
  rest          the t_j's + ceil(r / 256) + 256: one piece, the adds of the 256 pieces
A unit d of a row is UNDECIDED when |a64[d]| <= the bound of a[d]: the float32 mask may then differ from the float64 one, and g, the
features and the t_j with it.  The fixtures are chosen (`DRAW`) so that no explained row has an undecided unit;
tests/test_explain_cpu.py asserts it.  The score of the product path (`score_nodes`, `ResidentSweep.scores`) sums x1 in another order:
its z is bounded with r + 4 + F + 1 + D roundings (tests/width_reference.py: (r + 4) for its x1), and the sigmoid is 1/4-Lipschitz
with 4 roundings of its own (exp, the add, the division, the store) on a value of at most 1.
"""
import functools

import numpy as np

from ggad_amd import _lib, synth
from oracle import ggad_oracle as O

U = 2.0 ** -24
N_BASE = 3000
ISOLATED, PENDANT, ROW64, ROW65, HUB_A, HUB_B = (N_BASE + k for k in range(6))
FILL0 = N_BASE + 6
SELF_LOOP = 77
N_LIST = 457
BATCH_SIZES = (1, 7, 150)


def gam(n):
    return n * U / (1.0 - n * U)


@functools.lru_cache(maxsize=None)
def caps():
    lib = _lib.load()
    return int(lib.ggad_explain_lds_rows()), int(lib.ggad_explain_max_nbrs())


def closed_sizes(rowptr, col):
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    has_self = np.bincount(rows[col == rows], minlength=n) > 0
    return np.diff(rowptr) + 1 - has_self


@functools.lru_cache(maxsize=None)
def graph():
    import scipy.sparse as sp
    cap = caps()[0]
    n_fill = cap - 100 + 10
    n = FILL0 + n_fill
    rowptr, col = synth.make_graph(N_BASE, 45000, 2, kind="powerlaw", max_degree=600)
    rng = np.random.default_rng(43)
    deg = np.diff(rowptr)
    quiet = np.flatnonzero(deg < 40)
    fill = np.arange(FILL0, n)
    hub_a = np.concatenate([np.arange(0, 100), fill[:cap - 1 - 100]])            # cap - 1 columns: closed size cap
    hub_b = np.concatenate([np.arange(50, 150), fill[10:10 + cap - 100]])        # cap columns: closed size cap + 1
    src = [np.repeat(np.arange(N_BASE), deg), [PENDANT], np.full(63, ROW64), np.full(64, ROW65), np.full(len(hub_a), HUB_A),
           np.full(len(hub_b), HUB_B)]
    dst = [col, [3], rng.choice(quiet, 63, replace=False), rng.choice(quiet, 64, replace=False), hub_a, hub_b]
    r, c = np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)
    r, c = np.concatenate([r, c, [SELF_LOOP]]), np.concatenate([c, r, [SELF_LOOP]])
    a = sp.csr_matrix((np.ones(len(r), dtype=np.int8), (r, c)), shape=(n, n))
    a.sum_duplicates()
    a.sort_indices()
    rowptr, col = a.indptr.astype(np.int32), a.indices.astype(np.int32)
    closed = closed_sizes(rowptr, col)
    deg = np.diff(rowptr)
    assert deg[ISOLATED] == 0 and closed[ISOLATED] == 1 and closed[PENDANT] == 2
    assert closed[SELF_LOOP] == deg[SELF_LOOP] and closed[ROW64] == 64 and closed[ROW65] == 65
    assert closed[HUB_A] == cap and closed[HUB_B] == cap + 1 and closed.max() == cap + 1
    for x in (rowptr, col):
        x.setflags(write=False)
    return rowptr, col


def n_nodes():
    return len(graph()[0]) - 1


@functools.lru_cache(maxsize=None)
def feat(f):
    x = synth.make_features(n_nodes(), f, 11 + f).astype(np.float64) + 1e-3
    x = (x / np.sqrt((x * x).sum(1, keepdims=True))).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(17)
    ids = rng.choice(N_BASE, N_LIST, replace=False).astype(np.int64)
    ids[5] = ids[2]                                  # one id twice inside one slice (batch sizes 7 and 150)
    ids[300] = ids[10]                               # one id in two slices
    ids[20], ids[160] = HUB_A, HUB_B
    ids[19] = 60                                     # a base neighbour of both hubs, in hub A's slice at every batch size above 1
    rowptr, col = graph()
    ids[11] = col[rowptr[ids[10]]]                   # a neighbour of the id of two slices, beside its first occurrence only
    ids[25] = ISOLATED
    ids[30] = FILL0 + 12                             # a filler: its closed row is {itself, hub A, hub B}
    ids[149], ids[150], ids[299] = PENDANT, ROW64, ROW65      # last of slice 0, first of slice 1, last of slice 1 at batch size 150
    ids[N_LIST - 1] = SELF_LOOP                      # the short last slice
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def positions(bs):
    last0 = N_LIST - (N_LIST % bs or bs)             # first position of the last slice
    want = [0, bs - 1, bs, 2 * bs - 1, last0, N_LIST - 1, 2, 5, 10, 300, 20, 160, 25, 149, 150, 299, 30, 19]
    out = []
    for p in want:
        if 0 <= p < N_LIST and p not in out:
            out.append(p)
    return tuple(out)


def positions_twice(bs):
    p = positions(bs)
    return p + (p[3],)


# ------------------------------------------------------------------ parameters
# (d, f) -> draw: the first draw of the signed parameters at which no explained row of any batch size has an undecided unit (the
# inputs are chosen so that the condition holds; the condition is not fitted to the inputs)
DRAW = {}
VARIANTS = ("signed", "dead")


@functools.lru_cache(maxsize=None)
def params(d, f, variant="signed", draw=None):
    """(w (1, d), W (d, f), fc (d, d)) float32.  `signed`: uniform in [-1, 1] scaled like xavier.  `dead`: w and W all negative:
    with the non-negative features every unit of every row is off, z = 0 and every contribution is 0."""
    draw = DRAW.get((d, f), 0) if draw is None else draw
    rng = np.random.default_rng(9000 + 1000 * draw + 7 * d + f)
    w = rng.uniform(-1.0, 1.0, (1, d)) * np.sqrt(6.0 / (1 + d))
    W = rng.uniform(-1.0, 1.0, (d, f)) * np.sqrt(6.0 / (d + f))
    fc = rng.uniform(-1.0, 1.0, (d, d)) * np.sqrt(3.0 / d)
    if variant == "dead":
        w, W = -np.abs(w) - 1e-3, -np.abs(W) - 1e-3
    out = tuple(np.ascontiguousarray(x, dtype=np.float32) for x in (w, W, fc))
    for x in out:
        x.setflags(write=False)
    return out


# ------------------------------------------------------------------ the float64 reference
def x1_terms(r, f):
    """Roundings on x1[f] in csrc/explain.hip: omega (4), the fma chain of one piece of the list (ceil(r / NG)), the adds of the NG
    pieces (NG - 1)."""
    gs = 1
    while gs < f and gs < 64:
        gs *= 2
    ng = min(256 // gs, max(1, 1024 // f))
    return 4 + -(-r // ng) + (ng - 1)


@functools.lru_cache(maxsize=None)
def rows(f, bs):
    """Per explained position of `positions(bs)`: node, ids of the closed row (ascending), c_j, omega (float64), x1, S of x1, the
    closed rows' features; from `oracle.aggregate_batch(..., dtype=np.float64)` over the position's slice."""
    rowptr, col = graph()
    x = feat(f)
    ids = cases()
    by_slice = {}
    out = {}
    for p in positions(bs):
        s0 = p - p % bs
        if s0 not in by_slice:
            nodes = ids[s0:min(N_LIST, s0 + bs)]
            a64 = O.aggregate_batch(rowptr, col, x, nodes, False, dtype=np.float64)
            by_slice[s0] = (a64, np.bincount(a64.ent_pos, minlength=len(a64.unique)))
        a64, cnt = by_slice[s0]
        b = p - s0
        e = a64.ent_pos[a64.ent_ptr[b]:a64.ent_ptr[b + 1]]
        nbr = a64.unique[e].astype(np.int64)
        assert (np.diff(nbr) > 0).all() and int(ids[p]) in nbr
        c = cnt[e].astype(np.int64)
        r = len(nbr)
        om = (1.0 / np.sqrt(float(r))) / np.sqrt(c.astype(np.float64))
        fj = x[nbr].astype(np.float64)
        x1 = (om[:, None] * fj).sum(0)
        assert np.allclose(x1, a64.to_feats[b], rtol=1e-13, atol=1e-300)
        out[p] = dict(node=int(ids[p]), nbr=nbr, c=c, r=r, om=om, fj=fj, x1=a64.to_feats[b], s_x1=(om[:, None] * np.abs(fj)).sum(0))
    return out


@functools.lru_cache(maxsize=None)
def reference(d, f, bs, variant="signed", draw=None):
    """Per explained position: the row data of `rows` plus a, mask, g, z, per-feature and per-neighbour contributions (float64), their
    S, and the bounds of the module docstring: b_a, undecided, b_z, b_feature, b_t, and `b_score_z` (the product path's z)."""
    w, W, _ = params(d, f, variant, draw)
    w, W = w.reshape(-1).astype(np.float64), W.astype(np.float64)
    out = {}
    for p, row in rows(f, bs).items():
        r, om, fj, x1, s_x1 = row["r"], row["om"], row["fj"], row["x1"], row["s_x1"]
        g1 = x1_terms(r, f)
        a = W @ x1
        s_a = np.abs(W) @ s_x1
        b_a = gam(g1 + f) * s_a
        mask = a > 0
        z = float((w * np.maximum(a, 0.0)).sum())
        s_z = float((np.abs(w) * s_a).sum())
        g = (w * mask) @ W
        s_g = (np.abs(w) * mask) @ np.abs(W)
        feature = g * x1
        t = om * (fj @ g)
        s_t = om * (np.abs(fj) @ s_g)
        out[p] = dict(row, a=a, mask=mask, g=g, z=z, feature=feature, t=t, s_a=s_a, s_z=s_z, s_g=s_g, s_feature=s_g * s_x1, s_t=s_t,
                      b_a=b_a, undecided=np.abs(a) <= b_a, b_z=gam(g1 + f + 1 + d) * s_z, b_feature=gam(d + g1 + 1) * s_g * s_x1,
                      b_t=gam(d + f + 5) * s_t, rest_terms=d + f + 5 + -(-r // 256) + 256,
                      b_score_z=gam(r + 4 + f + 1 + d) * s_z)
    return out


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, dtype=np.float64)))


def shapes():
    """(d, f) over the branch points the engine accepts: d in {1, 64, 65, 256} x f in {1, 17}, plus the widest f the narrow engine
    takes at d = 64 (asked of the library, as minibatch.py asks it)."""
    lib = _lib.load()
    f_max = max(f for f in range(1, int(lib.ggad_max_feat_dim()) + 1) if lib.ggad_mb_supported(64, f))
    out = [(d, f) for d in (1, 64, 65, 256) for f in (1, 17)] + [(64, f_max)]
    for d, f in out:
        wide = d > int(lib.ggad_max_embed_dim())
        assert lib.ggad_mb_wide_supported(d, f) if wide else lib.ggad_mb_supported(d, f), (d, f)
    return out
