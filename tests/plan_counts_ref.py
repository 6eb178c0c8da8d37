"""Exact integers of the mini-batch plan: a numpy restatement of what `k_tile_counts`, `k_gather1c`, `k_seg_transpose` and
`k_build_groups` (csrc/plan.hip, csrc/hop2_ldsw.hip) leave in the plan's tables, and the table of graphs built to reach their
branches.  No torch on the reference side; `assert_plan_integers_exact` reads a built `BatchChunk` and compares with `==`.

What is fixed by the batch alone is compared element for element (counts, degrees, row starts, segment bounds, totals); what an
atomic hands out (`pw_base`, group ids, item positions) is compared as sets / disjoint intervals.

The thresholds the case table aims at are read from the sources (each pattern must match exactly once) or asked of the library,
never typed in: a changed constant moves the table with it or fails it loudly."""
import functools
import os
import re
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ggad_amd", "csrc")
F = 17


# ------------------------------------------------------------------ constants
def _once(text, pattern, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, f"{what}: pattern {pattern!r} matches {len(found)} times"
    return int(found[0])


SOURCE_PATTERNS = {
    "hop2_ldsw.hip": {
        "TW_T": r"constexpr int TW_T = (\d+);",
        "CACHE_IT": r"constexpr int CACHE_IT = (\d+);",
        "TW_BRK": r"constexpr int TW_BRK = (\d+);",
    },
    "common.h": {
        "CTR_STRIDE": r"constexpr int GGAD_CTR_STRIDE = (\d+);",
        "CTR_GROUPS": r"GGAD_CTR_GROUPS = (\d+) \* GGAD_CTR_STRIDE",
        "CTR_ITEMS": r"GGAD_CTR_ITEMS = (\d+) \* GGAD_CTR_STRIDE",
        "CTR_PART": r"GGAD_CTR_PART = (\d+) \* GGAD_CTR_STRIDE",
        "CTR_CURSOR": r"GGAD_CTR_CURSOR = (\d+) \* GGAD_CTR_STRIDE",
        "CTR_PC": r"GGAD_CTR_PC = (\d+) \* GGAD_CTR_STRIDE",
        "CTR_BIG": r"GGAD_CTR_BIG = (\d+) \* GGAD_CTR_STRIDE",
        "RANGES": r"constexpr int GGAD_RANGES = (\d+);",
        "RANGE_DEG": r"constexpr int GGAD_RANGE_DEG = (\d+);",
    },
}


@functools.lru_cache(maxsize=None)
def constants():
    from ggad_amd import _lib
    lib = _lib.load()
    c = {}
    for fname, pats in SOURCE_PATTERNS.items():
        with open(os.path.join(CSRC, fname)) as fh:
            text = fh.read()
        for name, pat in pats.items():
            c[name] = _once(text, pat, f"{fname}: {name}")
    for name in ("CTR_GROUPS", "CTR_ITEMS", "CTR_PART", "CTR_CURSOR", "CTR_PC", "CTR_BIG"):
        c[name] *= c["CTR_STRIDE"]
    c["SHIFT"] = int(lib.ggad_mb_ldsw_tile_shift())
    c["TILE"] = 1 << c["SHIFT"]
    c["MAXOWN"] = int(lib.ggad_mb_ldsw_max_owners())
    c["SLICE"] = int(lib.ggad_mb_slice_len())
    c["GRP_W"] = int(lib.ggad_mb_group_words())
    assert c["GRP_W"] == 10, "group record: 8 owner entries, partial-slot base, slices"
    return SimpleNamespace(**c)


def n_tiles_of(n):
    C = constants()
    return (n + C.TILE - 1) >> C.SHIFT


# ------------------------------------------------------------------ the restatement
def closed_rows(rowptr, col, nodes):
    """Sorted closed neighbourhood N(v) + {v} of every batch node, as the plan lays its entries out."""
    out = []
    for v in np.asarray(nodes, dtype=np.int64):
        r = col[rowptr[v]:rowptr[v + 1]].astype(np.int64)
        i = int(np.searchsorted(r, v))
        out.append(r if (i < len(r) and r[i] == v) else np.insert(r, i, v))
    return out


def rows_of(rowptr, col, nodes):
    """(ptr, ids): the CSR rows of `nodes`, concatenated."""
    nodes = np.asarray(nodes, dtype=np.int64)
    deg = rowptr[nodes + 1].astype(np.int64) - rowptr[nodes].astype(np.int64)
    ptr = np.concatenate(([0], np.cumsum(deg)))
    idx = np.repeat(rowptr[nodes].astype(np.int64) - ptr[:-1], deg) + np.arange(ptr[-1], dtype=np.int64)
    return ptr, col[idx].astype(np.int64)


def pair_counts(rowptr, col, batches):
    """Per batch: owners U_b (sorted distinct columns of the closed neighbourhoods), `ptr` of their rows, and for every owner the
    vector c'[col[rowptr[u]:rowptr[u + 1]]] with c'_k = #{u' in U_b : k in N(u')}, laid out like the owner's CSR row; `ids` are the
    neighbour ids beside the counts."""
    out = []
    for nodes in batches:
        U = np.unique(np.concatenate(closed_rows(rowptr, col, nodes)))
        ptr, ids = rows_of(rowptr, col, U)
        u2, inv = np.unique(ids, return_inverse=True)
        c2 = np.bincount(inv, minlength=len(u2)).astype(np.int64)
        out.append(SimpleNamespace(U=U, ptr=ptr, cp=c2[inv], ids=ids))
    return out


def x2_from_counts(feat, bc):
    """float64 x2 of every owner of one batch from the reference counts (a degree-0 owner: NaN, the dense 0/0 row)."""
    feat = np.asarray(feat, dtype=np.float64)
    deg = np.diff(bc.ptr)
    owner = np.repeat(np.arange(len(bc.U)), deg)
    w = 1.0 / np.sqrt(deg[owner].astype(np.float64)) / np.sqrt(bc.cp.astype(np.float64))
    out = np.empty((len(bc.U), feat.shape[1]), dtype=np.float64)
    for f in range(feat.shape[1]):
        out[:, f] = np.bincount(owner, weights=w * feat[bc.ids, f], minlength=len(bc.U))
    out[deg == 0] = np.nan
    return out


def tile_offsets(rowptr, col, nodes, n_tiles):
    """tile_off rows of `nodes`: positions in the CSR row where the neighbour ids cross a tile boundary, int64[len][n_tiles + 1]."""
    C = constants()
    ptr, ids = rows_of(rowptr, col, nodes)
    owner = np.repeat(np.arange(len(nodes), dtype=np.int64), np.diff(ptr))
    cnt = np.bincount(owner * n_tiles + (ids >> C.SHIFT), minlength=len(nodes) * n_tiles).reshape(len(nodes), n_tiles)
    return np.concatenate((np.zeros((len(nodes), 1), dtype=np.int64), np.cumsum(cnt, axis=1)), axis=1)


def tile_starts(rowptr, col, n, n_tiles):
    """tile_start of the whole graph: where segment (u, t) begins in the tile-major copy of col; last column 0."""
    off = tile_offsets(rowptr, col, np.arange(n), n_tiles)
    lens = np.diff(off, axis=1)
    base = np.concatenate(([0], np.cumsum(lens.sum(axis=0))))[:-1]
    start = base[None, :] + np.cumsum(lens, axis=0) - lens
    return np.concatenate((start, np.zeros((n, 1), dtype=np.int64)), axis=1)


def group_plan(owner_cols, rowptr, range_deg):
    """What k_build_groups must produce for the chunk whose owner entries have the columns `owner_cols`: per node m_u, groups
    ng = ceil(m_u / 8), slices ns, and the totals of the plan counters."""
    C = constants()
    nodes, m = np.unique(np.asarray(owner_cols, dtype=np.int64), return_counts=True)
    deg = rowptr[nodes + 1].astype(np.int64) - rowptr[nodes].astype(np.int64)
    ng = (m + 7) // 8
    big = deg > range_deg
    ns = np.where(big, C.RANGES, np.where(deg > C.SLICE, (deg + C.SLICE - 1) // C.SLICE, 1))
    return SimpleNamespace(nodes=nodes, m=m, deg=deg, ng=ng, ns=ns, big=big,
                           GROUPS=int(ng.sum()), ITEMS=int((ng * ns)[~big].sum()), BIG=int(ng[big].sum()),
                           PART=int((m * ns)[ns > 1].sum()), PC=int((m * deg).sum()))


def effective_range_deg(option):
    """The threshold the library derives from `ggad_mb_set_gather_options(-1, option)`: off (no owner is big) at 0."""
    C = constants()
    return max(int(option), C.RANGE_DEG) if option > 0 else 2 ** 31 - 1


# ------------------------------------------------------------------ the check of a built chunk
def assert_plan_integers_exact(ch, rowptr, col, batches, range_deg, only_batches=None):
    """`ch`: a BatchChunk built on `batches` with the LDS-counting 2-hop stage.  `range_deg`: the effective big-owner threshold
    (`effective_range_deg`).  `only_batches`: check the per-batch tables of these batches only and, of the chunk-wide checks, the
    counters (full-size chunks)."""
    C = constants()
    assert ch.last_hop2 == "ldsw"
    rowptr = np.asarray(rowptr)
    col = np.asarray(col)
    n = len(rowptr) - 1
    nt = n_tiles_of(n)
    ne = ch.n_ents
    rp64 = rowptr.astype(np.int64)
    ent_col = ch.ent_col[:ne].cpu().numpy().astype(np.int64)
    ent_own = ch.ent_own[:ne].cpu().numpy().astype(np.int64)
    own_deg = ch.own_deg[:ne].cpu().numpy().astype(np.int64)
    own_rp = ch.own_rp[:ne].cpu().numpy().astype(np.int64)
    pw_base = ch.pw_base[:ne].cpu().numpy().astype(np.int64)
    counters = ch.counters.cpu().numpy().astype(np.int64)
    is_own = ent_own == np.arange(ne)
    deg_ref = np.where(is_own, rp64[ent_col + 1] - rp64[ent_col], 0)
    assert np.array_equal(own_deg, deg_ref), "own_deg"
    assert np.array_equal(own_rp, np.where(is_own, rp64[ent_col], 0)), "own_rp"
    # pc[] storage: disjoint intervals inside [0, PC), PC = every owner's degree once
    PC = int(counters[C.CTR_PC])
    assert PC == int(deg_ref.sum()), ("counters[PC]", PC, int(deg_ref.sum()))
    oe = np.nonzero(is_own & (deg_ref > 0))[0]
    if len(oe):
        o = np.argsort(pw_base[oe], kind="stable")
        lo, ln = pw_base[oe][o], deg_ref[oe][o]
        assert lo[0] >= 0 and (lo[:-1] + ln[:-1] <= lo[1:]).all() and lo[-1] + ln[-1] <= PC, "pw_base intervals overlap or leave [0, PC)"
    pc = ch.pc[:PC].cpu().numpy().view(np.uint16).astype(np.int64)
    stride = (ne + 63) // 64 * 64
    tile_major = ch.plan.col_t is not None
    planes = ch.seg_t[:(2 if tile_major else 1) * (nt + 1) * stride].view(-1, nt + 1, stride)
    tstart = tile_starts(rowptr, col, n, nt) if tile_major else None
    which = range(len(batches)) if only_batches is None else only_batches
    ref = pair_counts(rowptr, col, [batches[b] for b in which])
    for bc, b in zip(ref, which):
        e0, e1 = ch.batch_ents(b)
        ents = np.arange(e0, e1)[is_own[e0:e1]]
        cols = ent_col[ents]
        o = np.argsort(cols, kind="stable")
        assert np.array_equal(cols[o], bc.U), f"batch {b}: the owner entries are not the distinct columns, each once"
        ents = ents[o]
        deg = np.diff(bc.ptr)
        within = np.arange(bc.ptr[-1]) - np.repeat(bc.ptr[:-1], deg)
        got = pc[np.repeat(pw_base[ents], deg) + within]
        if not np.array_equal(got, bc.cp):
            bad = np.nonzero(got != bc.cp)[0]
            i = int(bad[0])
            u = int(bc.U[np.searchsorted(bc.ptr, i, side="right") - 1])
            raise AssertionError(f"batch {b}: {len(bad)} of {len(got)} pair counts differ; first: owner {u}, neighbour {int(bc.ids[i])}, "
                                 f"pc {int(got[i])} != c' {int(bc.cp[i])}")
        # segment bounds, tile-major: seg_t[t][e] = tile_off[ent_col[e]][t] for owners, 0 for the other entries
        ucols, inv = np.unique(ent_col[e0:e1], return_inverse=True)
        toff = tile_offsets(rowptr, col, ucols, nt)
        own_b = is_own[e0:e1]
        seg = planes[0, :, e0:e1].cpu().numpy().astype(np.int64)
        assert np.array_equal(seg, np.where(own_b[None, :], toff[inv].T, 0)), f"batch {b}: seg_t"
        if tile_major:
            seg = planes[1, :, e0:e1].cpu().numpy().astype(np.int64)
            assert np.array_equal(seg, np.where(own_b[None, :], tstart[ent_col[e0:e1]].T, 0)), f"batch {b}: seg_t, tile_start plane"
    # plan counters and work lists
    gp = group_plan(ent_col[is_own], rowptr, range_deg)
    assert gp.PC == PC
    lists = bool(ch.node_major) and ch.F <= 64
    got = {k: int(counters[getattr(C, "CTR_" + k)]) for k in ("GROUPS", "ITEMS", "BIG", "PART")}
    want = {k: (getattr(gp, k) if lists else 0) for k in got}
    assert got == want, ("plan counters", got, want)
    assert int(ch.node_head.abs().sum()) == 0, "node_head is not clean"
    if not lists or only_batches is not None:
        return
    W, R = C.GRP_W, C.RANGES
    grp = ch.grp[:gp.GROUPS * W].cpu().numpy().astype(np.int64).reshape(gp.GROUPS, W)
    slots = grp[:, :8]
    filled = slots >= 0
    assert np.array_equal(np.sort(slots[filled]), np.nonzero(is_own)[0]), "group slots are not the owner entries, each once"
    assert filled[:, 0].all()
    rec_node = ent_col[slots[:, 0]]
    assert (~filled | (ent_col[np.where(filled, slots, 0)] == rec_node[:, None])).all(), "a group record mixes columns"
    n_occ = filled.sum(axis=1)
    ni = np.searchsorted(gp.nodes, rec_node)
    assert np.array_equal(np.bincount(ni, minlength=len(gp.nodes)), gp.ng), "groups per node"
    assert (np.bincount(ni, weights=(n_occ < 8), minlength=len(gp.nodes)) <= 1).all(), "more than one partial group of a node"
    assert np.array_equal(grp[:, 9], gp.ns[ni]), "rec[9] != ns"
    multi = np.nonzero(grp[:, 9] > 1)[0]
    if len(multi):
        o = multi[np.argsort(grp[multi, 8], kind="stable")]
        lo, ln = grp[o, 8], n_occ[o] * grp[o, 9]
        assert lo[0] >= 0 and (lo[:-1] + ln[:-1] <= lo[1:]).all() and lo[-1] + ln[-1] <= gp.PART, "partial-sum slots overlap or leave [0, PART)"
    cap = int(ch.item_cap)
    all_items = ch.items
    items = all_items[:2 * gp.ITEMS].cpu().numpy().astype(np.int64).reshape(gp.ITEMS, 2)
    rec_big = gp.big[ni]
    small = np.nonzero(~rec_big)[0]
    mx = int(gp.ns.max(initial=1)) + 1
    want_keys = np.repeat(small, grp[small, 9]) * mx + (np.arange(gp.ITEMS) - np.repeat(np.cumsum(grp[small, 9]) - grp[small, 9], grp[small, 9]))
    assert ((items[:, 1] >= 0) & (items[:, 1] < mx) & (items[:, 0] >= 0) & (items[:, 0] < gp.GROUPS)).all(), "item out of range"
    assert np.array_equal(np.sort(items[:, 0] * mx + items[:, 1]), np.sort(want_keys)), "items are not {(g, s)}, each once"
    if gp.ITEMS:
        inode = ni[items[:, 0]]
        starts = np.concatenate(([0], np.nonzero(np.diff(inode))[0] + 1))
        assert len(starts) == len(np.unique(inode)), "the items of a node are not consecutive"
        rank = np.arange(gp.ITEMS) - np.repeat(starts, np.diff(np.concatenate((starts, [gp.ITEMS]))))
        assert np.array_equal(items[:, 1], rank // gp.ng[inode]), "the items of a node are not slice-major"
    big = all_items[2 * cap:2 * cap + gp.BIG].cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(big), np.nonzero(rec_big)[0]), "big list is not the groups of the big nodes, each once"
    if gp.BIG:
        gbnd = all_items[3 * cap:3 * cap + gp.BIG * (R + 1)].cpu().numpy().astype(np.int64).reshape(gp.BIG, R + 1)
        toff = tile_offsets(rowptr, col, gp.nodes, nt)
        at = (np.arange(R + 1) * nt) // R
        assert np.array_equal(gbnd, toff[ni[big]][:, at]), "gbnd rows"


# ------------------------------------------------------------------ graphs by construction
def csr_from_edges(n, edges):
    """Symmetric CSR with sorted rows from undirected edges (no self loops; duplicates merged)."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    assert (e[:, 0] != e[:, 1]).all() and e.min(initial=0) >= 0 and e.max(initial=0) < n
    key = np.unique(np.concatenate((e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0])))
    src, dst = key // n, key % n
    rowptr = np.concatenate(([0], np.cumsum(np.bincount(src, minlength=n))))
    return rowptr.astype(np.int32), dst.astype(np.int32)


def features(n, seed):
    """Signed features of unit scale: sums of thousands of them cancel, so x2 stays O(1) at every degree of the table."""
    return (np.random.default_rng(seed).standard_normal((n, F)) * 0.25).astype(np.float32)


def hub_block(v, owners, ext_owners, n_extra, non_owners):
    """Batch node v adjacent to `owners` (the owners of batch [v]); extra edge i joins ext_owners[i % k] and non_owners[i // k]: one
    pair in the tile of the non-owner each, and c' = k at every non-owner but the last."""
    owners = np.asarray(owners, dtype=np.int64)
    ed = [np.stack((np.full(len(owners), v, dtype=np.int64), owners), axis=1)]
    if n_extra:
        ext = np.asarray(ext_owners, dtype=np.int64)
        i = np.arange(n_extra)
        assert len(non_owners) > (n_extra - 1) // len(ext)
        ed.append(np.stack((ext[i % len(ext)], np.asarray(non_owners, dtype=np.int64)[i // len(ext)]), axis=1))
    return np.concatenate(ed)


class _Ids:
    def __init__(self, first):
        self.next = first

    def take(self, k=1):
        a = np.arange(self.next, self.next + k, dtype=np.int64)
        self.next += k
        return a


def _finish(n, edges, seed):
    rowptr, col = csr_from_edges(n, np.concatenate(edges) if edges else np.zeros((0, 2), dtype=np.int64))
    return SimpleNamespace(n=n, rowptr=rowptr, col=col, feat=features(n, seed))


def pair_targets():
    """P of one (tile, batch) -> the branch of k_tile_counts it is the smallest / largest size of."""
    C = constants()
    T, K = C.TW_T, C.CACHE_IT
    return {0: "P=0: an empty tile next to a non-empty one", 1: "P=1: single pair",
            T: "P=TW_T: first trip full", T + 1: "P=TW_T+1: second trip",
            4 * T: "P=4 TW_T: first group of four cached trips full", 4 * T + 1: "P=4 TW_T+1: second group of four cached trips",
            K * T: "P=CACHE_IT TW_T: cache exactly full, tail loop not entered", K * T + 1: "P=CACHE_IT TW_T+1: tail loop entered",
            (K + 4) * T + 1: "P=(CACHE_IT+4) TW_T+1: second trip of the tail loop",
            64 * (C.TW_BRK - 1): "P=64 (TW_BRK-1): last size with the bracket table", 64 * (C.TW_BRK - 1) + 1: "P=64 (TW_BRK-1)+1: full descent"}


@functools.lru_cache(maxsize=None)
def graph_pairs():
    """3 tiles, the last partial.  Tile 0: hubs and their owners; tile 1: the non-owners every extra edge goes to; tile 2: untouched.
    Batch b = [hub b]: P(tile 0) = 2 m, P(tile 1) = the target, P(tile 2) = 0."""
    C = constants()
    T = C.TILE
    n = 2 * T + 1000
    ids = _Ids(5)
    non = np.concatenate(([T, 2 * T - 1], np.arange(T + 1, 2 * T - 1)))      # first and last id of the tile first
    edges, hubs, decl = [], [], []
    for P in pair_targets():
        m = 37 if P <= 4 * C.TW_T + 1 else (301 if P < 64 * (C.TW_BRK - 1) else 400)
        v, owners = int(ids.take()[0]), ids.take(m)
        edges.append(hub_block(v, owners, owners, P, non))
        hubs.append(v)
        decl.append(dict(P={0: 2 * m, 1: P, 2: 0}, n_own=m + 1, max_count=max(m, min(m, P))))
    # brackets: owners holding > 128 consecutive pairs each (neighbouring brackets equal: descent width 0)
    v, owners = int(ids.take()[0]), ids.take(64)
    edges.append(hub_block(v, owners, owners, 64 * 1500, non))
    hubs.append(v)
    decl.append(dict(P={0: 128, 1: 96000, 2: 0}, n_own=65, max_count=64))
    # brackets: 258 owners with empty segments in tile 1 between two non-empty ones
    v, owners = int(ids.take()[0]), ids.take(260)
    edges.append(hub_block(v, owners, owners[[0, -1]], 600, non))
    hubs.append(v)
    decl.append(dict(P={0: 520, 1: 600, 2: 0}, n_own=261, max_count=260))
    g = _finish(n, edges, 11)
    g.hubs, g.decl = hubs, decl
    return g


SLAB_OWNERS = (1, 62, 63, 64)      # + the hub itself: batches of 2, 63, 64 and 65 entries


@functools.lru_cache(maxsize=None)
def graph_slabs():
    """2 tiles (the second partial).  Hubs with 1, 62, 63, 64, MAXOWN - 1, MAXOWN and 3 MAXOWN + 68 owners and an isolated node."""
    C = constants()
    T, M = C.TILE, C.MAXOWN
    n = T + 500
    ids = _Ids(2)
    non = np.arange(T, n)
    g_edges, hubs, decl = [], {}, {}
    for m in SLAB_OWNERS + (M - 1, M):
        v, owners = int(ids.take()[0]), ids.take(m)
        g_edges.append(hub_block(v, owners, owners, 2 * m if m >= M - 1 else m, non))
        hubs[m + 1] = v
        decl[m + 1] = dict(P={0: 2 * m, 1: 2 * m if m >= M - 1 else m}, n_own=m + 1, max_count=m)
    m = 3 * M + 68
    v, owners = int(ids.take()[0]), ids.take(m)
    ext = np.concatenate((owners[:M - 1], owners[2 * M - 1:]))      # entries [M, 2 M) = owners [M - 1, 2 M - 1): no pair in tile 1
    g_edges.append(hub_block(v, owners, ext, len(ext), non))
    hubs["slabs"] = v
    decl["slabs"] = dict(P={0: 2 * m, 1: len(ext)}, n_own=m + 1, max_count=m, slab_P={(0, 1): M - 1, (1, 1): 0, (2, 1): M, (3, 1): 69})
    assert ids.next < T - 1
    hubs["iso"] = T - 1                                             # isolated: degree 0, one entry, P = 0 everywhere, x2 NaN
    decl["iso"] = dict(P={0: 0, 1: 0}, n_own=1, max_count=0)
    g = _finish(n, g_edges, 12)
    g.hubs, g.decl = hubs, decl
    return g


@functools.lru_cache(maxsize=None)
def graph_star(L):
    """Two centres a (even) and a + 1, not adjacent, L leaves adjacent to both; every other id is a leaf: 0, TILE - 1, TILE and
    n - 1 (in the partial last tile) among them.  Batch [a]: L + 1 entries, c'_a = c'_{a+1} = L in the two halves of one LDS word."""
    n = L + 2
    a = 1000
    leaves = np.concatenate((np.arange(0, a), np.arange(a + 2, n)))
    edges = [np.stack((np.full(L, a), leaves), axis=1), np.stack((np.full(L, a + 1), leaves), axis=1)]
    g = _finish(n, edges, 13)
    g.a, g.L = a, L
    return g


OCC = (8, 9, 16, 17)


@functools.lru_cache(maxsize=None)
def graph_occ():
    """17 batches [hub b]; node w_j is an owner in the first j of them (j = 8, 9, 16, 17: one full group, 8 + 1, two full, 16 + 1);
    hub b has 2 b filler owners besides, and every w and filler is adjacent to the non-owner z: c'_z differs in every batch."""
    n = 2000
    ids = _Ids(1)
    z = 1999
    w = {j: int(ids.take()[0]) for j in OCC}
    edges, hubs, cz = [], [], []
    for b in range(17):
        v = int(ids.take()[0])
        fill = ids.take(2 * b)
        owners = np.array(sorted([w[j] for j in OCC if b < j] + list(fill)), dtype=np.int64)
        edges.append(hub_block(v, owners, owners, len(owners), [z]))
        hubs.append(v)
        cz.append(len(owners))
    g = _finish(n, edges, 14)
    g.hubs, g.w, g.z, g.cz = hubs, w, z, cz
    assert len(set(cz)) == 17
    return g


OWNER_DEGREES = (0, 1, 256, 257, 512, 513)


@functools.lru_cache(maxsize=None)
def graph_degrees():
    """One tile.  Hub v whose owners have 1, SLICE, SLICE + 1, 2 SLICE and 2 SLICE + 1 neighbours; an isolated node (0) beside it in
    the batch; a second hub shares the owners, so each is an owner twice."""
    C = constants()
    S = C.SLICE
    degs = (1, S, S + 1, 2 * S, 2 * S + 1)
    assert (0,) + degs == OWNER_DEGREES and S == C.RANGE_DEG
    n = 3000
    ids = _Ids(1)                                                  # (node 0: isolated)
    v, v2 = int(ids.take()[0]), int(ids.take()[0])
    owners = ids.take(len(degs))
    non = np.arange(1000, 2000)
    edges = [hub_block(v, owners, [], 0, non)]
    edges.append(np.stack((np.full(len(degs) - 1, v2), owners[1:]), axis=1))      # (every owner but the first: degree + 1 below)
    for u, d in zip(owners, degs):
        k = d - 1 if d == 1 else d - 2
        edges.append(np.stack((np.full(k, u), non[:k]), axis=1))
    g = _finish(n, edges, 15)
    g.v, g.v2, g.iso, g.owners, g.degs = v, v2, 0, owners, degs
    return g


@functools.lru_cache(maxsize=None)
def graph_tiles(full_tiles):
    """`full_tiles` whole tiles and a last one of 5 nodes; few edges.  Hub 3 has one owner in every tile; the owners reach the first
    and the last id of every tile and n - 1; one owner has 600 neighbours spread over all tiles; a second hub shares the owners."""
    C = constants()
    T = C.TILE
    n = full_tiles * T + 5
    nt = full_tiles + 1
    v, v2 = 3, 4
    owners = np.array([t * T + 7 for t in range(nt - 1)] + [n - 2], dtype=np.int64)
    corner = np.array(sorted({t * T for t in range(nt)} | {t * T + T - 1 for t in range(nt - 1)} | {n - 1}), dtype=np.int64)
    edges = [hub_block(v, owners, [], 0, []), hub_block(v2, owners[::2], [], 0, [])]
    for i, u in enumerate(owners):
        edges.append(np.stack((np.full(len(corner) - i, u), corner[i:]), axis=1))
    wide = np.linspace(100, n - 100, 600).astype(np.int64)
    edges.append(np.stack((np.full(600, owners[1]), wide), axis=1))
    g = _finish(n, edges, 16 + full_tiles)
    g.v, g.v2, g.owners, g.nt = v, v2, owners, nt
    return g


# ------------------------------------------------------------------ the case table
def _case(graph, batches, reaches, hop2="ldsw", **declares):
    return dict(graph=graph, batches=[np.asarray(b, dtype=np.int64) for b in batches], reaches=tuple(reaches), hop2=hop2, declares=declares)


def _build_cases():
    C = constants()
    cases = {}
    gp = graph_pairs
    labels = list(pair_targets().values()) + ["brackets: one owner holds > 128 consecutive pairs (width 0)",
                                              "brackets: >= 200 owners with empty segments between two non-empty ones"]
    cases["pairs"] = lambda: _case(gp, [[h] for h in gp().hubs], labels + ["tiles: 3, the last partial"],
                                   P={(t, b): p for b, d in enumerate(gp().decl) for t, p in d["P"].items()},
                                   n_own={b: d["n_own"] for b, d in enumerate(gp().decl)}, max_count=400, n_tiles=3)
    cases["pairs_single"] = lambda: _case(gp, [[gp().hubs[1]]], ["rebuild: a smaller chunk after a larger one"],
                                          P={(1, 0): 1}, n_own={0: 38}, max_count=37, n_tiles=3)
    gs = graph_slabs
    for k, label in [(1, "n_own=1: an isolated node"), (2, "n_own=2"), (63, "n_own=63"), (64, "n_own=64"), (65, "n_own=65"),
                     (C.MAXOWN, "n_own=TW_MAXOWN: one slab"), (C.MAXOWN + 1, "n_own=TW_MAXOWN+1: a second slab of one entry")]:
        key = "iso" if k == 1 else k
        cases[f"own{k}"] = (lambda key=key, label=label: _case(
            gs, [[gs().hubs[key]]], [label], P={(t, 0): p for t, p in gs().decl[key]["P"].items()},
            n_own={0: gs().decl[key]["n_own"]}, max_count=gs().decl[key]["max_count"], n_tiles=2,
            deg={gs().hubs[key]: 0} if key == "iso" else {}))
    cases["slabs"] = lambda: _case(gs, [[gs().hubs["slabs"]], [gs().hubs[2]]], ["n_own: four slabs, one of them with P=0 in a tile"],
                                   P={(0, 0): 2 * (3 * C.MAXOWN + 68), (1, 0): 2 * C.MAXOWN + 68}, n_own={0: 3 * C.MAXOWN + 69, 1: 2},
                                   max_count=3 * C.MAXOWN + 68, n_tiles=2, slab_P=gs().decl["slabs"]["slab_P"])
    st = graph_star
    cases["star65000"] = lambda: _case(lambda: st(65000), [[st(65000).a]], ["counts: both halves of one LDS word above 32,767"],
                                       n_own={0: 65001}, max_count=65000, n_tiles=2, P={(0, 0): 32766 + 2 * 65000, (1, 0): 65000 - 32766})
    cases["star65600"] = lambda: _case(lambda: st(65600), [[st(65600).a]], ["entries >= 65,536: the device-atomic path by itself"],
                                       hop2="global", n_own={0: 65601}, max_count=65600, n_tiles=3)
    go = graph_occ
    cases["occ"] = lambda: _case(go, [[h] for h in go().hubs], ["occurrences: 8, 9, 16 and 17 of 17 batches"],
                                 m_u={go().w[j]: j for j in OCC}, n_own={b: c + 1 for b, c in enumerate(go().cz)}, max_count=max(go().cz), n_tiles=1)
    gd = graph_degrees
    cases["degrees"] = lambda: _case(gd, [[gd().v, gd().iso], [gd().v2]], ["owner degrees 0, 1, 256, 257, 512, 513", "tiles: 1"],
                                     deg=dict(zip([gd().iso] + list(gd().owners), OWNER_DEGREES)), m_u={int(u): 2 for u in gd().owners[1:]},
                                     n_own={0: 7, 1: 5}, max_count=5, n_tiles=1)
    for ft in (8, 9):
        gt = functools.partial(graph_tiles, ft)
        cases[f"tiles{ft + 1}"] = (lambda gt=gt, ft=ft: _case(
            gt, [[gt().v], [gt().v2]], [f"tiles: {ft} whole and a last one of 5 nodes"], n_own={0: ft + 2, 1: (ft + 2) // 2 + 1},
            max_count=ft + 1, n_tiles=ft + 1, m_u={int(u): 2 for u in gt().owners[::2]}))
    return cases


CASE_NAMES = ("pairs", "pairs_single", "own1", "own2", "own63", "own64", "own65", "own6144", "own6145", "slabs", "star65000", "star65600",
              "occ", "degrees", "tiles9", "tiles10")
RANGE_CASES = ("degrees", "tiles9", "tiles10", "pairs")       # also run with the id ranges on (257 neighbours: big, 256: not)
TILE_MAJOR_CASES = ("pairs", "tiles9", "tiles10")            # 3 tiles: residue classes without a tile; 9, 10: classes with two
GLOBAL_CASES = ("pairs_single", "own1", "own65", "occ", "degrees", "tiles9")
REBUILDS = (("pairs", "pairs_single"), ("slabs", "own2"))


@functools.lru_cache(maxsize=None)
def case(name):
    c = _build_cases()[name]()
    g = c["graph"]()
    c["g"] = g
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """(pair counts, float64 x2) per batch of a case: computed once, shared by every test that needs them, never written to."""
    c = case(name)
    g = c["g"]
    pcs = pair_counts(g.rowptr, g.col, c["batches"])
    return pcs, [x2_from_counts(g.feat, bc) for bc in pcs]


def branches():
    """Every branch label of the table -> the case that reaches it."""
    out = {}
    for name in CASE_NAMES:
        for label in _build_cases()[name]()["reaches"]:
            out.setdefault(label, name)
    return out


def reached(name):
    """What a case's graph really gives: entries and P per (tile, batch), P per (slab, tile) of single-row batches, the largest c',
    owner occurrences per node over the chunk, degrees."""
    C = constants()
    c = case(name)
    g = c["g"]
    nt = n_tiles_of(g.n)
    pcs, _ = reference(name)
    P, n_own, slab_P, occ = {}, {}, {}, {}
    mx = 0
    for b, (bc, nodes) in enumerate(zip(pcs, c["batches"])):
        rows = closed_rows(g.rowptr, g.col, nodes)
        n_own[b] = int(sum(len(r) for r in rows))
        owner = np.repeat(np.arange(len(bc.U)), np.diff(bc.ptr))
        per = np.bincount(bc.ids >> C.SHIFT, minlength=nt)
        for t in range(nt):
            P[(t, b)] = int(per[t])
        if len(rows) == 1:                                         # no duplicates: entry order = id order, slabs are fixed
            sp = np.bincount(owner // C.MAXOWN * nt + (bc.ids >> C.SHIFT), minlength=nt * ((len(bc.U) - 1) // C.MAXOWN + 1))
            for s in range((len(bc.U) - 1) // C.MAXOWN + 1):
                for t in range(nt):
                    slab_P[(b, s, t)] = int(sp[s * nt + t])
        mx = max(mx, int(bc.cp.max(initial=0)))
        for u in bc.U:
            occ[int(u)] = occ.get(int(u), 0) + 1
    deg = np.diff(g.rowptr.astype(np.int64))
    return SimpleNamespace(P=P, n_own=n_own, slab_P=slab_P, max_count=mx, m_u=occ, deg=deg, n_tiles=nt)
