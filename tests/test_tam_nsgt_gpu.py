"""TAM's truncation round on the MI355X (`ggad_amd.tam_utils.DeviceNsgt`, csrc/tam_nsgt.hip, `tam.py --device_cut`): the device path
gives exactly the graphs of the host path -- same pattern, same bits in every normalised value, numpy's stream at the same position
-- on the vectors captured from the imported reference (`tests/golden/fullgraph_tam.npz`) and on a graph built here that walks the
branches of the kernels.  Every comparison is exact: the device path only selects entries and forms one rounded fp32 product."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import ggad_oracle as O

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N_BRANCH = 1100          # more rows than 1,024; the 2,048-row tile of the row-count scan: `test_scan_over_more_than_one_tile`
ROUNDS = 3


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(HERE, "golden", "fullgraph_tam.npz"))


def _raw(g):
    n = int(g["n"])
    a = sp.csr_matrix((np.ones(len(g["col"]), np.float32), g["col"], g["rowptr"]), shape=(n, n))
    r = (a + sp.eye(n)).tocsr()
    r.sort_indices()
    return r


def _sorted_pairs(m):
    coo = sp.csr_matrix(m).tocoo()
    got = np.stack([coo.row, coo.col], 1).astype(np.int32)
    return got[np.lexsort((got[:, 1], got[:, 0]))]


def _dev_csr(step):
    rowptr, col, val = (t.cpu().numpy() for t in step)
    return rowptr, col, val


def _assert_same_graph(step, host_norm, what):
    """Device (rowptr, col, val) == the host's normalised CSR, exactly."""
    rowptr, col, val = _dev_csr(step)
    assert rowptr.dtype == np.int32 and col.dtype == np.int32 and val.dtype == np.float32
    np.testing.assert_array_equal(rowptr, host_norm.indptr, err_msg=what)
    np.testing.assert_array_equal(col, host_norm.indices, err_msg=what)
    np.testing.assert_array_equal(val, host_norm.data, err_msg=what)


# ------------------------------------------------------------------------------------------------ the branch graph
SPECIAL = {1: 700, 2: 512, 3: 513, 4: 63, 5: 64, 6: 65}          # node -> stored entries of its row of A + I (self loop included)
HUB, TWIN_A, TWIN_B, FIRST_FILLER, FIRST_LONER = 0, 7, 8, 7, 1090


def branch_graph(seed=5):
    """(raw, dis): a symmetric A + I over 1,100 nodes and the attribute distance of each entry.  Node 0 is adjacent to nodes 1 .. 1049
    (1,050 entries: more than 1,024), node 1 has 700 entries (more than 512), nodes 2 .. 6 have exactly 512, 513, 63, 64 and 65, the
    ten nodes 1090 .. 1099 have only their self loop, nodes 7 and 8 are adjacent and have the same features (an off-diagonal
    distance of exactly 0); the special nodes get their entries from the fillers 7 .. 1089, which also hold 1,500 random pairs."""
    rng = np.random.default_rng(seed)
    n = N_BRANCH
    rows, cols = [], []

    def edge(a, b):
        rows.extend((a, b))
        cols.extend((b, a))

    for j in range(1, 1050):
        edge(HUB, j)
    fillers = np.arange(FIRST_FILLER, FIRST_LONER)
    for node, entries in SPECIAL.items():
        for j in rng.choice(fillers, size=entries - 2, replace=False):          # - self loop - the hub
            edge(node, int(j))
    edge(TWIN_A, TWIN_B)
    pairs = rng.choice(fillers, size=(1500, 2))
    for a, b in pairs[pairs[:, 0] != pairs[:, 1]]:
        edge(int(a), int(b))
    a = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n, n))
    a.data[:] = 1.0                                                              # (a pair drawn twice)
    raw = (a + sp.eye(n, dtype=np.float32)).tocsr()
    raw.sum_duplicates()
    raw.sort_indices()
    raw.data[:] = 1.0
    feat = rng.standard_normal((n, 8)).astype(np.float32)
    feat[TWIN_B] = feat[TWIN_A]
    dis = O.tam_calc_distance(raw.indptr, raw.indices, feat)                     # `calc_distance`'s formula
    return raw, dis


class _Recorder:
    """numpy's global stream, remembering what was drawn."""

    def __init__(self):
        self.drawn = []

    def random_sample(self, k):
        u = np.random.random_sample(k)
        self.drawn.append(u)
        return u


class _Replay:
    def __init__(self, drawn):
        self.drawn = list(drawn)

    def random_sample(self, k):
        u = self.drawn.pop(0)
        assert len(u) == k
        return u


@pytest.fixture(scope="module")
def branch():
    """The branch graph and its three host rounds from np.random.seed(11) (computed once, never changed): patterns, normalised CSRs, the
    numpy tail, and -- from the HOST result alone -- the facts that make the graph worth running."""
    from ggad_amd import tam_utils as T
    raw, dis = branch_graph()
    deg = np.diff(raw.indptr)
    assert deg[HUB] == 1050 and [int(deg[k]) for k in SPECIAL] == list(SPECIAL.values())
    assert np.all(deg[FIRST_LONER:] == 1) and raw.shape == (N_BRANCH, N_BRANCH) and abs(raw - raw.T).nnz == 0
    twin = raw.indptr[TWIN_A] + int(np.searchsorted(raw.indices[raw.indptr[TWIN_A]:raw.indptr[TWIN_A + 1]], TWIN_B))
    assert raw.indices[twin] == TWIN_B and dis[twin] == 0.0
    np.random.seed(11)
    cur, pats, norms, facts = raw, [], [], []
    for _ in range(ROUNDS):
        rec = _Recorder()
        new = T.graph_nsgt(raw, dis, cur, rec)
        # what this round did, restated from the host quantities: rows that do not qualify, entries cut in one direction only
        c = sp.csr_matrix(cur)
        c.sort_indices()
        key_raw = np.repeat(np.arange(N_BRANCH, dtype=np.int64), np.diff(raw.indptr)) * N_BRANCH + raw.indices
        key_cur = np.repeat(np.arange(N_BRANCH, dtype=np.int64), np.diff(c.indptr)) * N_BRANCH + c.indices
        d = dis[np.searchsorted(key_raw, key_cur)]
        cnt = np.diff(c.indptr)
        mean = T._nsgt_mean(d[d != 0])
        mx = np.zeros(N_BRANCH, np.float32)
        mx[cnt > 0] = np.maximum.reduceat(d, c.indptr[:-1][cnt > 0])
        thr = T.nsgt_thresholds(mx, cnt, mean, _Replay(rec.drawn))
        keep = sp.csr_matrix(((~(d > np.repeat(thr, cnt))).astype(np.float32), c.indices.copy(), c.indptr.copy()), shape=c.shape)
        keep.eliminate_zeros()
        facts.append(dict(before=int(c.nnz), after=int(new.nnz), not_qualifying=int(((cnt > 0) & ~(mx > mean)).sum()),
                          one_direction=int(abs(keep - keep.T).nnz), min_degree=int(np.diff(new.indptr).min())))
        pats.append(new)
        norms.append(T.normalize_adj_tensor(new))
        cur = new
    tail = np.random.random_sample(3)
    return dict(raw=raw, dis=dis, pats=pats, norms=norms, tail=tail, facts=facts)


# ------------------------------------------------------------------------------------------------ tests
def test_reference_fixture_two_rounds(g):
    """The two truncated graphs the imported reference produced, their normalised values and the position of numpy's stream."""
    from ggad_amd import tam_utils as T
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    tree = T.DeviceNsgt(_raw(g), g["dis_array_nz"], dev)
    np.random.seed(int(g["seed"]))
    for c in range(2):
        rowptr, col, val = _dev_csr(tree.step())
        rows = np.repeat(np.arange(int(g["n"]), dtype=np.int32), np.diff(rowptr))
        assert np.array_equal(np.stack([rows, col], 1), g[f"cut{c}.adj_nz"])
        np.testing.assert_array_equal(val, g[f"cut{c}.adj_norm_vals"])
        assert np.array_equal(_sorted_pairs(tree.pattern()), g[f"cut{c}.adj_nz"])
    np.testing.assert_array_equal(np.random.random_sample(3), g["nprandom_tail"])


def test_branches_three_rounds_equal_host_and_oracle(branch):
    """Rows of 1 / 63 / 64 / 65 / 512 / 513 / 700 / 1,050 entries, 1,100 rows for the scan, a zero off-diagonal distance: three rounds
    equal `graph_nsgt` + `normalize_adj_tensor` (pattern, rowptr, value bits, numpy tail) and the dense oracle's pattern."""
    from ggad_amd import tam_utils as T
    for k, f in enumerate(branch["facts"]):                  # from the host result alone, before the device is looked at
        print("round", k, f)
        assert f["after"] < f["before"], f
        assert f["not_qualifying"] >= 1, f
        assert f["one_direction"] >= 1, f
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    raw, dis = branch["raw"], branch["dis"]
    tree = T.DeviceNsgt(raw, dis, dev)
    np.random.seed(11)
    dev_pats = []
    for k in range(ROUNDS):
        step = tree.step()
        _assert_same_graph(step, branch["norms"][k], f"round {k}")
        pat = tree.pattern()
        assert np.array_equal(_sorted_pairs(pat), _sorted_pairs(branch["pats"][k]))
        dev_pats.append(pat)
    np.testing.assert_array_equal(np.random.random_sample(3), branch["tail"])
    # the dense restatement of the reference's loop, from the same seed
    dense_dis = torch.zeros(N_BRANCH, N_BRANCH)
    coo = raw.tocoo()
    dense_dis[torch.from_numpy(coo.row.astype(np.int64)), torch.from_numpy(coo.col.astype(np.int64))] = torch.from_numpy(dis)
    cur = torch.from_numpy(raw.toarray().astype(np.float32))
    np.random.seed(11)
    for k in range(ROUNDS):
        cur = O.tam_graph_nsgt(dense_dis, cur, np.random)
        assert np.array_equal(np.argwhere(cur.numpy() > 0).astype(np.int32), _sorted_pairs(dev_pats[k])), k
    np.testing.assert_array_equal(np.random.random_sample(3), branch["tail"])


def test_asymmetric_raw_is_refused():
    from ggad_amd import tam_utils as T
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    raw = sp.csr_matrix(np.array([[1, 1, 0], [1, 1, 1], [0, 0, 1]], dtype=np.float32))        # (1, 2) without (2, 1)
    with pytest.raises(ValueError, match="symmetric"):
        T.DeviceNsgt(raw, np.ones(raw.nnz, np.float32), dev)


def test_with_adjacency_equals_host_built_adjacency(branch, g):
    """`FullGraphAdj.with_adjacency(base, *step)` against `FullGraphAdj(normalize_adj_tensor(cut), raw, dev)`: bit-equal SpMM on the
    branch graph, bit-equal forward loss and `inference` on the fixture graph; the raw side is base's own."""
    from ggad_amd import tam_utils as T
    from ggad_amd.fullgraph import FullGraphAdj, spmm
    from ggad_amd.model_tam import Model
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    raw, dis = branch["raw"], branch["dis"]
    base = FullGraphAdj(T.normalize_adj_tensor(raw), raw, dev)
    tree = T.DeviceNsgt(raw, dis, dev)
    np.random.seed(11)
    shared = FullGraphAdj.with_adjacency(base, *tree.step())
    host = FullGraphAdj(branch["norms"][0], raw, dev)
    assert shared.Rt is base.Rt and shared.raw_host is base.raw_host and shared.At is shared.A and shared.symmetric
    assert shared.r_inv_dev() is base.r_inv_dev()
    X = torch.randn(N_BRANCH, 128, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    assert torch.equal(spmm(shared.A, X), spmm(host.A, X))
    # the fixture graph with the captured initial weights of its first round
    raw_g = _raw(g)
    base_g = FullGraphAdj(T.normalize_adj_tensor(raw_g), raw_g, dev)
    head = T.tam_head(base_g, g["normal_idx"])
    tree_g = T.DeviceNsgt(raw_g, g["dis_array_nz"], dev)
    np.random.seed(int(g["seed"]))
    shared_g = FullGraphAdj.with_adjacency(base_g, *tree_g.step())
    np.random.seed(int(g["seed"]))
    host_g = FullGraphAdj(T.normalize_adj_tensor(T.graph_nsgt(raw_g, g["dis_array_nz"], raw_g)), raw_g, dev)
    assert T.tam_head(shared_g, g["normal_idx"]) is head                    # the cached head of base
    model = Model(int(g["f"]), int(g["n_h"]), "prelu", 2, "avg").to(dev)
    model.load_state_dict({k[len("init0."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("init0.")})
    feats = torch.from_numpy(g["features"])[None].to(dev)
    out = []
    for adj in (shared_g, host_g):
        with torch.no_grad():
            emb = model.forward(feats, adj)[0]
            loss, m = T.max_message(emb[0], adj, g["normal_idx"])
            out.append((loss.clone(), m.clone(), T.inference(emb[0], adj).clone(), emb.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_forks_stepped_alternately(g):
    """Two trees of one run (`--N_tree 2`) share the static part and nothing else: stepped A, B, A, B they reproduce two host trees
    stepped in the same order from the same seed."""
    from ggad_amd import tam_utils as T
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    raw, dis = _raw(g), g["dis_array_nz"]
    np.random.seed(21)
    cur, host = [raw, raw], []
    for k in range(4):
        cur[k % 2] = T.graph_nsgt(raw, dis, cur[k % 2])
        host.append(T.normalize_adj_tensor(cur[k % 2]))
    tail = np.random.random_sample(3)
    trees = [T.DeviceNsgt(raw, dis, dev)]
    trees.append(trees[0].fork())
    assert trees[1]._s is trees[0]._s and trees[1].alive is not trees[0].alive
    np.random.seed(21)
    for k in range(4):
        _assert_same_graph(trees[k % 2].step(), host[k], f"step {k}")
    np.testing.assert_array_equal(np.random.random_sample(3), tail)
    assert not np.array_equal(host[2].indices, host[3].indices)              # (the two trees did diverge)


def test_scan_over_more_than_one_tile():
    """A chain of 5,000 nodes: the row counts cross the 2,048-element tile of the scan, so the per-tile offsets are used."""
    from ggad_amd import tam_utils as T
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n = 5000
    i = np.arange(n - 1)
    a = sp.csr_matrix((np.ones(2 * (n - 1), np.float32), (np.concatenate((i, i + 1)), np.concatenate((i + 1, i)))), shape=(n, n))
    raw = (a + sp.eye(n, dtype=np.float32)).tocsr()
    raw.sort_indices()
    dis = O.tam_calc_distance(raw.indptr, raw.indices, np.random.default_rng(2).standard_normal((n, 8)).astype(np.float32))
    np.random.seed(4)
    cut = T.graph_nsgt(raw, dis, raw)
    tail = np.random.random_sample(3)
    assert cut.nnz < raw.nnz
    np.random.seed(4)
    _assert_same_graph(T.DeviceNsgt(raw, dis, dev).step(), T.normalize_adj_tensor(cut), "chain")
    np.testing.assert_array_equal(np.random.random_sample(3), tail)


@pytest.mark.parametrize("fused", [False, True])
def test_tam_loop_with_device_cut_equals_default(g, fused, capsys):
    """`tam.py`'s round loop, 2 rounds x 2 trees x 5 epochs on a synthetic graph of the fixture's size: with `--device_cut` every loss
    and every message has the bits of the run without it, and numpy's stream ends at the same position."""
    import tam
    from ggad_amd import synth
    from ggad_amd import tam_utils as T
    from ggad_amd.fullgraph import FlatAdam
    from ggad_amd.model_tam import Model
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, f = int(g["n"]), int(g["f"])
    rowptr, col = synth.make_graph(n, 6 * n, 3, kind="powerlaw", max_degree=max(16, n // 8))
    adj = synth.csr_to_scipy(rowptr, col, n)
    adj = ((adj + adj.T) > 0).astype(np.float32)
    raw = (adj + sp.eye(n)).tocsr()
    raw.sort_indices()
    feats = torch.from_numpy(synth.make_features(n, f, 3).astype(np.float32))[None].to(dev)
    ano = synth.make_labels(n, 0.08, 3)
    normal = np.flatnonzero(ano == 0)[::3]
    y = torch.as_tensor(ano.astype(np.int64), device=dev)
    idx_test = torch.arange(0, n, 2, device=dev)
    dis = T.calc_distance(raw, feats[0])
    runs = []
    for flag in ([], ["--device_cut"]):
        args = tam.parse(["--synthetic", "--quiet", "--cutting", "2", "--N_tree", "2", "--num_epoch", "5", "--lr", "1e-3"]
                         + (["--fused_head"] if fused else []) + flag)
        assert args.device_cut == bool(flag)
        torch.manual_seed(5)
        models = [Model(f, args.embedding_dim, "prelu", args.negsamp_ratio, args.readout).to(dev) for _ in range(4)]
        opts = [FlatAdam(m.parameters(), lr=args.lr, weight_decay=0.0) for m in models]
        np.random.seed(9)
        losses, msgs, _ = tam.train_rounds(args, dev, raw, dis, feats, models, opts, normal, y, idx_test)
        runs.append((losses, msgs, np.random.random_sample(3)))
    capsys.readouterr()
    assert len(runs[0][0]) == 4
    for a, b in zip(runs[0][0] + runs[0][1], runs[1][0] + runs[1][1]):
        assert torch.equal(a, b)
    np.testing.assert_array_equal(runs[0][2], runs[1][2])
