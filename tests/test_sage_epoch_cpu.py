"""The native epoch scheduler of the GraphSAGE epoch path (csrc/sampler.cpp: `ggad_sage_sched_epoch`, `PyCompatRandom.sage_epoch`): the
`random` stream of the reference fixture (tests/golden/minibatch_sage.npz), equality with the per-call path (`shuffle` and
`sample_rows` per batch) on the branch graph of tests/test_sage_device_gpu.py, and the refusals before the first draw.  No GPU."""
import numpy as np
import pytest

from conftest import load_golden
from ggad_amd import _lib
from ggad_amd.sampler import PyCompatRandom, sample_setsize
from test_sage_device_gpu import D0, D1, D9, D10, D11, D85, D86, HUB, _branch_graph

K = 10


def _split(table, b_max, k):
    """(nodes, cnt, labels, nbr) views of an epoch table (num_batches, b_max * (3 + k))."""
    nb = table.shape[0]
    return (table[:, :b_max], table[:, b_max:2 * b_max], table[:, 2 * b_max:3 * b_max],
            table[:, 3 * b_max:].reshape(nb, b_max, k))


def _per_call_epoch(rng, rowptr, col, train, pool, bs, n_pseudo, nb, k):
    """What `_train_sage_device` draws per epoch on the step path: [(nodes, nbr, cnt)] per batch."""
    rng.shuffle(train)
    out = []
    for b in range(nb):
        i0, i1 = b * bs, min((b + 1) * bs, len(train))
        rng.shuffle(pool)
        nodes = np.concatenate([train[i0:i1], pool[:n_pseudo]])
        out.append((nodes,) + tuple(rng.sample_rows(rowptr, col, nodes, k)))
    return out


def test_fixture_stream_in_two_scheduler_calls():
    """Two calls (one per epoch) reproduce the 8 batches of the fixture row for row, their tables equal the per-call sampler's,
    and after the three test chunks of 30 the generator stands where the fixture's `random` stood, word for word."""
    g = load_golden("minibatch_sage.npz")
    rowptr, col, labels = g["rowptr"], g["col"], g["labels"].astype(np.int64)
    train = np.arange(100, 700, dtype=np.int64)
    pool = np.nonzero(labels)[0][:60].astype(np.int64)
    rng, twin = PyCompatRandom(72), PyCompatRandom(72)
    t_train, t_pool = train.copy(), pool.copy()
    bs, nb, n_pseudo = 40, 4, 10
    step = 0
    for epoch in range(2):
        table, lens = rng.sage_epoch(rowptr, col, labels, train, pool, bs, n_pseudo, nb, K, checked=epoch > 0)
        nodes, cnt, lab, nbr = _split(table, bs + n_pseudo, K)
        assert lens.tolist() == [bs + n_pseudo] * nb
        want = _per_call_epoch(twin, rowptr, col, t_train, t_pool, bs, n_pseudo, nb, K)
        for b in range(nb):
            assert np.array_equal(nodes[b], g["batches"][step]), step
            assert np.array_equal(lab[b], labels[g["batches"][step]])
            assert np.array_equal(nbr[b], want[b][1]) and np.array_equal(cnt[b], want[b][2]), step
            step += 1
    assert step == 8
    for s in range(0, 90, 30):
        rng.sample_rows(rowptr, col, g["test_nodes"][s:s + 30], K)
    assert np.array_equal(np.array(rng.to_python_state()[1], dtype=np.uint64), g["py_random_after"])


def _branch_lists(short_pool):
    """Train list of 103 ids on the branch graph: every special degree, the hub twice; batches of 25 over 6 steps give one
    short batch (3 train rows) and one without train rows.  The pool shares an id with the train list."""
    gen = np.random.default_rng(9)
    special = [D0, D1, D9, D10, D11, D85, D86, HUB, HUB]
    train = np.array(special + [int(v) for v in gen.choice(np.arange(1, 500), size=94, replace=False)], dtype=np.int64)
    pool = np.array([int(v) for v in gen.choice(np.arange(1, 500), size=4 if short_pool else 11, replace=False)] + [D86],
                    dtype=np.int64)
    assert len(train) == 103
    return train, pool


@pytest.mark.parametrize("short_pool", [False, True], ids=["pool 12 >= 8", "pool 5 < 8"])
def test_scheduler_equals_the_per_call_path_bit_for_bit(short_pool):
    """Three consecutive epochs on the branch graph (rows of degree 0, 1, 9, 10, 11, 85, 86 and the hub of 1,535 entries): tables,
    row counts, labels, -1 padding, both shuffled arrays and the generator state equal the per-call path's after every epoch.
    n_train = 103 with batch_size 25 and 6 batches: batch 4 is short (3 + pool rows), batch 5 holds pool rows alone."""
    rowptr, col = _branch_graph()
    n = len(rowptr) - 1
    labels = (np.random.default_rng(3).random(n) < 0.3).astype(np.int64)
    train, pool = _branch_lists(short_pool)
    t_train, t_pool = train.copy(), pool.copy()
    bs, nb, n_pseudo = 25, 6, 8
    n_p = min(n_pseudo, len(pool))
    b_max = bs + n_pseudo
    rng, twin = PyCompatRandom(5), PyCompatRandom(5)
    buf = np.empty(nb * b_max * (3 + K), dtype=np.int32)
    for epoch in range(3):
        buf[:] = 77                                                         # every word of the table is written
        table, lens = rng.sage_epoch(rowptr, col, labels, train, pool, bs, n_pseudo, nb, K, out=buf, checked=epoch > 0)
        assert np.shares_memory(table, buf)
        nodes, cnt, lab, nbr = _split(table, b_max, K)
        want = _per_call_epoch(twin, rowptr, col, t_train, t_pool, bs, n_pseudo, nb, K)
        assert lens.tolist() == [25 + n_p] * 4 + [3 + n_p, n_p]
        for b in range(nb):
            w_nodes, w_nbr, w_cnt = want[b]
            m = len(w_nodes)
            assert lens[b] == m
            assert np.array_equal(nodes[b, :m], w_nodes) and np.array_equal(cnt[b, :m], w_cnt), (epoch, b)
            assert np.array_equal(nbr[b, :m], w_nbr) and np.array_equal(lab[b, :m], labels[w_nodes]), (epoch, b)
            assert (nodes[b, m:] == 0).all() and (cnt[b, m:] == 0).all() and (lab[b, m:] == 0).all() and (nbr[b, m:] == -1).all()
        assert np.array_equal(train, t_train) and np.array_equal(pool, t_pool)
        assert rng.to_python_state() == twin.to_python_state()
    assert (cnt == 0).any() and (cnt == 1).any() and (cnt == 9).any() and (cnt == K).any()


def _raw(rng, rowptr, col, labels, train, pool, bs, n_pseudo, nb, k, checked=0):
    """The return code of the entry point itself."""
    b_max = bs + n_pseudo
    stride = b_max * (3 + max(k, 1))
    table = np.full(max(nb, 1) * stride, 77, dtype=np.int32)
    lens = np.full(max(nb, 1), 77, dtype=np.int32)
    rc = _lib.load().ggad_sage_sched_epoch(rng._h, train.ctypes.data, len(train), pool.ctypes.data, len(pool), bs, n_pseudo, nb,
                                           rowptr.ctypes.data, col.ctypes.data, len(rowptr) - 1, labels.ctypes.data, k,
                                           sample_setsize(max(k, 1)), checked, table.ctypes.data, stride, lens.ctypes.data)
    return rc, table, lens


def test_refusals_come_before_the_first_draw():
    """GGAD_E_INVALID (-1) with the generator, both arrays and the output untouched: an id outside [0, n_nodes) in train or in pool,
    k < 1, an unsorted CSR row of a listed id, a batch of zero rows (no pool rows and the train list used up)."""
    rowptr, col = _branch_graph()
    n = len(rowptr) - 1
    labels = np.zeros(n, dtype=np.int64)
    train, pool = _branch_lists(False)
    bad_col = col.copy()
    a = int(rowptr[D11])
    bad_col[a], bad_col[a + 1] = bad_col[a + 1], bad_col[a]
    empty = np.zeros(0, dtype=np.int64)

    def with_id(a, pos, v):
        a = a.copy()
        a[pos] = v
        return a
    cases = {"train id = n": (with_id(train, 50, n), pool, col, 25, 8, 6, K),
             "train id < 0": (with_id(train, 0, -1), pool, col, 25, 8, 6, K),
             "pool id = n": (train, with_id(pool, 11, n), col, 25, 8, 6, K),
             "pool id < 0": (train, with_id(pool, 3, -5), col, 25, 8, 6, K),
             "k = 0": (train, pool, col, 25, 8, 6, 0),
             "k < 0": (train, pool, col, 25, 8, 6, -3),
             "unsorted row": (train, pool, bad_col, 25, 8, 6, K),
             "empty batch, n_pseudo = 0": (train, pool, col, 25, 0, 6, K),
             "empty batch, empty pool": (train, empty, col, 25, 8, 6, K)}
    rng = PyCompatRandom(13)
    before = rng.to_python_state()
    for name, (tr, po, cc, bs, n_pseudo, nb, k) in cases.items():
        tr0, po0 = tr.copy(), po.copy()
        rc, table, lens = _raw(rng, rowptr, cc, labels, tr, po, bs, n_pseudo, nb, k)
        assert rc == -1, name
        assert rng.to_python_state() == before, name
        assert np.array_equal(tr, tr0) and np.array_equal(po, po0), name
        assert (table == 77).all() and (lens == 77).all(), name
    with pytest.raises(ValueError):
        rng.sage_epoch(rowptr, bad_col, labels, train, pool, 25, 8, 6, K)
    assert rng.to_python_state() == before
    # the same arguments, valid: five batches with n_pseudo = 0 (the sixth would be empty), and the full schedule
    rc, _, lens = _raw(rng, rowptr, col, labels, train.copy(), pool.copy(), 25, 0, 5, K)
    assert rc == 0 and lens[:5].tolist() == [25, 25, 25, 25, 3]
    rc, _, lens = _raw(rng, rowptr, col, labels, train.copy(), pool.copy(), 25, 8, 6, K)
    assert rc == 0 and lens.tolist() == [33, 33, 33, 33, 11, 8]
