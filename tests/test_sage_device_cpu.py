"""The native neighbour sampler of the GraphSAGE device path (csrc/sampler.cpp: `ggad_pyset_order_i32`, `ggad_mt_sample_rows`)
against the RUNNING interpreter: the iteration order of a python set of ints, `random.sample` over it, and the whole `random`
stream of the reference fixture (tests/golden/minibatch_sage.npz).  No GPU: the library is loaded as tests/test_sampler.py does."""
import random

import numpy as np
import pytest

from conftest import load_golden
from ggad_amd.sampler import PyCompatRandom, pyset_order, sample_setsize

DEGREES = list(range(1, 130)) + [200, 341, 342, 343, 1365, 1366, 5000, 60000]      # resize points and the 50,000 switch among them
STRIDES = (1, 8, 1024, 32768)


def test_set_order_equals_the_interpreters():
    """`ggad_pyset_order_i32` == `list(set(int(c) for c in keys))` here and now: a CPython whose set table differs fails this test
    instead of drifting silently.  Keys start at 0, at an odd offset and so that the last one is 2^31 - 1."""
    cases = 0
    for deg in DEGREES:
        for stride in STRIDES:
            top = (deg - 1) * stride
            for base in (0, 7, 2 ** 31 - 1 - top):
                if base < 0 or base + top > 2 ** 31 - 1:
                    continue
                keys = np.arange(deg, dtype=np.int64) * stride + base
                want = list(set(int(c) for c in keys))
                got = pyset_order(keys.astype(np.int32)).tolist()
                assert got == want, (deg, stride, base)
                cases += 1
    assert cases > 1500
    assert pyset_order(np.zeros(0, dtype=np.int32)).tolist() == []
    for bad in ([3, 3], [5, 4], [-1, 2]):
        with pytest.raises(ValueError):
            pyset_order(np.array(bad, dtype=np.int32))


def _graph_with_degrees(degrees, rng):
    """CSR whose row r has degrees[r] distinct ascending columns, spread over [0, n)."""
    n = max(len(degrees), max(degrees) * 3 + 5)
    rowptr = np.zeros(n + 1, dtype=np.int32)
    cols = []
    for r in range(n):
        d = degrees[r] if r < len(degrees) else 0
        cols.append(np.sort(rng.choice(n, size=d, replace=False)).astype(np.int32))
        rowptr[r + 1] = rowptr[r] + d
    return rowptr, np.concatenate(cols) if cols else np.zeros(0, dtype=np.int32)


@pytest.mark.parametrize("k", [1, 5, 6, 10, 25])
def test_sample_rows_equals_random_sample_row_by_row(k):
    """Tables, lengths, -1 padding and the generator state after every call, against `sorted(random.sample(tuple(s), k))` on sets
    filled in ascending order; degrees around k, around both sides of `setsize` for k <= 5 (21), k = 6 .. 21 (85) and beyond, 0;
    a node listed twice is sampled twice; a row shorter than k consumes nothing."""
    degrees = sorted(set(d for d in (k - 1, k, k + 1, 21, 22, 85, 86, 300, 0, sample_setsize(k), sample_setsize(k) + 1) if d >= 0))
    rowptr, col = _graph_with_degrees(degrees, np.random.default_rng(k))
    adj = [set(int(c) for c in col[rowptr[v]:rowptr[v + 1]]) for v in range(len(rowptr) - 1)]
    nodes = list(range(len(degrees))) + [len(degrees) - 1, 0, len(degrees) - 1] + list(range(len(degrees)))[::-1]
    random.seed(1000 + k)
    rng = PyCompatRandom.from_python_state(random.getstate())
    nbr, cnt = rng.sample_rows(rowptr, col, nodes, k)
    assert nbr.shape == (len(nodes), k) and nbr.dtype == np.int32 and cnt.shape == (len(nodes),)
    for r, v in enumerate(nodes):
        s = adj[v]
        want = sorted(random.sample(tuple(s), k)) if len(s) >= k else sorted(s)
        assert cnt[r] == len(want), (r, v)
        assert nbr[r, :cnt[r]].tolist() == want, (r, v)
        assert (nbr[r, cnt[r]:] == -1).all()
    assert rng.to_python_state() == random.getstate()
    # rows shorter than k alone: nothing is drawn
    short = [v for v in range(len(degrees)) if degrees[v] < k]
    if short:
        before = rng.to_python_state()
        nbr, cnt = rng.sample_rows(rowptr, col, short * 3, k)
        assert rng.to_python_state() == before
        assert cnt.tolist() == [degrees[v] for v in short] * 3
    before = rng.to_python_state()
    with pytest.raises(ValueError):
        rng.sample_rows(rowptr, col, [0, len(rowptr) - 1], k)            # an id outside the graph
    bad_col = col.copy()
    a = int(rowptr[len(degrees) - 1])
    bad_col[a], bad_col[a + 1] = bad_col[a + 1], bad_col[a]
    with pytest.raises(ValueError):
        rng.sample_rows(rowptr, bad_col, [0, len(degrees) - 1], k)        # an unsorted row
    assert rng.to_python_state() == before                               # a refused call draws nothing


def test_fixture_stream_on_the_native_generator_alone():
    """The loop of `test_graphsage_training_loop_vs_reference_golden` (tests/test_dropin_gpu.py) with every shuffle and every
    neighbour sample drawn by the native generator: the 8 batches of the fixture, and its `random` state after three test chunks
    of 30; one call over the 90 test nodes gives the tables and the state of the three."""
    g = load_golden("minibatch_sage.npz")
    rowptr, col = g["rowptr"], g["col"]
    labels = g["labels"]
    idx_train = np.arange(100, 700, dtype=np.int64)
    idx_anomaly = np.nonzero(labels)[0][:60].astype(np.int64)
    rng = PyCompatRandom(72)
    bs, nb, n_pseudo, k = 40, 4, 10, 10
    step = 0
    for epoch in range(2):
        rng.shuffle(idx_train)
        for b in range(nb):
            rng.shuffle(idx_anomaly)
            batch = np.concatenate([idx_train[b * bs:(b + 1) * bs], idx_anomaly[:n_pseudo]])
            assert np.array_equal(batch, g["batches"][step]), step
            rng.sample_rows(rowptr, col, batch, k)
            step += 1
    assert step == 8
    test_nodes = g["test_nodes"]
    fork = PyCompatRandom.from_python_state(rng.to_python_state())
    chunks = [rng.sample_rows(rowptr, col, test_nodes[s:s + 30], k) for s in range(0, 90, 30)]
    assert np.array_equal(np.array(rng.to_python_state()[1], dtype=np.uint64), g["py_random_after"])
    nbr, cnt = fork.sample_rows(rowptr, col, test_nodes, k)
    assert np.array_equal(nbr, np.concatenate([c[0] for c in chunks])) and np.array_equal(cnt, np.concatenate([c[1] for c in chunks]))
    assert fork.to_python_state() == rng.to_python_state()
