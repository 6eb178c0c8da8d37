"""The host side of TAM's device truncation path (`tam.py --device_cut`), no GPU involved: the threshold helper that `graph_nsgt` and
`DeviceNsgt.step` share, fed what the device hands it (per-row maximum and count, the mean), against the vectors captured from the
imported reference (`tests/golden/fullgraph_tam.npz`); and the switch of `tam.py`."""
import os

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))


def _raw(g):
    n = int(g["n"])
    a = sp.csr_matrix((np.ones(len(g["col"]), np.float32), g["col"], g["rowptr"]), shape=(n, n))
    r = (a + sp.eye(n)).tocsr()
    r.sort_indices()
    return r


def test_threshold_helper_reproduces_the_reference_cuts():
    """Mask over raw's entries + numpy row statistics + `nsgt_thresholds` + keep / symmetrise, i.e. the device path's arithmetic done
    with numpy: both captured cuts and the position of numpy's stream afterwards."""
    from ggad_amd import tam_utils as T
    g = np.load(os.path.join(HERE, "golden", "fullgraph_tam.npz"))
    raw = _raw(g)
    n = raw.shape[0]
    dis = g["dis_array_nz"].astype(np.float32)
    rows = np.repeat(np.arange(n), np.diff(raw.indptr))
    key = rows.astype(np.int64) * n + raw.indices
    tpos = np.searchsorted(key, raw.indices.astype(np.int64) * n + rows)
    assert np.array_equal(key[tpos], raw.indices.astype(np.int64) * n + rows)          # raw is symmetric
    alive = np.ones(raw.nnz, dtype=bool)
    np.random.seed(int(g["seed"]))
    for c in range(2):
        cnt = np.bincount(rows[alive], minlength=n)
        mx = np.full(n, -np.inf, dtype=np.float32)
        np.maximum.at(mx, rows[alive], dis[alive])
        nz = dis[alive & (dis != 0)]
        mean = np.mean(nz, dtype=np.float32)
        thr = T.nsgt_thresholds(mx, cnt, mean, np.random)
        assert thr.dtype == np.float32 and thr.shape == (n,)
        keep = alive & ~(dis > thr[rows])
        alive = keep | keep[tpos]
        got = np.stack([rows[alive], raw.indices[alive]], 1).astype(np.int32)
        assert np.array_equal(got, g[f"cut{c}.adj_nz"])
    np.testing.assert_array_equal(np.random.random_sample(3), g["nprandom_tail"])


def test_threshold_helper_rows_that_take_no_draw():
    """Rows without entries and rows whose maximum does not exceed the mean get +inf and take nothing from the stream."""
    from ggad_amd import tam_utils as T

    class Stream:
        asked = []

        def random_sample(self, k):
            self.asked.append(k)
            return np.full(k, 0.5)

    s = Stream()
    thr = T.nsgt_thresholds(np.array([9.0, 1.0, 2.0, 3.0], np.float32), np.array([0, 4, 2, 1]), np.float32(2.0), s)
    assert s.asked == [1]
    np.testing.assert_array_equal(thr, np.array([np.inf, np.inf, np.inf, 2.5], np.float32))
    thr = T.nsgt_thresholds(np.array([9.0], np.float32), np.array([3]), np.float32("nan"), s)      # no non-zero distance at all
    assert s.asked == [1, 0] and np.isinf(thr[0])


def test_parser_knows_device_cut_and_defaults_it_off():
    import tam
    assert tam.parse([]).device_cut is False
    assert tam.parse(["--device_cut"]).device_cut is True
    assert tam.parse(["--fused_head"]).device_cut is False
