"""Host-side sparse structures of the full-graph path: the device CSR (`Csr`) and the launch plans of its SpMM kernels.

A plan is a set of integer tables built once per matrix on the host and cached: segment tables (`plan`, `sliced_plan`,
`rowslice_plan`; the last two hang on the `plan` whose rows they cover, the sliced one per column-range count) for the CSR /
sliced / row-slice kernels, and the entry streams of the LDS-panel and LDS-ring products (`panel_plan`, `ring_plan`; kernels
k_spmm_panel / k_spmm_ring in csrc/fullgraph.hip, fill loops in csrc/spmm_panel_build.cpp / csrc/spmm_ring_build.cpp).  The two
stream plans share their round layout, the dealing of rounds to waves and the XCD workgroup table (`_round_layout`, `_deal_rounds`,
`_xcd_workgroup_table`); `fullgraph.spmm_route` chooses the kernel of a product and `fullgraph.spmm` launches it.
"""
from __future__ import annotations

import heapq
import os
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import _lib


def _dev_i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _dev_f32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


WIDE = 0x40000000                                                         # row_tab flag of a wide round (GGAD_SPMM_PANEL_WIDE in ggad_hip.h)

# What the panel and the ring plan share: the rows of the product in rounds of 8 (one per lane group), longest first.
Rounds = namedtuple("Rounds", "nnz n_rounds nb kr round_rows round_out round_wide")


def _plan_rows(m, diag, rows_sel):
    """(rowptr, colv, skip_diag, cnt, rows) of a panel / ring plan over host matrix `m`: `cnt` = stream entries per output row
    (without the diagonal when `diag` carries it), `rows` = None or the matrix row of every output row."""
    skip_diag = 1 if diag is not None else 0                              # the diagonal is applied in the epilogue
    rowptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
    colv = np.ascontiguousarray(m.indices, dtype=np.int32)
    cnt = np.diff(rowptr)
    if skip_diag:
        cnt = cnt - (m.diagonal() != 0)
    rows = None if rows_sel is None else np.asarray(rows_sel, dtype=np.int64)
    if rows is not None:                                                  # output row i = matrix row rows[i]
        cnt = cnt[rows]
    return rowptr, colv, skip_diag, cnt, rows


def _scale_vectors(fac, rows, dev):
    """rs / cs / diag of a plan on the device, straight from `value_factors()` (rs per output row)."""
    rs, cs, diag = fac
    if rs is not None and rows is not None:
        rs = rs[rows]
    return dict(rs=None if rs is None else _dev_f32(rs, dev), cs=None if cs is None else _dev_f32(cs, dev),
                diag=None if diag is None else _dev_f32(diag, dev))


def _round_layout(cnt, rows, n_slices, NW, KR):
    """Rounds of 8 output rows for `nb` row blocks of `NW` waves with at most `KR` rounds each, or None (no entries / more than `KR`
    rounds per wave at 64 x 256 workgroups).  round_rows (flat) = matrix rows, round_out = output rows (row_tab), -1 = none."""
    n_rows = len(cnt)
    nnz = int(cnt.sum())
    if nnz == 0:
        return None
    order = np.argsort(-cnt, kind="stable")                               # rows of similar length share a round
    # Hub rows get a round of their own, WIDE: the row's entries are dealt over all 8 lane groups and the kernel adds the 8
    # accumulators in its epilogue.  A round of 8 hub rows of 7,000 entries is 7,000 steps for ONE wave -- 1.4 times the share
    # of a wave on the T-Finance-size graph, so the slowest wave of a panel had 1.5 x the mean work however the rounds were
    # dealt; as 8 wide rounds of 900 steps the same work spreads over 8 waves.  Wide: rows longer than half a wave's share.
    nb0 = max(1, 256 // n_slices)
    while -(-((n_rows + 7) // 8) // (nb0 * NW)) > KR:
        nb0 += max(1, 256 // n_slices)
    share = nnz / 8.0 / (nb0 * NW)                                        # steps of a wave if all slots were full
    n_wide = int(np.searchsorted(-cnt[order], -max(256.0, share / 2.0), side="left"))
    # (bounded: a wide row takes a round slot of its own, and the workgroup count -- every workgroup stages the whole operand --
    # must not grow for it: with 76 instead of 51 row blocks the T-Finance product took 654 instead of 573 us)
    room = nb0 * NW * KR - (n_rows + 7) // 8
    n_wide = max(0, min(n_wide, int(room * 8 // 7 * 0.9)))
    n_rounds = n_wide + (n_rows - n_wide + 7) // 8
    nb = kr = None
    for mult in range(1, 65):                                             # workgroups ~ a multiple of the 256 CUs
        nb = max(1, (256 * mult) // n_slices)
        kr = -(-n_rounds // (nb * NW))
        if kr <= KR:
            break
    if kr is None or kr > KR:
        return None
    src_rows = (order if rows is None else rows[order]).astype(np.int32)  # matrix row of every output row, longest first
    round_rows = np.full((n_rounds, 8), -1, dtype=np.int32)               # matrix rows of a round (lane group = position)
    round_out = np.full((n_rounds, 8), -1, dtype=np.int32)                # output rows of a round (row_tab)
    round_rows[:n_wide, :] = src_rows[:n_wide, None]                      # (a wide round: its row in all 8 slots, flagged)
    round_out[:n_wide, :] = (order[:n_wide, None] | WIDE).astype(np.int32)
    rest = n_rows - n_wide
    round_rows[n_wide:].reshape(-1)[:rest] = src_rows[n_wide:]
    round_out[n_wide:].reshape(-1)[:rest] = order[n_wide:].astype(np.int32)
    round_wide = np.zeros(n_rounds, dtype=np.int32)
    round_wide[:n_wide] = 1
    return Rounds(nnz, n_rounds, nb, kr, np.ascontiguousarray(round_rows.reshape(-1)), round_out, round_wide)


def _deal_rounds(work, nb, NW, KR):
    """(blk_of_round, wave_of_round, k_of_round): row block, wave and accumulator slot of every round, by its `work`.
    A workgroup waits at its barriers for its slowest wave, and the rounds of the hub rows are many times longer than the others:
    rounds are dealt to the workgroups in a snake over the work order and inside a workgroup to the least loaded wave that has a
    free slot (longest first) -- dealt in rank order, the slowest wave of a panel had 2.2 x the mean work on the T-Finance-size graph
    (1.5 x with 8-row rounds only: the longest round alone was 1.4 mean wave loads -- hence the wide rounds of `_round_layout`)."""
    n_rounds = len(work)
    by_work = np.argsort(-work, kind="stable")
    pos_w = np.arange(n_rounds, dtype=np.int64)
    lap, idx = pos_w // nb, pos_w % nb
    blk_of_round = np.empty(n_rounds, dtype=np.int64)
    blk_of_round[by_work] = np.where(lap % 2 == 0, idx, nb - 1 - idx)
    wave_of_round = np.empty(n_rounds, dtype=np.int64)
    k_of_round = np.empty(n_rounds, dtype=np.int64)
    members = [[] for _ in range(nb)]
    for r_ in by_work.tolist():                                           # every workgroup's rounds, longest first
        members[blk_of_round[r_]].append(r_)
    work_l = work.tolist()
    for b in range(nb):
        heap = [(0, w) for w in range(NW)]
        used = [0] * NW
        for r_ in members[b]:
            load, w = heapq.heappop(heap)
            wave_of_round[r_], k_of_round[r_] = w, used[w]
            used[w] += 1
            if used[w] < KR:
                heapq.heappush(heap, (load + work_l[r_], w))
    return blk_of_round, wave_of_round, k_of_round


def _xcd_workgroup_table(n_slices, nb, block=False):
    """(wg, n_wg): wg[i] = (slice, row block) of workgroup i or (-1, -1); workgroup i runs on XCD i % 8.  Default: the workgroups of
    a slice share an XCD and its L2 (the loads of the operand hit); the slices of an incomplete round of 8 are dealt over all XCDs.
    `block` (the ring's GGAD_RING_XCD=block): the workgroups of a row block do (their common quad stream hits)."""
    lists = [[] for _ in range(8)]
    if block:
        allw = [(sl, b) for b in range(nb) for sl in range(n_slices)]
        q, rem = divmod(len(allw), 8)
        at = 0
        for x in range(8):
            take = q + (1 if x < rem else 0)
            lists[x] = allw[at:at + take]
            at += take
    else:
        full = (n_slices // 8) * 8
        for sl in range(full):
            lists[sl % 8].extend((sl, b) for b in range(nb))
        for i, it in enumerate([(sl, b) for b in range(nb) for sl in range(full, n_slices)]):
            lists[i % 8].append(it)
    L = max(len(x) for x in lists)
    wg = np.full((L * 8, 2), -1, dtype=np.int32)
    for x in range(8):
        if lists[x]:
            wg[x + 8 * np.arange(len(lists[x]))] = np.asarray(lists[x], dtype=np.int32)
    return wg, L * 8


class Csr:
    """Device CSR (int32 indices, fp32 values) with sorted columns."""

    def __init__(self, mat, dev):
        m = mat.tocsr().copy()
        m.sum_duplicates()
        m.sort_indices()
        if m.nnz >= 2 ** 31:
            raise ValueError("matrix too large for int32 CSR")
        self.shape = m.shape
        self.nnz = int(m.nnz)
        self.rowptr = _dev_i32(m.indptr, dev)
        self.col = _dev_i32(m.indices, dev)
        self.val = _dev_f32(m.data.astype(np.float32), dev)     # run.py:103-109 casts the fp64 values to fp32
        self.host = m
        self.dev = dev
        self._plans = {}

    @classmethod
    def from_device(cls, rowptr: torch.Tensor, col: torch.Tensor, val: torch.Tensor, shape):
        """A Csr over arrays that are ALREADY on the device and canonical (int32 rowptr [rows + 1] / col, fp32 val, columns sorted and
        distinct inside a row): they are kept as they are, and downloaded once into the host matrix the plan builders read -- no
        `sum_duplicates`, no `sort_indices`, no upload."""
        import scipy.sparse as sp
        if rowptr.dtype != torch.int32 or col.dtype != torch.int32 or val.dtype != torch.float32:
            raise TypeError("Csr.from_device takes int32 rowptr / col and fp32 val")
        if rowptr.numel() != int(shape[0]) + 1 or col.numel() != val.numel():
            raise ValueError("Csr.from_device: array lengths do not fit the shape")
        self = cls.__new__(cls)
        self.shape = (int(shape[0]), int(shape[1]))
        self.nnz = int(col.numel())
        self.rowptr, self.col, self.val = rowptr.contiguous(), col.contiguous(), val.contiguous()
        m = sp.csr_matrix((val.cpu().numpy(), col.cpu().numpy(), rowptr.cpu().numpy()), shape=self.shape)
        m.has_sorted_indices = True
        m.has_canonical_format = True
        self.host = m
        self.dev = val.device
        self._plans = {}
        return self

    def entries(self) -> torch.Tensor:
        """(column, bits of the value) per stored entry, interleaved int32 (what k_spmm_rowline fetches with one 8-byte load)."""
        e = self._plans.get("entries")
        if e is None:
            e = self._plans["entries"] = torch.stack((self.col, self.val.view(torch.int32)), 1).contiguous()
        return e

    def plan(self, rows_sel: Optional[np.ndarray] = None, key=None, seg: Optional[int] = None, col_ranges: int = 1):
        """Segment tables for ggad_spmm_csr_f32 / ggad_spmm_sliced_f32 (whole matrix, or the row subset `rows_sel`); cached.
        `seg`: segment length (default: the 64 of the wave-per-segment kernel).  `col_ranges` > 1: segments never cross
        the boundaries of that many equal column ranges and are launched range by range (columns are sorted inside a row,
        so a row is cut where its columns cross a boundary) -- the gathered operand rows of one phase then fit an L2."""
        key = "all" if rows_sel is None else key
        if key is not None and (seg is not None or col_ranges > 1):
            key = (key, "seg", seg, col_ranges)
        p = self._plans.get(key) if key is not None else None
        if p is not None:
            return p
        seg = int(_lib.load().ggad_spmm_seg_len()) if seg is None else int(seg)
        rp = self.host.indptr.astype(np.int64)
        rows = np.arange(self.shape[0], dtype=np.int64) if rows_sel is None else np.asarray(rows_sel, dtype=np.int64)
        beg, end = rp[rows], rp[rows + 1]
        if col_ranges > 1:
            # runs of (row, column range): cut positions inside every selected row
            width = -(-self.shape[1] // int(col_ranges))
            bounds = np.arange(1, int(col_ranges), dtype=np.int64) * width
            cnt = end - beg
            tot = int(cnt.sum())
            off = np.zeros(len(rows) + 1, dtype=np.int64)
            np.cumsum(cnt, out=off[1:])
            pos = np.repeat(beg - off[:-1], cnt) + np.arange(tot, dtype=np.int64)        # CSR position of every selected entry
            bucket = np.searchsorted(bounds, self.host.indices[pos], side="right")
            owner_e = np.repeat(np.arange(len(rows), dtype=np.int64), cnt)
            keyv = owner_e * int(col_ranges) + bucket
            start = np.flatnonzero(np.concatenate(([True], keyv[1:] != keyv[:-1]))) if tot else np.zeros(0, dtype=np.int64)
            run_beg = pos[start] if tot else np.zeros(0, dtype=np.int64)
            run_len = np.diff(np.concatenate((start, [tot]))) if tot else np.zeros(0, dtype=np.int64)
            run_row, run_bucket = owner_e[start], bucket[start]
            empty = np.flatnonzero(cnt == 0)                                              # rows without entries keep one empty segment
            run_beg = np.concatenate((run_beg, beg[empty]))
            run_len = np.concatenate((run_len, np.zeros(len(empty), dtype=np.int64)))
            run_row = np.concatenate((run_row, empty))
            run_bucket = np.concatenate((run_bucket, np.zeros(len(empty), dtype=np.int64)))
            o = np.lexsort((run_bucket, run_row))                                         # row-major: slots of a row are consecutive
            run_beg, run_len, run_row, run_bucket = run_beg[o], run_len[o], run_row[o], run_bucket[o]
        else:
            run_beg, run_len, run_row = beg, end - beg, np.arange(len(rows), dtype=np.int64)
            run_bucket = np.zeros(len(rows), dtype=np.int64)
        npiece = np.maximum(1, (run_len + seg - 1) // seg)
        firstp = np.zeros(len(run_beg) + 1, dtype=np.int64)
        np.cumsum(npiece, out=firstp[1:])
        total = int(firstp[-1])
        run_of = np.repeat(np.arange(len(run_beg), dtype=np.int64), npiece)              # run of every segment (slot order)
        k = np.arange(total, dtype=np.int64) - firstp[run_of]
        sbeg = run_beg[run_of] + k * seg
        send = np.minimum(run_beg[run_of] + run_len[run_of], sbeg + seg)
        owner = run_row[run_of]                                                           # output row of every segment
        nseg = np.bincount(owner, minlength=len(rows)).astype(np.int64)                  # segments per output row
        first = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum(nseg, out=first[1:])                                                    # slot order == (row, range, piece) order
        single = nseg[owner] == 1
        seg_out = np.where(single, owner, -(np.arange(total, dtype=np.int64) + 1))       # < 0: partial sum slot = -seg_out - 1
        if col_ranges > 1:
            launch = np.argsort(run_bucket[run_of], kind="stable")                        # launch order: column range by range
            sbeg, send, seg_out = sbeg[launch], send[launch], seg_out[launch]
        multi = np.nonzero(nseg > 1)[0]
        dev = self.dev
        p = dict(seg_beg=_dev_i32(sbeg, dev), seg_end=_dev_i32(send, dev), seg_out=_dev_i32(seg_out, dev), n_seg=total,
                 multi_row=_dev_i32(multi, dev), multi_first=_dev_i32(first[multi], dev), multi_count=_dev_i32(nseg[multi], dev),
                 n_multi=int(len(multi)), n_out=int(len(rows)), part=None, nnz=int((end - beg).sum()),
                 rows=None if rows_sel is None else rows)
        if key is not None:
            self._plans[key] = p
        return p

    def sliced_plan(self, p):
        """The rows of segment plan `p` in the long segments the sliced kernel walks (8 index loads, one reduction and store per
        wave), cut into GGAD_SPMM_COL_RANGES column ranges (default 1).  Cached on the plan, per range count."""
        # (more than one range launches range by range so that one phase's operand rows fit an L2 -- measured slower, 1.35 -> 1.67 ms
        # with 2 ranges on T-Finance: the sliced kernel is bound by the L1 line rate, not by L2 capacity, and shorter segments cost
        # more prologues; kept for experiments)
        ranges = max(1, int(os.environ.get("GGAD_SPMM_COL_RANGES", 1)))
        long = p.setdefault("long", {})
        if ranges not in long:
            long[ranges] = self.plan(p["rows"], key=None, seg=int(_lib.load().ggad_spmm_sliced_seg_len()), col_ranges=ranges)
        return long[ranges]

    def rowslice_plan(self, p, lines: bool = False):
        """Units of the column-sliced kernel for sparse neighbourhoods (k_spmm_rowslice) for the rows of segment plan `p` (whole
        matrix or a row subset): rows sorted by length into groups of 6 (8 for the line-granular variant, `lines`), rows of more
        than `ggad_spmm_rowslice_long()` entries apart.  Cached on the plan."""
        slot = "rowline" if lines else "rowslice"
        rs = p.get(slot)
        if rs is not None:
            return rs
        lib = _lib.load()
        G, SHORT, LONG = int(lib.ggad_spmm_rowslice_group()), int(lib.ggad_spmm_rowslice_short()), int(lib.ggad_spmm_rowslice_long())
        if lines:
            G = 8
        rp = self.host.indptr.astype(np.int64)
        rows = np.arange(self.shape[0], dtype=np.int64) if p.get("rows") is None else np.asarray(p["rows"], dtype=np.int64)
        outr = np.arange(len(rows), dtype=np.int64)
        deg = rp[rows + 1] - rp[rows]
        is_short, is_hub = deg <= SHORT, deg > LONG
        is_med = ~is_short & ~is_hub
        order = np.argsort(-deg[is_short], kind="stable")
        sr, so = rows[is_short][order], outr[is_short][order]
        n_units = (len(sr) + G - 1) // G
        ur = np.full(n_units * G, -1, dtype=np.int64)
        uo = np.zeros(n_units * G, dtype=np.int64)
        ur[:len(sr)], uo[:len(so)] = sr, so
        mo = np.argsort(-deg[is_med], kind="stable")                    # longest first: they start first
        ho = np.argsort(-deg[is_hub], kind="stable")
        dev = self.dev
        if lines:                                                       # (first entry, end, output row, 0) per slot: k_spmm_rowline
            def tab(r, o):
                t = np.zeros((len(r), 4), dtype=np.int32)
                ok = r >= 0
                t[ok, 0], t[ok, 1] = rp[r[ok]], rp[r[ok] + 1]
                t[:, 2] = np.where(ok, o, -1)
                return torch.from_numpy(t.reshape(-1)).to(dev)
            rs = dict(unit_tab=tab(ur, uo), n_units=int(n_units), long_tab=tab(rows[is_med][mo], outr[is_med][mo]), n_long=int(is_med.sum()),
                      hub_tab=tab(rows[is_hub][ho], outr[is_hub][ho]), n_hub=int(is_hub.sum()))
        else:
            rs = dict(unit_rows=_dev_i32(ur, dev), unit_out=_dev_i32(uo, dev), n_units=int(n_units),
                      long_rows=_dev_i32(rows[is_med][mo], dev), long_out=_dev_i32(outr[is_med][mo], dev), n_long=int(is_med.sum()),
                      hub_rows=_dev_i32(rows[is_hub], dev), hub_out=_dev_i32(outr[is_hub], dev), n_hub=int(is_hub.sum()))
        p[slot] = rs
        return rs

    def value_factors(self):
        """(rs, cs, diag) such that value[i][j] = rs[i] * cs[j] off the diagonal (to fp32 round-off) and value[i][i] = diag[i] --
        the shape `normalize_adj` (`utils.py:47-54`: D^-1/2 A D^-1/2 of a 0/1 matrix, with or without self loops, `+ I`
        afterwards or not) gives every adjacency of this code base.  (None, None, None): all stored values are 1.
        False: the values do not factor (the LDS-panel product is then not used).  Host arrays, cached."""
        f = self._plans.get("factors")
        if f is not None:
            return f
        m = self.host
        val = np.ascontiguousarray(m.data, dtype=np.float32)
        f = False
        if np.all(val == np.float32(1.0)):
            f = (None, None, None)
        elif m.shape[0] == m.shape[1]:
            n = m.shape[0]
            lib = _lib.load()
            rowptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
            colv = np.ascontiguousarray(m.indices, dtype=np.int32)
            cnt = np.diff(rowptr)
            diag = m.diagonal().astype(np.float32)
            n_off = cnt - (diag != 0)
            for degree in (n_off, cnt):                                   # normalize_adj(A) [+ I]  /  normalize_adj(A + I)
                with np.errstate(divide="ignore"):
                    r = np.power(degree.astype(np.float64), -0.5)
                r[np.isinf(r)] = 0.0
                ok = int(lib.ggad_spmm_panel_values_factor(rowptr.ctypes.data, colv.ctypes.data, val.ctypes.data, r.ctypes.data, n,
                                                           4e-7, 0))
                if ok < 0:
                    raise _lib.GgadKernelError("ggad_spmm_panel_values_factor: invalid arguments")
                if ok == 1:
                    r32 = r.astype(np.float32)
                    f = (r32, r32, diag if np.any(diag != 0) else None)
                    break
        self._plans["factors"] = f
        return f

    def panel_plan(self, n_slices: int, rows_sel: Optional[np.ndarray] = None, cache: Optional[dict] = None):
        """Entry stream, directory, row table and workgroup table of `ggad_spmm_panel_f32` (layout described at k_spmm_panel in
        fullgraph.hip) for the whole matrix or the row subset `rows_sel` (output row i = matrix row rows_sel[i]), or None when
        the values do not factor / the step slots would be less than 40 % full / a row subset has a separate diagonal.
        Built in the library (0.1 s at 21 M entries), cached per slice count (in `cache`, default: on the matrix)."""
        key = ("panel", int(n_slices))
        store = self._plans if cache is None else cache
        if key in store:
            return store[key]
        lib = _lib.load()
        R, NW, KR = int(lib.ggad_spmm_panel_rows()), int(lib.ggad_spmm_panel_waves()), int(lib.ggad_spmm_panel_rounds())
        fac = self.value_factors()
        plan = None
        if fac is not False and (rows_sel is None or fac[2] is None):
            plan = self._build_panel(int(n_slices), R, NW, KR, fac, rows_sel)
        store[key] = plan
        return plan

    def _build_panel(self, n_slices, R, NW, KR, fac, rows_sel=None):
        lib = _lib.load()
        m = self.host
        rowptr, colv, skip_diag, cnt, rows = _plan_rows(m, fac[2], rows_sel)
        lay = _round_layout(cnt, rows, n_slices, NW, KR)
        if lay is None:
            return None
        nnz, n_rounds, nb, kr, round_rows, round_out, round_wide = lay
        NC = (m.shape[1] + R - 1) // R
        steps_rc = np.empty(n_rounds * NC, dtype=np.int32)
        hp = lambda a: a.ctypes.data
        _lib.check(lib.ggad_spmm_panel_count(hp(rowptr), hp(colv), n_rounds, hp(round_rows), hp(round_wide), skip_diag, R, NC,
                                             hp(steps_rc), 0), "ggad_spmm_panel_count")
        # work of a round = its quads over all panels (the longest of its 8 rows counts); a workgroup waits at two barriers per
        # panel for its slowest wave
        octs_rc = (steps_rc.astype(np.int64) + 7) // 8
        quads_rc = (steps_rc.astype(np.int64) + 3) // 4                   # what the kernel walks: whole octs, then half of the last one
        blk_of_round, wave_of_round, k_of_round = _deal_rounds(quads_rc.reshape(n_rounds, NC).sum(1), nb, NW, KR)
        gwave_of_round = blk_of_round * NW + wave_of_round                # (block, wave)
        n_tiles = nb * NW * NC * KR
        tq = np.zeros(n_tiles, dtype=np.int64)                            # octs (8 steps = one 16-byte load per lane) per tile
        tile_of_rc = ((gwave_of_round[:, None] * NC + np.arange(NC, dtype=np.int64)[None, :]) * KR + k_of_round[:, None]).reshape(-1)
        tq[tile_of_rc] = octs_rc
        th = np.zeros(n_tiles, dtype=np.int64)                            # quads (4 steps) walked per tile: 2 * octs or 2 * octs - 1
        th[tile_of_rc] = quads_rc
        total_q = int(tq.sum())
        fill = nnz / float(max(1, int(th.sum())) * 32)
        if fill < 0.4 or total_q + 8 >= 2 ** 28 or int(th.max()) > 0xffff:
            return None
        offq = np.zeros(n_tiles + 1, dtype=np.int64)
        np.cumsum(tq, out=offq[1:])
        tile_oct = np.ascontiguousarray(offq[tile_of_rc])
        stream = np.empty((total_q + 8) * 64, dtype=np.uint16)            # [oct][lane group][step]: panel row index; 8 spare octs (read-ahead)
        _lib.check(lib.ggad_spmm_panel_fill(hp(rowptr), hp(colv), n_rounds, hp(round_rows), hp(round_wide), skip_diag, R, NC,
                                            hp(steps_rc), hp(tile_oct), hp(stream), total_q, 8, 0), "ggad_spmm_panel_fill")
        stream = stream.view(np.uint32)
        tq2 = th.reshape(nb * NW * NC, KR).astype(np.uint32)             # the directory counts quads
        dirv = np.zeros((nb * NW * NC, 8), dtype=np.uint32)
        dirv[:, 0] = offq[:-1].reshape(nb * NW * NC, KR)[:, 0].astype(np.uint32)
        for k in range(KR):
            dirv[:, 1 + (k >> 1)] |= tq2[:, k] << np.uint32(16 * (k & 1))
        row_tab = np.full((nb * NW * KR, 8), -1, dtype=np.int32)
        row_tab[gwave_of_round * KR + k_of_round] = round_out
        wg, n_wg = _xcd_workgroup_table(n_slices, nb)
        dev = self.dev
        as_i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
        return dict(wg=_dev_i32(wg, dev), n_wg=int(n_wg), dir=as_i32(dirv), stream=as_i32(stream), row_tab=_dev_i32(row_tab, dev),
                    n_chunks=int(NC), fill=fill, blocks=int(nb), rounds=int(kr), **_scale_vectors(fac, rows, dev))

    def ring_plan(self, n_slices: int, rows_sel: Optional[np.ndarray] = None, cache: Optional[dict] = None):
        """Quad stream, control bytes, per-wave extents, row table and workgroup table of `ggad_spmm_ring_f32` (layout described at
        k_spmm_ring in fullgraph.hip and in csrc/spmm_ring_build.cpp) for the whole matrix or the row subset `rows_sel`, or None
        under the conditions of `panel_plan`.  Cached per slice count."""
        key = ("ring", int(n_slices), os.environ.get("GGAD_RING_XCD", "slice"))
        store = self._plans if cache is None else cache
        if key in store:
            return store[key]
        fac = self.value_factors()
        plan = None
        if fac is not False and (rows_sel is None or fac[2] is None):
            lib = _lib.load()
            plan = self._build_ring(int(n_slices), fac, rows_sel, int(lib.ggad_spmm_ring_walkers()))
            # round 6: ONE loader wave is issue-bound (~100 clocks per 1-KB LDS-DMA instruction: ~2 us per 416-row slot).  The products over
            # a row subset and their transposes (10-20 steps per walker and phase) waited for it outright -- 276 -> 153 us (T-Finance loss
            # rows), 92 -> 52 us (Amazon) with three loader waves and 13 walkers -- and so did the whole-matrix product at Amazon size
            # (56 steps per phase: 112.6 -> 93.8 us); at T-Finance size (91 steps) 13 walkers are 2 % faster than 15.  Same-box sweep,
            # profiles/r06_ring_loaders_ab.log: epochs 2.013 -> 1.868 ms (T-Finance), 0.730 -> 0.639 (Amazon).  So every plan takes the
            # three-loader variant; GGAD_RING_SUBSET_STEPS = the steps per walker and phase below which a plan does (0: never = round 5).
            lim = float(os.environ.get("GGAD_RING_SUBSET_STEPS", "1e9"))
            if plan is not None and plan["steps_per_phase"] < lim and int(lib.ggad_spmm_ring_walkers_subset()) != plan["walkers"]:
                alt = self._build_ring(int(n_slices), fac, rows_sel, int(lib.ggad_spmm_ring_walkers_subset()))
                if alt is not None:
                    plan = alt
        store[key] = plan
        return plan

    def _build_ring(self, n_slices, fac, rows_sel=None, NW=None):
        lib = _lib.load()
        RS, S, V = int(lib.ggad_spmm_ring_slot_rows()), int(lib.ggad_spmm_ring_slots()), int(lib.ggad_spmm_ring_window())
        KR = int(lib.ggad_spmm_ring_rounds())
        NW = int(lib.ggad_spmm_ring_walkers()) if NW is None else int(NW)
        m = self.host
        rowptr, colv, skip_diag, cnt, rows = _plan_rows(m, fac[2], rows_sel)
        lay = _round_layout(cnt, rows, n_slices, NW, KR)
        if lay is None:
            return None
        nnz, n_rounds, nb, kr, round_rows, round_out, round_wide = lay
        NP = (m.shape[1] + RS - 1) // RS                                  # phases = slots of the operand
        quads = np.empty(n_rounds * NP, dtype=np.uint16)
        hp = lambda a: a.ctypes.data
        _lib.check(lib.ggad_spmm_ring_count(hp(rowptr), hp(colv), n_rounds, hp(round_rows), hp(round_wide), skip_diag, RS, S, V, NP,
                                            hp(quads), 0), "ggad_spmm_ring_count")
        quads = quads.reshape(n_rounds, NP)
        work = quads.astype(np.int64).sum(1)
        fill = nnz / float(max(1, int(work.sum())) * 32)
        if fill < 0.4:
            return None
        blk_of_round, wave_of_round, k_of_round = _deal_rounds(work, nb, NW, KR)
        gw_of_round = blk_of_round * NW + wave_of_round
        n_gw = nb * NW
        # stream of a walker: phase-major, inside a phase its rounds in accumulator order; a phase without work gets one dummy quad
        # (zero rows) that carries the end-of-phase flag -- every walker meets every barrier
        if n_gw * NP * (KR + 1) * 32 > (4 << 30):                         # the dense (walker, phase, slot) host tables below: ~32 B per cell
            return None                                                  # (a very large operand: the panel / sliced kernels take it)
        tab = np.zeros((n_gw, NP, KR + 1), dtype=np.int64)
        tab[gw_of_round, :, k_of_round] = quads
        tab[:, :, KR] = tab[:, :, :KR].sum(2) == 0
        flat = tab.reshape(n_gw, NP * (KR + 1))
        ends = np.cumsum(flat, axis=1)                                   # quads of the walker up to and including (phase, slot)
        tq = ends[:, -1]
        nsb = (tq + 3) // 4
        sb_off = np.zeros(n_gw + 1, dtype=np.int64)
        np.cumsum(nsb, out=sb_off[1:])
        total_sb = int(sb_off[-1])
        if total_sb * 128 >= 2 ** 31:
            return None
        starts = (ends - flat).reshape(n_gw, NP, KR + 1) + (sb_off[:-1] * 4)[:, None, None]
        quad_off = np.ascontiguousarray(starts[gw_of_round, :, k_of_round])         # (n_rounds, NP): absolute quad of every tile
        # control byte per quad: accumulator offset (4 * slot) in bits 0..5, bit 6 = last quad of its phase
        ctl = np.zeros((total_sb + 2) * 4, dtype=np.uint8)
        kbyte = np.tile(np.concatenate((np.arange(KR, dtype=np.int64) * 4, [0])), NP)
        for g_ in range(n_gw):
            base = int(sb_off[g_]) * 4
            ctl[base:base + int(tq[g_])] = np.repeat(kbyte, flat[g_]).astype(np.uint8)
            phase_end = ends[g_].reshape(NP, KR + 1)[:, -1] - 1 + base
            ctl[phase_end] |= 0x40
        idx = np.empty((total_sb + 2) * 128, dtype=np.uint16)            # two spare super-blocks: the walk requests its stream two ahead
        _lib.check(lib.ggad_spmm_ring_fill(hp(rowptr), hp(colv), n_rounds, hp(round_rows), hp(round_wide), skip_diag, RS, S, V, NP,
                                           hp(np.ascontiguousarray(quads.reshape(-1))), hp(quad_off.reshape(-1)), hp(idx), total_sb + 2, 0),
                   "ggad_spmm_ring_fill")
        wave_sb = np.stack((sb_off[:-1], nsb), axis=1).astype(np.int32)
        row_tab = np.full((n_gw * KR, 8), -1, dtype=np.int32)
        row_tab[gw_of_round * KR + k_of_round] = round_out
        wg, n_wg = _xcd_workgroup_table(n_slices, nb, os.environ.get("GGAD_RING_XCD", "slice") == "block")
        dev = self.dev
        t16 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev)
        per_phase = flat.reshape(n_gw, NP, KR + 1).sum(2)                 # quads per (walker, phase): the barrier waits for the longest
        return dict(wg=_dev_i32(wg, dev), n_wg=int(n_wg), wave_sb=_dev_i32(wave_sb, dev), idx=t16(idx),
                    ctl=torch.from_numpy(ctl.view(np.int32)).to(dev), row_tab=_dev_i32(row_tab, dev), n_phases=int(NP),
                    fill=fill, blocks=int(nb), rounds=int(kr), quads=int(tq.sum()),
                    phase_skew=float(per_phase.reshape(nb, NW, NP).max(1).sum() / max(1.0, per_phase.sum() / NW)),
                    walkers=int(NW), steps_per_phase=float(4.0 * tq.sum() / max(1, n_gw * NP)), **_scale_vectors(fac, rows, dev))
