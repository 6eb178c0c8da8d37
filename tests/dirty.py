"""Dirty, reused memory for the kernels that take a workspace (tests/test_dirty_memory_gpu.py).

Outputs and workspaces are carved out of NaN-filled blocks with a guard zone on both sides, so that an element a kernel does not
store stays NaN, a word it reads before writing it poisons the result, and a store outside the tensor breaks a sentinel.
`run_sequence` drives one entry point the way an epoch does: the larger case A, the smaller case B, A and B again, all on ONE
workspace that was NaN-filled before the first call only, with 32 MB of dirty cache lines between the calls."""
import numpy as np
import torch

DEV = "cuda:0"
GUARD = 64                                   # floats in front of and behind every tensor: 256 bytes, keeps 16-byte alignment
NAN_BITS = 0x7FC00000                        # what torch.full(..., nan) stores
ORDER = ("A", "B", "A", "B")
_JUNK = []


def padded(rows, cols, ld):
    """A (rows, cols) float32 view with row stride `ld` >= cols inside a NaN block: padding columns and guards hold NaN."""
    assert ld >= cols >= 1 and rows >= 1
    block = torch.full((GUARD + rows * ld + GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    t = block[GUARD:GUARD + rows * ld].view(rows, ld)[:, :cols]
    t.dirty_block = (block, rows, cols, ld)        # (an attribute of this tensor object: views of it do not carry it)
    return t


def nan_like(*shape):
    """A contiguous NaN-filled float32 tensor of `shape` (one or two dimensions) with NaN guards around it."""
    rows, cols = (1, shape[0]) if len(shape) == 1 else shape
    t = padded(rows, cols, cols)
    if len(shape) == 1:
        t, t2 = t.view(cols), t
        t.dirty_block = t2.dirty_block
    return t


def int_like(n, fill):
    """int32[n] filled with `fill`, with guards of the same value."""
    block = torch.full((GUARD + n + GUARD,), fill, dtype=torch.int32, device=DEV)
    return block, block[GUARD:GUARD + n]


def guards_intact(t):
    """Bit for bit: the guards in front of and behind `t` and the padding of its rows still hold the NaN they were filled with."""
    block, rows, cols, ld = t.dirty_block
    bits = block.view(torch.int32).clone()
    bits[GUARD:GUARD + rows * ld].view(rows, ld)[:, :cols] = NAN_BITS
    bad = torch.nonzero(bits != NAN_BITS).reshape(-1)
    assert bad.numel() == 0, f"{bad.numel()} words outside the tensor were written, first at float {int(bad[0]) - GUARD} of its block"


def dirty_lines():
    """32 MB of dirty lines between two calls (the `junk.add_(1.0)` of test_handoff_gpu.py)."""
    if not _JUNK:
        _JUNK.append(torch.zeros(8 << 20, device=DEV))
    _JUNK[0].add_(1.0)


def host(o):
    torch.cuda.synchronize()
    return {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in o.items()}


def _tensors(ws):
    return [w for w in (ws if isinstance(ws, (tuple, list)) else (ws,)) if isinstance(w, torch.Tensor) and hasattr(w, "dirty_block")]


def run_sequence(ep):
    """A, B, A, B with k = 0..3 on one workspace.  Every call: bit-equal to the same call on a fresh NaN workspace of exactly its
    own size; no NaN in any element the header says is written (`ep.untouched(x, name)`, where an entry point has one, is the mask
    of the elements that must KEEP their NaN instead); guards and padding of every output and of the workspaces intact; and
    `ep.check`: the float64 reference at the tolerance of the entry point's own test."""
    ep.check_shape()
    ws = ep.workspace("A")
    for k, case in enumerate(ORDER):
        x = ep.inputs(case, k)
        got_t = ep.run(x, ws)
        got = host(got_t)
        dirty_lines()
        own = ep.workspace(case)
        alone_t = ep.run(x, own)
        alone = host(alone_t)
        assert got.keys() == alone.keys()
        for q in got:
            for t in (got_t[q], alone_t[q]):
                guards_intact(t)
            keep = ep.untouched(x, q) if hasattr(ep, "untouched") else None
            if keep is None:
                assert not np.isnan(got[q]).any(), (case, k, q, int(np.isnan(got[q]).sum()))
            else:
                assert np.array_equal(got[q].view(np.int32)[keep], np.full(int(keep.sum()), NAN_BITS, dtype=np.int32)), (case, k, q)
                assert not np.isnan(got[q][~keep]).any(), (case, k, q)
            assert got[q].tobytes() == alone[q].tobytes(), (case, k, q)
        for w in _tensors(ws) + _tensors(own):
            guards_intact(w)
        ep.check(x, got)
