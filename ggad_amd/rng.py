"""torch's CPU generator, continued on the device (csrc/rng.hip).

The reference draws its per-epoch Gaussian noise with `torch.randn` from the CPU generator, and its numbers are reproduced only
because the same values are drawn in the same order.  `DeviceMT` takes a snapshot of that generator (MT19937: 624 words and a read
position), keeps it in HBM, and `randn_` writes what `torch.randn(n) * scale + shift` would have returned while advancing the state on
the device -- so the draw can be a node of a captured epoch and every replay draws the next values.  `to_host` hands the advanced state
back to the host generator.  Values agree with the host's to float32 rounding of log / sin / cos (not bit for bit); the state, and
with it the number of words consumed, is exact.

Layout of `torch.get_rng_state()` (5,056 bytes), read as uint64 words: [0] seed, [1] `left` (low 32 bits) and `seeded` (high 32 bits),
[2] `next`, [3:627] the 624 state words, then the cached-normal fields of the n < 16 path, which pass through untouched.  The engine
regenerates its block when `left` reaches 1: a freshly seeded generator has left = 1, next = 0, a running one left = 625 - next.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

MT_N = 624
STATE_BYTES = 5056
MIN_DRAW = 16       # torch.randn below 16 elements is a different algorithm (double-precision pairs with a cached second value)


def parse_rng_state(state: torch.Tensor):
    """(words, pos): the 624 MT19937 words (uint32) of a `torch.get_rng_state()` tensor and how many of them are consumed (0..624;
    624: the next draw regenerates the block first)."""
    raw = np.ascontiguousarray(state.numpy() if isinstance(state, torch.Tensor) else np.asarray(state, dtype=np.uint8))
    if raw.dtype != np.uint8 or raw.size != STATE_BYTES:
        raise ValueError(f"not a CPU generator state: expected {STATE_BYTES} bytes of uint8, got {raw.size} of {raw.dtype}")
    q = raw.view(np.uint64)
    left, seeded, nxt = int(q[1] & np.uint64(0xFFFFFFFF)), int(q[1] >> np.uint64(32)), int(q[2])
    if seeded != 1:
        raise ValueError("the CPU generator state is not seeded")
    if left == 1 and nxt in (0, MT_N):
        pos = MT_N
    elif 1 < left <= MT_N and nxt == MT_N + 1 - left:
        pos = nxt
    else:
        raise ValueError(f"inconsistent CPU generator state: left = {left}, next = {nxt}")
    words = q[3:3 + MT_N]
    if (words >> np.uint64(32)).any():
        raise ValueError("the CPU generator state holds words wider than 32 bits")
    return words.astype(np.uint32), pos


def format_rng_state(template: torch.Tensor, words, pos: int) -> torch.Tensor:
    """A `torch.set_rng_state` tensor: `template` (a `torch.get_rng_state()`) with the 624 words and the position replaced; every other
    byte (seed, cached normals) is the template's."""
    words = np.ascontiguousarray(np.asarray(words)).astype(np.uint32)
    pos = int(pos)
    if words.shape != (MT_N,) or not 0 <= pos <= MT_N:
        raise ValueError("need 624 words and a position in 0..624")
    old_words, old_pos = parse_rng_state(template)
    out = template.clone()
    q = out.numpy().view(np.uint64)
    if pos == MT_N and old_pos == MT_N and np.array_equal(words, old_words):
        return out                                  # nothing was drawn from a block that was due: keep the template's spelling of it
    q[3:3 + MT_N] = words.astype(np.uint64)
    q[2] = np.uint64(pos)
    q[1] = (np.uint64(1) << np.uint64(32)) | np.uint64(MT_N + 1 - pos)
    return out


def _check_buffer(buf: torch.Tensor) -> int:
    if not isinstance(buf, torch.Tensor) or buf.dtype != torch.float32:
        raise ValueError("DeviceMT.randn_ fills float32 tensors only")
    if not buf.is_contiguous():
        raise ValueError("DeviceMT.randn_ needs a contiguous buffer")
    n = buf.numel()
    if n < MIN_DRAW:
        raise ValueError(f"DeviceMT.randn_ draws at least {MIN_DRAW} values (torch.randn below that is a different algorithm)")
    return n


class DeviceMT:
    """MT19937 state of torch's CPU generator in device memory."""

    def __init__(self, dev, words, pos: int, template: torch.Tensor | None = None):
        lib = _lib.load()
        self.dev = torch.device(dev)
        block = np.zeros(int(lib.ggad_mt_state_words()), dtype=np.uint32)
        block[:MT_N] = np.asarray(words, dtype=np.uint32)
        block[MT_N] = int(pos)
        self.state = torch.from_numpy(block.view(np.int32)).to(self.dev)
        self.template = template.clone() if template is not None else torch.get_rng_state()
        self.scratch = None

    @classmethod
    def from_host(cls, dev) -> "DeviceMT":
        """Snapshot of torch's default CPU generator (which is left as it is until `to_host`)."""
        st = torch.get_rng_state()
        words, pos = parse_rng_state(st)
        return cls(dev, words, pos, st)

    def reserve(self, n: int) -> None:
        """Scratch for draws of up to n values (the raw words): call outside a capture."""
        need = int(_lib.load().ggad_mt_randn_scratch_elems(int(n)))
        if self.scratch is None or self.scratch.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DeviceMT scratch must exist before a capture: call reserve(n) or draw once eagerly first")
            self.scratch = torch.empty(need, dtype=torch.int32, device=self.dev)

    def randn_(self, buf: torch.Tensor, scale: float = 1.0, shift: float = 0.0) -> torch.Tensor:
        """buf <- what `torch.randn(buf.shape) * scale + shift` returns on the host, advancing the device state.  One call into the
        library on the current stream; no allocation once the scratch exists, no host read."""
        n = _check_buffer(buf)
        if buf.device != self.state.device:
            raise ValueError("DeviceMT.randn_: the buffer is not on the generator's device")
        self.reserve(n)
        _lib.call("ggad_mt_randn_f32", _lib.ptr(self.state), _lib.ptr(buf), n, float(scale), float(shift), _lib.ptr(self.scratch))
        return buf

    def state_host(self):
        """(words, pos) of the device state (synchronises)."""
        block = self.state.cpu().numpy().view(np.uint32)
        return block[:MT_N].copy(), int(block[MT_N])

    def to_host(self) -> None:
        """Hand the stream back: the next host `torch.randn` continues where the device stopped."""
        words, pos = self.state_host()
        torch.set_rng_state(format_rng_state(self.template, words, pos))
