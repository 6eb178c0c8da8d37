"""Cases, float64 reference and runner of tests/test_gemm_routes_gpu.py and tests/test_gemm_routes_cpu.py  --  TEST INFRASTRUCTURE.

`ggad_gemm_f32` is one entry point in front of seven kernels ("GEMM routes").  Every case below names a product -- M, N,
K, the layout, the padding of the three row strides, an offset of A's pointer -- and the kernel it must reach: the route and variant
that `ggad_gemm_last_route()` reports (include/ggad_hip.h), and for the split-K routes how many trailing splits have an empty K
range.  Where bias + ReLU send the product elsewhere (the row-range kernel takes no epilogue) the case names that route too.  The
routes are written down here from the conditions of csrc/gemm.hip and csrc/gemm_slab.hip, shape by shape; nothing in this module
predicts them from the code under test, and tests/test_gemm_routes_cpu.py holds the split arithmetic against the library.

The reference is numpy in float64 on the same float32 operands.  `run_case` makes the direct C-ABI call with explicit strides:
operands in NaN-padded blocks, C a view of a NaN block with guards (tests/dirty.py), the workspace NaN-filled before the first call.
Run as a program (`python tests/gemm_fp64.py --group tiled`) it runs one group in THIS process and prints one JSON line per case:
the switches the library reads once per process (GGAD_GEMM_DMA, _SCALAR, _TM, _DMA_BUFS) are tested that way, one child each.
"""
import json
import os
import sys

import numpy as np

BOUND = 2e-6                      # max |got - ref| / (max |ref| + 1): what test_gemm_f32_all_layouts holds these kernels to, up to K = 10984
ROUTES = ("NONE", "SLAB", "BRES", "WGRAD_TN", "SMALL", "DMA", "DMA_SPLITK", "TILED", "TILED_SPLITK")      # enum ggad_gemm_route
SPLIT_ROUTES = ("DMA_SPLITK", "TILED_SPLITK")


# ---- the variant of a route, packed as the GGAD_GEMM_VARIANT_* macros of include/ggad_hip.h pack it
def v_tn(vp, vq):
    return vp << 4 | vq


def v_dma(splits, bufs=2):
    return splits | bufs << 8


def v_tiled(splits, vec, tm=64):
    return splits | vec << 8 | tm << 10


def describe(route, variant):
    if route in ("SLAB", "BRES"):
        return f"{route}<{variant}>"
    if route == "WGRAD_TN":
        return f"WGRAD_TN vp={variant >> 4} vq={variant & 15}"
    if route in ("DMA", "DMA_SPLITK"):
        return f"{route} splits={variant & 255} bufs={variant >> 8}"
    if route in ("TILED", "TILED_SPLITK"):
        return f"{route} splits={variant & 255} vec={variant >> 8 & 3} tm={variant >> 10}"
    return route


def splits_of(variant):
    return variant & 255


# ---- `gemm_splits` of csrc/gemm.hip restated (tests/test_gemm_routes_cpu.py checks it against ggad_gemm_workspace_elems)
def _cdiv(a, b):
    return -(-a // b)


def gemm_splits(M, N, K, tm=64):
    """(splits, K per split rounded up to BK = 32) of the tiled kernels; (1, K) = no split."""
    tiles = _cdiv(M, tm) * _cdiv(N, 64)
    if K < 512 or tiles >= 256:
        return 1, K
    s = max(512 // tiles, 1)
    s = max(min(s, _cdiv(K, 256) if K >= 2048 else _cdiv(K, 128), 128), 1)
    if s == 1:
        return 1, K
    return s, _cdiv(_cdiv(K, s), 32) * 32


def empty_splits(M, N, K, tm=64):
    s, kps = gemm_splits(M, N, K, tm)
    return sum(1 for i in range(s) if i * kps >= K)


def wgrad_tn_ws(K, M, N):
    """`ggad_int_wgrad_tn_ws` of csrc/mlp.hip restated: the partials of the row-range kernel, 0 = shape not taken."""
    if M < 1 or N < 1 or M > 512 or N > 512 or K < 1024 or min(M, N) > 32:
        return 0
    return min(max(1, K // 64), 64) * M * N + 16


# ================================================================================================ the table
CASES = {}


def _case(group, M, N, K, lay, route, variant=0, *, empty=0, br=None, pad=(0, 0, 0), off_a=0, ws=True):
    """lay: "NN" / "NT" / "TN" / "TT" = (A transposed in memory, B transposed in memory).  br: (route, variant, empty) of the bias + ReLU
    call when it differs.  pad: floats added to the row strides of A, B, C.  off_a: floats A's pointer is moved off 16-byte alignment.
    ws=False: the caller passes no workspace (NULL is allowed: the product then runs unsplit)."""
    name = f"{group}-{M}x{N}x{K}-{lay}"
    if pad != (0, 0, 0):
        name += "-pad" + ".".join(str(p) for p in pad)
    if off_a:
        name += f"-offA{off_a}"
    if not ws:
        name += "-nows"
    assert name not in CASES, name
    assert route in ROUTES and (br is None or br[0] in ROUTES)
    CASES[name] = dict(name=name, group=group, M=M, N=N, K=K, ta=lay[0] == "T", tb=lay[1] == "T", route=route, variant=variant, empty=empty,
                       br=br if br is not None else (route, variant, empty), pad=pad, off_a=off_a, ws=ws)


LAYOUTS = ("NN", "NT", "TN", "TT")

# ---- BRES: M >= 16384, 128 <= K <= 320 (K % 4 == 0), 64 < N <= 1024, A K-fast, where the slab kernel declines (KSn 8 .. 15, or < 8 column tiles)
for _i, (_k, _ks) in enumerate(((128, 8), (132, 9), (144, 9), (160, 10), (176, 11), (192, 12), (208, 13), (224, 14), (240, 15))):
    _case("bres", 16384, 100, _k, ("NT", "NN")[_i % 2], "BRES", _ks)                       # both fill loops; K % 16 != 0 at 132
for _i, (_k, _ks, _n) in enumerate(((244, 16, 68), (260, 17, 80), (276, 18, 96), (300, 19, 100), (320, 20, 112))):
    _case("bres", 16384, _n, _k, ("NN", "NT")[_i % 2], "BRES", _ks)                        # n_tiles < 8: not the slab kernel's
_case("bres", 16385, 100, 132, "NT", "BRES", 9)                                            # ragged last row block: clamped rows of A
_case("bres", 16399, 100, 300, "NN", "BRES", 19)
_case("bres", 16384, 65, 128, "NT", "BRES", 8)                                             # 5 tiles: the last slab holds one (TC = 1) of one column
_case("bres", 16384, 81, 260, "NT", "BRES", 17)                                            # 6 tiles, the last of one column
_case("bres", 16384, 1024, 128, "NT", "BRES", 8)                                           # 32 slabs
_case("bres", 16384, 1028, 128, "NT", "DMA", v_dma(1))                                     # N > 1024: declined
_case("bres", 16384, 100, 132, "NT", "BRES", 9, pad=(4, 4, 3))                             # lda > K, ldb > K, ldc > N
_case("bres", 16399, 96, 244, "NN", "BRES", 16, pad=(8, 4, 4))

# ---- SLAB through ggad_gemm_f32: M >= 4096, KSn in {2, 4, 16 .. 20}, >= 8 column tiles that split into slabs of 5 and 4
_case("slab", 4096, 128, 20, "NT", "SLAB", 2)
_case("slab", 4097, 128, 32, "NN", "SLAB", 2)
_case("slab", 4111, 128, 52, "NT", "SLAB", 4)
_case("slab", 4096, 128, 64, "NN", "SLAB", 4)
_case("slab", 4096, 128, 244, "NT", "SLAB", 16)
_case("slab", 4097, 128, 260, "NT", "SLAB", 17)
_case("slab", 4096, 128, 260, "NN", "SLAB", 17)
_case("slab", 4111, 128, 276, "NN", "SLAB", 18)
_case("slab", 4096, 128, 276, "NT", "SLAB", 18)
_case("slab", 4096, 128, 300, "NN", "SLAB", 19)
_case("slab", 4096, 128, 320, "NT", "SLAB", 20)
_case("slab", 4096, 113, 260, "NT", "SLAB", 17)                                            # N % 4 != 0: scalar stores
_case("slab", 4096, 113, 20, "NT", "SLAB", 2)
_case("slab", 4096, 176, 260, "NT", "DMA", v_dma(1))                                       # 11 tiles: no 5 + 4 split with 3 slabs
_case("slab", 4096, 1280, 20, "NT", "SLAB", 2)                                             # 16 slabs
_case("slab", 4096, 1280, 20, "NN", "SLAB", 2)
_case("slab", 4096, 1284, 20, "NT", "TILED", v_tiled(1, 1))                                # 17 slabs: declined (K < 32: not DMA either)
_case("slab", 4095, 128, 260, "NT", "DMA", v_dma(1))                                       # M < 4096: declined
_case("slab", 4096, 128, 260, "NT", "SLAB", 17, pad=(4, 4, 4))                             # 16-byte stores into a padded C
_case("slab", 4097, 128, 276, "NN", "SLAB", 18, pad=(8, 4, 1))                             # ldc % 4 != 0: scalar stores

# ---- SMALL: K <= 512, M <= 1024, M N <= 524288, no workspace
_case("small", 64, 48, 1, "NN", "SMALL")
_case("small", 2, 16384, 512, "NT", "SMALL")                                               # K = 512 with >= 256 tiles: no split, so no workspace
_case("small", 2, 16384, 513, "NT", "TILED", v_tiled(1, 2))
_case("small", 100, 60, 512, "NT", "SMALL", ws=False)                                      # K = 512 from a caller without a workspace
_case("small", 100, 60, 513, "NT", "TILED", v_tiled(1, 2), ws=False)
_case("small", 100, 60, 512, "NT", "DMA_SPLITK", v_dma(4))                                 # K >= 512, few tiles, a workspace: split-K owns it
_case("small", 100, 60, 513, "NN", "TILED_SPLITK", v_tiled(5, 2))
_case("small", 1024, 40, 64, "NN", "SMALL")
_case("small", 1025, 40, 64, "NN", "DMA", v_dma(1))
_case("small", 1024, 512, 16, "NT", "SMALL")                                               # M N = 524288
_case("small", 1024, 513, 16, "NN", "TILED", v_tiled(1, 2))                                # one column more (K < 32: not DMA)
_case("small", 1, 32768, 16, "NN", "SMALL")                                                # 1,024 tiles of 32 x 32: the grid's ceiling
_case("small", 1, 40000, 16, "NN", "TILED", v_tiled(1, 1))                                 # 1,250 tiles: declined by that alone
for _l in LAYOUTS:
    _case("small", 130, 70, 100, _l, "SMALL")
_case("small", 130, 70, 33, "NN", "SMALL")                                                 # K % 4 != 0: the per-float fill
_case("small", 130, 70, 100, "NT", "SMALL", off_a=1)                                       # A off 16-byte alignment: the per-float fill
_case("small", 130, 70, 100, "TN", "SMALL", pad=(3, 5, 2))

# ---- WGRAD_TN: "TN", K >= 1024, min(M, N) <= 32, max <= 512, contiguous C, no epilogue; (vp, vq) by wg_pick_vec.  With bias + ReLU the
# product stays with the split-K tiles: 8 splits of 128 for K = 1024
_case("wgrad", 32, 64, 1024, "TN", "WGRAD_TN", v_tn(2, 4), br=("DMA_SPLITK", v_dma(8), 0))
_case("wgrad", 32, 64, 1023, "TN", "DMA_SPLITK", v_dma(8))                                 # K < 1024: not taken
_case("wgrad", 33, 64, 1024, "TN", "TILED_SPLITK", v_tiled(8, 2))                          # min(M, N) = 33: not taken
_case("wgrad", 8, 512, 1024, "TN", "WGRAD_TN", v_tn(2, 4), br=("DMA_SPLITK", v_dma(8), 0))
_case("wgrad", 8, 516, 1024, "TN", "DMA_SPLITK", v_dma(8))                                 # N = 516: not taken
_case("wgrad", 32, 66, 1024, "TN", "WGRAD_TN", v_tn(2, 2), br=("TILED_SPLITK", v_tiled(8, 2), 0))
_case("wgrad", 31, 64, 1024, "TN", "WGRAD_TN", v_tn(1, 4), br=("TILED_SPLITK", v_tiled(8, 2), 0))
_case("wgrad", 31, 66, 1024, "TN", "WGRAD_TN", v_tn(1, 2), br=("TILED_SPLITK", v_tiled(8, 2), 0))
_case("wgrad", 32, 65, 1024, "TN", "WGRAD_TN", v_tn(1, 1), br=("TILED_SPLITK", v_tiled(8, 2), 0))      # (2, 1) is no instance: (1, 1)
_case("wgrad", 32, 64, 1024, "TN", "WGRAD_TN", v_tn(1, 1), pad=(0, 1, 0), br=("TILED_SPLITK", v_tiled(8, 1), 0))      # odd row stride of B
_case("wgrad", 32, 64, 1024, "TN", "WGRAD_TN", v_tn(1, 4), pad=(1, 0, 0), br=("TILED_SPLITK", v_tiled(8, 1), 0))      # odd row stride of A
_case("wgrad", 20, 300, 1500, "TN", "WGRAD_TN", v_tn(2, 4), br=("DMA_SPLITK", v_dma(12), 0))           # 23 row ranges

# ---- DMA / DMA_SPLITK: 16-byte chunks of both operands aligned and inside one row, K >= 32
for _l in LAYOUTS:
    _case("dma", 1028, 132, 32, _l, "DMA", v_dma(1))                                       # one K-tile
    _case("dma", 1028, 132, 36, _l, "DMA", v_dma(1))                                       # a tail K-tile of 4
    _case("dma", 300, 300, 5124, _l, "DMA_SPLITK", v_dma(20), empty=2)                     # kps = 288: splits 18 and 19 are empty
_case("dma", 1088, 64, 508, "NT", "DMA", v_dma(1))                                         # K < 512: no split
_case("dma", 1088, 64, 512, "NT", "DMA_SPLITK", v_dma(4))                                  # 17 tiles -> 30, capped at ceil(K / 128)
_case("dma", 1088, 64, 2044, "NN", "DMA_SPLITK", v_dma(16))
_case("dma", 1088, 64, 2048, "NN", "DMA_SPLITK", v_dma(8))                                 # K >= 2048: capped at ceil(K / 256)
_case("dma", 512, 512, 1025, "TN", "DMA_SPLITK", v_dma(8), empty=1)                        # kps = 160
_case("dma", 300, 300, 5200, "NT", "DMA_SPLITK", v_dma(20), empty=1)
_case("dma", 300, 300, 8708, "NT", "DMA_SPLITK", v_dma(20))                                # (as 8705 below: three empty splits at 128-row tiles)
_case("dma", 64, 64, 16385, "TN", "DMA_SPLITK", v_dma(65))                                 # the last split holds one k
_case("dma", 300, 300, 5124, "NN", "DMA_SPLITK", v_dma(20), empty=2, pad=(4, 4, 4))

# ---- TILED / TILED_SPLITK in a process with the default switches: what DMA cannot take
for _l in LAYOUTS:
    _case("tiled", 1028, 132, 28, _l, "TILED", v_tiled(1, 1))                              # aligned, K < 32, M > 1024
    _case("tiled", 1027, 131, 37, _l, "TILED", v_tiled(1, 2))                              # float4 loads with the per-float path at the edges
_case("tiled", 4092, 68, 28, "NT", "TILED", v_tiled(1, 1))
for _l in ("NN", "NT", "TT"):
    _case("tiled", 512, 512, 1025, _l, "TILED_SPLITK", v_tiled(8, 2), empty=1)
_case("tiled", 510, 512, 1025, "TN", "TILED_SPLITK", v_tiled(8, 2), empty=1)
_case("tiled", 300, 300, 8705, "NN", "TILED_SPLITK", v_tiled(20, 2))                       # 128-row tiles: 34 splits of 288, 31 .. 33 empty
_case("tiled", 300, 298, 5124, "NN", "TILED_SPLITK", v_tiled(20, 2), empty=2)
_case("tiled", 300, 300, 5200, "NN", "TILED_SPLITK", v_tiled(20, 1), empty=1, pad=(0, 1, 0))      # aligned extents, odd row stride of B
_case("tiled", 64, 64, 16385, "NN", "TILED_SPLITK", v_tiled(65, 2))
_case("tiled", 1027, 131, 37, "NN", "TILED", v_tiled(1, 2), pad=(3, 2, 5))

GROUPS = ("bres", "slab", "small", "wgrad", "dma", "tiled")
SWITCH_GROUP = ("dma", "tiled")                   # what a child process of the read-once switches runs
SWITCHES = ("GGAD_GEMM_DMA=0", "GGAD_GEMM_SCALAR=1", "GGAD_GEMM_TM=128", "GGAD_GEMM_DMA_BUFS=3")


def expected(c, which):
    """(route, variant, empty splits) of the plain call (which = "plain") or of the one with bias + ReLU ("br")."""
    return (c["route"], c["variant"], c["empty"]) if which == "plain" else tuple(c["br"])


def expected_under(c, switch, which):
    """`expected` of a SWITCH_GROUP case in a process started with `switch`."""
    route, variant, empty = expected(c, which)
    assert c["group"] in SWITCH_GROUP
    dma = route in ("DMA", "DMA_SPLITK")
    splits = splits_of(variant)
    vec = 1 if dma else variant >> 8 & 3          # what DMA takes has extents that are multiples of 4
    split_route = lambda s: "TILED_SPLITK" if s > 1 else "TILED"          # noqa: E731
    if switch == "GGAD_GEMM_DMA=0":
        return (split_route(splits), v_tiled(splits, vec), empty) if dma else (route, variant, empty)
    if switch == "GGAD_GEMM_SCALAR=1":
        return (route, variant, empty) if dma else (route, v_tiled(splits, 0), empty)
    if switch == "GGAD_GEMM_TM=128":              # 128-row tiles: another tile count, so other splits; the DMA kernel has no such form
        s, _ = gemm_splits(c["M"], c["N"], c["K"], 128)
        return split_route(s), v_tiled(s, vec, 128), empty_splits(c["M"], c["N"], c["K"], 128)
    if switch == "GGAD_GEMM_DMA_BUFS=3":
        return (route, v_dma(splits, 3), empty) if dma else (route, variant, empty)
    raise ValueError(switch)


# ================================================================================================ reference and runner
def operands(c):
    """The case's float32 operands as they lie in memory: A (K, M) if ta else (M, K), B (N, K) if tb else (K, N), bias (N)."""
    M, N, K = c["M"], c["N"], c["K"]
    rng = np.random.default_rng(7 * M + 3 * N + K + 2 * c["ta"] + c["tb"])
    a = rng.standard_normal((K, M) if c["ta"] else (M, K)).astype(np.float32)
    b = rng.standard_normal((N, K) if c["tb"] else (K, N)).astype(np.float32)
    return a, b, rng.standard_normal(N).astype(np.float32)


def reference(c, a, b, bias):
    """float64: (op(A) op(B), max(op(A) op(B) + bias, 0))."""
    ref = (a.T if c["ta"] else a).astype(np.float64) @ (b.T if c["tb"] else b).astype(np.float64)
    return ref, np.maximum(ref + bias.astype(np.float64), 0.0)


def distance(got, ref):
    if not np.isfinite(got).all():
        return float("inf")
    return float(np.abs(got.astype(np.float64) - ref).max() / (np.abs(ref).max() + 1.0))


def _stage(arr, ld, off=0):
    """`arr` on the device with row stride ld inside a NaN block, `off` floats behind a 256-byte boundary."""
    import torch
    import dirty as D
    rows, cols = arr.shape
    block = torch.full((D.GUARD + off + rows * ld + D.GUARD,), float("nan"), dtype=torch.float32, device=D.DEV)
    view = block[D.GUARD + off:D.GUARD + off + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(torch.from_numpy(arr))
    return view


def run_case(c):
    """Both calls of a case (plain, bias + ReLU), each made twice.  Returns {"plain": r, "br": r}, r = dict(route, variant, err, nans,
    repeat_equal, empty, empty_zero): the recorded route, the distance to float64, NaN left in C, the second call bit-equal to the first
    (on the workspace the first one left behind), and for a split route the number of splits with an empty K range and whether their
    partials in the workspace are all zero (None: there is none).  Guards and the
    padding of C and of the workspace are asserted here (`dirty.guards_intact`)."""
    import torch
    import dirty as D
    from ggad_amd import _lib
    lib = _lib.load()
    M, N, K = c["M"], c["N"], c["K"]
    a, b, bias = operands(c)
    refs = reference(c, a, b, bias)
    lda, ldb, ldc = a.shape[1] + c["pad"][0], b.shape[1] + c["pad"][1], N + c["pad"][2]
    da, db = _stage(a, lda, c["off_a"]), _stage(b, ldb)
    dbias = torch.from_numpy(bias).to(D.DEV)
    sam, sak = (1, lda) if c["ta"] else (lda, 1)
    sbk, sbn = (1, ldb) if c["tb"] else (ldb, 1)
    ws_n = int(lib.ggad_gemm_workspace_elems(M, N, K)) if c["ws"] else 0
    out = {}
    for which, ref in zip(("plain", "br"), refs):
        ws = D.nan_like(ws_n) if ws_n else None
        got = []
        for _ in range(2):
            cbuf = D.padded(M, N, ldc)
            _lib.call("ggad_gemm_f32", da.data_ptr(), db.data_ptr(), cbuf.data_ptr(), M, N, K, sam, sak, sbk, sbn, ldc,
                      dbias.data_ptr() if which == "br" else 0, 1 if which == "br" else 0, ws.data_ptr() if ws is not None else 0)
            route, variant = _lib.gemm_last_route()
            torch.cuda.synchronize()
            D.guards_intact(cbuf)
            if ws is not None:
                D.guards_intact(ws)
            got.append(np.ascontiguousarray(cbuf.cpu().numpy()))
        r = dict(route=route, variant=variant, err=distance(got[0], ref), nans=int(np.isnan(got[0]).sum()),
                 repeat_equal=got[0].tobytes() == got[1].tobytes(), empty_zero=None)
        if route in SPLIT_ROUTES:
            s = splits_of(variant)
            e = r["empty"] = empty_splits(M, N, K, variant >> 10 if route == "TILED_SPLITK" else 64)      # (at the tile height that ran)
            if e:
                r["empty_zero"] = bool((ws[(s - e) * M * N:s * M * N] == 0).all())
        if K > 10984:                              # longer than anything the bound was set on: numpy's own float32 product beside it
            r["err_numpy_f32"] = distance((a.T if c["ta"] else a) @ (b.T if c["tb"] else b), refs[0])
        out[which] = r
    return out


def main(argv):
    groups = argv[argv.index("--group") + 1].split(",")
    for c in CASES.values():
        if c["group"] in groups:
            print(json.dumps(dict(name=c["name"], **run_case(c))), flush=True)
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.exit(main(sys.argv))
