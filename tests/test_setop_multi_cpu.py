"""ukm_setop2_multi without a GPU: the symbol in the header, in lib.SYMBOLS and in both libraries; the binding; the tile
size the GPU tests build their shapes from; and the numpy twins of the shapes that aim at the union's straddle term.

The union's output offset of tile t is d_t - MP[t] + s_t, s_t = 1 when a matched pair straddles
the tile's front boundary: A's record is the last of tile t - 1, B's the first of tile t.  merge_path() below computes the
merge path as the kernels define it (A before B on ties) and straddles() reads s_t off it; straddle_sets() builds the two
shapes tests/test_gpu_setop_multi.py runs: every interior boundary straddled, and none.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
TILE = 9728                     # records per workgroup of setop_multi_tile_kernel: SETOP_NT x SETOP_VT_MULTI = 512 x 19


def merge_path(A, B, tile=TILE):
    """a_t for every boundary t = 0 .. ntiles: how many records of A lie in the first t * tile merged records (A before B
    on ties)"""
    na, nb = len(A), len(B)
    keys = np.concatenate([A, B])
    from_b = np.concatenate([np.zeros(na, np.int8), np.ones(nb, np.int8)])
    order = np.lexsort((from_b, keys))                      # by key, A first among equals
    a_before = np.concatenate([[0], np.cumsum(from_b[order] == 0)])
    ntiles = (na + nb + tile - 1) // tile
    d = np.minimum(np.arange(ntiles + 1) * tile, na + nb)
    return d, a_before[d]


def straddles(A, B, tile=TILE):
    """s_t of every INTERIOR boundary (t = 1 .. ntiles - 1)"""
    d, a = merge_path(A, B, tile)
    out = []
    for dt, at in zip(d[1:-1], a[1:-1]):
        bt = dt - at
        out.append(int(at > 0 and bt < len(B) and A[at - 1] == B[bt]))
    return out


def straddle_sets(mirrored, tile=TILE):
    """A = [10, 11, .., 10 + n], B = [11, .., 10 + n]: the merged order is A10, A11 B11, A12 B12, ... -- the A record of
    pair k stands at the odd position 2k - 1, so every boundary (a multiple of the even tile) falls between the two
    records of a pair.  mirrored: one more record, 5, in front of B: every pair moves one place up and no boundary
    straddles.  n: a little over two tiles of pairs, so that the inputs span five tiles."""
    assert tile % 2 == 0
    n = 2 * tile + 137
    A = np.arange(10, 10 + n + 1, dtype=U64)
    B = np.arange(11, 10 + n + 1, dtype=U64)
    if mirrored:
        B = np.concatenate([np.array([5], dtype=U64), B])
    return A, B


def test_the_straddle_shape_straddles_every_interior_boundary():
    A, B = straddle_sets(False)
    s = straddles(A, B)
    assert len(s) >= 3 and all(x == 1 for x in s), s


def test_the_mirrored_shape_straddles_none():
    A, B = straddle_sets(True)
    s = straddles(A, B)
    assert len(s) >= 3 and all(x == 0 for x in s), s


def test_merge_path_twin_on_a_known_case():
    A = np.array([1, 3, 5, 7], dtype=U64)
    B = np.array([3, 4, 7, 9], dtype=U64)
    d, a = merge_path(A, B, tile=2)          # merged: A1 A3 | B3 B4 | A5 A7 | B7 B9
    assert d.tolist() == [0, 2, 4, 6, 8] and a.tolist() == [0, 2, 2, 4, 4]
    assert straddles(A, B, tile=2) == [1, 0, 1]


def test_tile_constant_matches_the_source():
    # the set-op translation unit: the source and the three headers it is split into (ukm_setops.hip's header comment)
    src = "".join(open(os.path.join(ROOT, "unikmer_amd", "csrc", f)).read()
                  for f in ("ukm_setop_part.h", "ukm_setop_tile.h", "ukm_setop_kernels.h", "ukm_setops.hip"))
    defs = dict(re.findall(r"^#define (SETOP_NT|SETOP_VT|SETOP_VT_MULTI) (\w+)", src, flags=re.M))
    nt = int(defs["SETOP_NT"])
    vt = defs["SETOP_VT_MULTI"]
    vt = int(defs[vt]) if vt in defs else int(vt)
    assert nt * vt == TILE, (nt, vt)
    # ... and these are what the host pass partitions by and launches with
    assert re.search(r"constexpr int NTS = SETOP_NT;", src) and re.search(r"constexpr int VT_MULTI = SETOP_VT_MULTI;", src)
    body = src[src.index("int run_setop_multi_pass("):]
    body = body[:body.index("\n}\n")]
    assert "tile_items = (u64)NTS * VT_MULTI" in body
    assert "setop_multi_tile_kernel<OPS, true, NTS, VT_MULTI>" in src and "setop_multi_tile_kernel<OPS, false, NTS, VT_MULTI>" in src


def test_symbol_is_declared_listed_and_exported_from_both_libraries():
    from unikmer_amd import build, lib
    build.build()
    hdr = open(os.path.join(ROOT, "include", "unikmer_hip.h")).read()
    assert re.search(r"\bint ukm_setop2_multi\s*\(", hdr)
    for seam in ("union.go:186-208", "inter.go:205-278", "diff.go:379-454"):
        assert seam in hdr[hdr.index("two or three 2-way operations"):hdr.index("int ukm_setop2_multi")], seam
    assert "ukm_setop2_multi" in lib.SYMBOLS
    import shutil
    import subprocess
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    for so in (build.SO, build.SO_LBTEST):
        out = subprocess.run([nm, "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
        assert any(ln.split()[-1] == "ukm_setop2_multi" for ln in out.splitlines() if ln.split()), so
    L = lib.load()
    assert L.ukm_setop2_multi.argtypes is not None and len(L.ukm_setop2_multi.argtypes) == 15


def test_binding_is_callable_and_null_arguments_are_refused():
    import ctypes as C
    from unikmer_amd import lib
    assert callable(lib.Context.setop2_multi)
    L = lib.load()
    n = (C.c_uint64 * 3)()
    assert L.ukm_setop2_multi(None, 3, None, None, 0, 0, None, None, 0, 0, 0, None, None, None, n) == lib.ERR_INVALID
