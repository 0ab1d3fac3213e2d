"""ukm_pair_counts without a GPU: the plain arithmetic of unikmer_amd/csrc/ukm_pairs.h (block plan, row stride, tile maps,
K split, grid checks, and a host restatement of the device passes) as a stand-alone program under the address and
undefined-behaviour sanitizers (tests/pairs_units.cpp); the symbol in the header, the binding and both libraries; the pure
functions of unikmer_amd/similarity.py against hand-computed matrices."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from unikmer_amd import build, lib as L
    build.build()
    return L


def test_pair_arithmetic_under_sanitizers(tmp_path):
    """no Python-loaded code runs under a sanitizer: the header is plain C++ and gets a main() of its own"""
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the driver; it must be here"
    exe = str(tmp_path / "pairs_units")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
           "-I", os.path.join(ROOT, "unikmer_amd", "csrc"), os.path.join(ROOT, "tests", "pairs_units.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.returncode, r.stdout, r.stderr)


def test_symbol_in_header_binding_and_both_libraries(lib):
    from unikmer_amd import build
    hdr = open(os.path.join(ROOT, "include", "unikmer_hip.h")).read()
    assert re.search(r"\bint\s+ukm_pair_counts\s*\(", hdr)
    assert "ukm_pair_counts" in lib.SYMBOLS and hasattr(lib.load(), "ukm_pair_counts")
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    for so in (build.SO, build.SO_LBTEST):
        out = subprocess.run([nm, "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
        assert any(ln.split()[-1] == "ukm_pair_counts" for ln in out.splitlines() if ln.split()), so
    assert "ukm_pairs.hip" in build.SOURCES and "ukm_pairs.h" in build.HEADERS


def test_call_fails_with_an_error_code(lib):
    """like every entry point: no context, no result -- and the argument limits are checked before anything touches a device"""
    L = lib.load()
    assert L.ukm_pair_counts(None, None, None, 1, 1, 0, None, None) == lib.ERR_INVALID
    assert b"ctx is NULL" in L.ukm_last_error()
    n = C.c_int(-1)
    assert L.ukm_device_count(C.byref(n)) == 0
    if n.value == 0:
        with pytest.raises(RuntimeError):
            lib.Context().pair_counts([np.arange(3, dtype=np.uint64)])


def test_jaccard_containment_mash_by_hand():
    from unikmer_amd import similarity as S
    # A = {1,2,3,4}, B = {3,4,5}, C = {} , D = {}
    counts = np.array([[4, 2, 0, 0], [2, 3, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], dtype=np.uint64)
    sizes = np.array([4, 3, 0, 0], dtype=np.uint64)
    j = S.jaccard(counts, sizes)
    want = np.array([[1, 2 / 5, 0, 0], [2 / 5, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    assert np.array_equal(j, want), j                                   # 0/0: 1.0 on the diagonal, 0.0 elsewhere
    c = S.containment(counts, sizes)
    assert np.array_equal(c, np.array([[1, 2 / 4, 0, 0], [2 / 3, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])), c
    # rectangular: the first two sets as queries
    assert np.array_equal(S.jaccard(counts[:2], sizes), want[:2])
    assert np.array_equal(S.containment(counts[:1], sizes), np.array([[1, 0.5, 0, 0]]))
    d = S.mash_distance(j, 21)
    assert d[0, 0] == 0.0 and d[2, 3] == 1.0 and d[0, 2] == 1.0
    assert d[0, 1] == pytest.approx(-np.log(2 * 0.4 / 1.4) / 21, rel=1e-15)
    assert S.mash_distance(0.0, 31) == 1.0 and S.mash_distance(1.0, 31) == 0.0
    assert S.mash_distance(0.5, 31) == pytest.approx(-np.log(2 / 3) / 31, rel=1e-15)
    assert S.mash_distance(1e-30, 1) == 1.0                             # clipped, as Mash does
    assert np.array_equal(S.matrix("count", counts, sizes, 21), counts)
    assert np.array_equal(S.matrix("mash", counts, sizes, 21), d)
    with pytest.raises(ValueError):
        S.jaccard(counts, sizes[:3])
    # counts near 2^63 keep their value up to float64's rounding
    big = np.array([[2 ** 62]], dtype=np.uint64)
    assert S.jaccard(big, big[0])[0, 0] == 1.0


def test_tsv_and_header_check():
    from unikmer_amd import similarity as S, unikfile as U
    t = S.format_tsv(["a.unik", "b.unik"], ["a.unik"], np.array([[3, 1]], dtype=np.uint64))
    assert t == "\ta.unik\tb.unik\na.unik\t3\t1\n"
    assert S.format_tsv(["a", "b"], ["a"], np.array([[1.0, 0.25]])) == "\ta\tb\na\t1\t0.25\n"
    h = {"k": 21, "flag": U.CANONICAL | U.SORTED, "scale": 1}
    S.check_compatible(["x", "y"], [h, dict(h, flag=U.CANONICAL)])            # sorted or not: the same codes
    S.check_compatible(["x", "y"], [h, dict(h, scale=7)])                     # a scale without the scaled flag says nothing
    for other, word in ((dict(h, k=23), "k"), (dict(h, flag=U.SORTED), "flags"), (dict(h, flag=h["flag"] | U.HASHED), "flags")):
        with pytest.raises(ValueError) as e:
            S.check_compatible(["x.unik", "y.unik"], [h, other])
        assert "x.unik" in str(e.value) and "y.unik" in str(e.value) and word in str(e.value)
    hs = dict(h, flag=h["flag"] | U.SCALED | U.HASHED, scale=100)
    with pytest.raises(ValueError) as e:
        S.check_compatible(["x.unik", "y.unik", "z.unik"], [hs, hs, dict(hs, scale=200)])
    assert "x.unik" in str(e.value) and "z.unik" in str(e.value) and "scale" in str(e.value)
