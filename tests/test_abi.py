"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/unikmer_hip.h
declares, and fails loudly (no fallback) when there is no GPU.  No compute calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from unikmer_amd import build, lib as L
    build.build()
    return L


def test_header_symbols_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "unikmer_hip.h")).read()
    declared = set(re.findall(r"\b(ukm_[a-z0-9_]+)\s*\(", hdr)) - {"ukm_ctx"}
    assert declared == set(lib.SYMBOLS), declared ^ set(lib.SYMBOLS)
    L = lib.load()
    for name in declared:
        assert hasattr(L, name), name


def _exported_ukm(path):
    """the ukm_* symbols a shared library defines and exports, read without loading it"""
    import shutil
    import subprocess
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("ukm_")}


def test_seam_library_exports_the_same_symbols(lib):
    """build() also leaves the look-back test library (tests/test_gpu_lb_retry.py): the same sources, six of them compiled
    with UKM_LB_TEST_TIMEOUT -- the same C ABI, symbol for symbol"""
    from unikmer_amd import build
    assert os.path.exists(build.SO_LBTEST)
    product, seam = _exported_ukm(build.SO), _exported_ukm(build.SO_LBTEST)
    assert set(lib.SYMBOLS) <= product, set(lib.SYMBOLS) - product
    assert seam == product, seam ^ product


def test_pure_host_entry_points(lib):
    L = lib.load()
    assert L.ukm_version() >= 1
    assert L.ukm_max_hash(1000) == 18446744073709552          # count.go:98
    assert L.ukm_max_hash(15) == 1229782938247303424
    assert L.ukm_common_threshold(10, 0.75, 0) == 7            # common.go:93-105 (truncation)
    assert L.ukm_common_threshold(10, 1.0, 3) == 3


def test_shard_plan_capacity_is_decided_collectively(lib):
    """ukm_shard_plan (the capacity decision inside ukm_shard_exchange): every rank evaluates the same predicate over
    ALL ranks, so a rank whose buffer is too small makes EVERY rank return UKM_ERR_CAPACITY before anything is
    posted -- a local failure on one rank would leave its peers blocked in their grouped Send/Recv (round-2 advice).
    Skewed counts: rank 1 holds nothing but owns the dense prefix range."""
    W = 2
    big = 1_000_000
    # [source][dest 0, dest 1 | capacity of source]: rank 0 sends 10 to itself and 1e6 to rank 1; rank 1 sends nothing
    ok = np.array([[10, big, 10], [0, 0, big]], dtype=np.uint64)
    for me, want in ((0, [10, 0]), (1, [big, 0])):
        rc, n = lib.Context.shard_plan(W, me, ok)
        assert rc.tolist() == want and n == sum(want)
    # rank 1 sized its buffer n_local x W = 0 -> max(1, 0) = 1: BOTH ranks must fail, and rank 1 learns what it needs
    short = ok.copy()
    short[1, W] = 1
    for me in (0, 1):
        with pytest.raises(lib.CapacityError) as e:
            lib.Context.shard_plan(W, me, short)
        assert "rank 1" in str(e.value)
    L = lib.load()
    rcv = np.zeros(W, dtype=np.uint64)
    n = C.c_uint64()
    assert L.ukm_shard_plan(W, 1, short.ctypes.data, rcv.ctypes.data, C.byref(n)) == lib.ERR_CAPACITY
    assert n.value == big and rcv.tolist() == [big, 0]
    assert L.ukm_shard_plan(0, 0, short.ctypes.data, rcv.ctypes.data, C.byref(n)) == lib.ERR_INVALID
    # 8 ranks, uniform: everybody receives W x 5
    W = 8
    g = np.full((W, W + 1), 5, dtype=np.uint64)
    g[:, W] = 40
    for me in range(W):
        rc, n = lib.Context.shard_plan(W, me, g)
        assert n == 40 and rc.tolist() == [5] * W
    g[3, W] = 39
    for me in range(W):
        with pytest.raises(lib.CapacityError):
            lib.Context.shard_plan(W, me, g)


def test_shard_collectives_agree_on_taxids_and_on_a_failed_rank(lib):
    """The decisions that only N > 1 can exercise, as the pure host functions every rank evaluates over the SAME gathered
    words (round-5 review / advice):
      * ukm_shard_plan: bit 63 of a rank's capacity word says "I passed taxids"; ranks that disagree ALL return
        UKM_ERR_INVALID before anything is posted (a mixed call would leave taxid transfers unmatched inside the group);
      * ukm_shard_counts_plan (ukm_shard_counts_tax's gather): the same per file for the two-step exchange;
      * ukm_shard_splitters_plan: a rank whose preparation failed sends UKM_SHARD_RANK_FAILED as its record count and EVERY
        rank returns UKM_ERR_PEER -- no host goes on to the next collective with a rank missing."""
    L = lib.load()
    HAS = 1 << 63
    W = 2
    g = np.array([[3, 4, 10 | HAS], [5, 6, 20 | HAS]], dtype=np.uint64)
    for me, want in ((0, [3, 5]), (1, [4, 6])):
        rc, n = lib.Context.shard_plan(W, me, g)                 # all with taxids: the bit is not part of the capacity
        assert rc.tolist() == want and n == sum(want)
    mixed = g.copy()
    mixed[1, W] = 20
    rcv = np.zeros(W, dtype=np.uint64)
    n = C.c_uint64()
    for me in range(W):
        assert L.ukm_shard_plan(W, me, mixed.ctypes.data, rcv.ctypes.data, C.byref(n)) == lib.ERR_INVALID
        assert b"taxids" in L.ukm_last_error()
    short = g.copy()
    short[0, W] = 7 | HAS                                        # 8 records arrive at rank 0
    for me in range(W):
        assert L.ukm_shard_plan(W, me, short.ctypes.data, rcv.ctypes.data, C.byref(n)) == lib.ERR_CAPACITY
    # two-step exchange: [rank][nfiles * W sizes | nfiles flags]
    nfiles = 3
    rows = np.zeros((W, nfiles * (W + 1)), dtype=np.uint64)
    rows[0, :nfiles * W] = [1, 2, 3, 4, 5, 6]
    rows[1, :nfiles * W] = [7, 8, 9, 10, 11, 12]
    rows[0, nfiles * W:] = [1, 0, 2]                             # file 2: rank 0 did not say
    rows[1, nfiles * W:] = [1, 0, 1]
    assert lib.Context.shard_counts_plan(W, 0, rows).tolist() == [[1, 7], [3, 9], [5, 11]]
    assert lib.Context.shard_counts_plan(W, 1, rows).tolist() == [[2, 8], [4, 10], [6, 12]]
    rows[1, nfiles * W + 1] = 1                                  # file 1: without taxids on rank 0, with on rank 1
    for me in range(W):
        with pytest.raises(lib.UkmError) as e:
            lib.Context.shard_counts_plan(W, me, rows)
        assert e.value.code == lib.ERR_INVALID and "file 1" in str(e.value)
    # splitters: rank 2 of 3 failed
    M = 8
    allw = np.zeros((3, M + 1), dtype=np.uint64)
    allw[0, 0], allw[0, 1:] = 80, np.arange(10, 90, 10)
    allw[1, 0], allw[1, 1:] = 80, np.arange(15, 95, 10)
    assert len(lib.Context.shard_splitters_plan(3, allw, 62)) == 4
    allw[2, 0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    with pytest.raises(lib.UkmError) as e:
        lib.Context.shard_splitters_plan(3, allw, 62)
    assert e.value.code == lib.ERR_PEER and "rank 2" in str(e.value)


def test_no_gpu_fails_loudly(lib):
    L = lib.load()
    n = C.c_int(-1)
    assert L.ukm_device_count(C.byref(n)) == 0
    if n.value > 0:
        pytest.skip("a GPU is visible")
    h = C.c_void_p()
    rc = L.ukm_ctx_create(0, C.byref(h))
    assert rc == lib.ERR_HIP and not h.value
    assert b"no HIP device" in L.ukm_last_error()
    with pytest.raises(RuntimeError):
        lib.Context()


def test_null_arguments_return_error_codes(lib):
    L = lib.load()
    n = C.c_uint64()
    assert L.ukm_setop2(None, 0, None, None, 0, None, None, 0, 0, None, None, 0, C.byref(n)) == lib.ERR_INVALID
    assert L.ukm_sort_u64(None, None, 0, 64) == lib.ERR_INVALID
    assert L.ukm_ctx_destroy(None) == 0


def test_header_is_plain_c_and_links(lib, tmp_path):
    """include/unikmer_hip.h must be usable from C (cgo compiles it as C): the example client builds
    with gcc -std=c99 -Wall -Werror and links against the shared library without any HIP header."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "count_union")
    libdir = os.path.join(ROOT, "unikmer_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "count_union.c"), "-L", libdir, "-lunikmer_hip", "-Wl,-rpath," + libdir,
           "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    # exit code 2 = "no HIP device" (this container); 0 = ran on a GPU and inclusion-exclusion held
    assert r.returncode in (0, 2), (r.returncode, r.stdout, r.stderr)
