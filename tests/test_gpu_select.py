"""ukm_grep / ukm_filter / ukm_sample and the `grep` / `filter` / `sample` commands on the GPU.

The expected values come from a model in this file -- the plain loops of filterCode (filter.go:181-221, the loops over the
bases and over the window positions kept as they are, every record a row of a numpy array), the grep predicate with Python
sets, and range(start - 1, n, window) -- never from the library under test.  Inputs: the oracle's kmer_iter / hash_iter over
the golden genomes, and splitmix64.  Every comparison is bit-exact on every record.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import AMUC, GOLDEN, IAI39, MG1655, splitmix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")
TILE = 2048  # records per tile of the selection kernel (ukm_select.hip)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from unikmer_amd import lib
    from oracle import oracle
    ctx = lib.Context(0)
    yield lib, ctx, oracle
    ctx.close()


# ---- the models ----------------------------------------------------------------------------------------------------------
def model_filter(codes, k, threshold=15, window=7, penalty_s=3, penalty_d=1, test_last_window=False):
    """filterCode (filter.go:181-221) for every code: True = hit (low complexity).  test_last_window: what the loop would
    give if it also tested position k - window (it does not: iLast = k - window - 1)."""
    codes = np.ascontiguousarray(codes, dtype=np.uint64)
    hits = np.zeros(len(codes), dtype=bool)
    if window > k:
        window = k
    step = 1 << 18
    for a in range(0, len(codes), step):
        code = codes[a:a + step].copy()
        scores = np.zeros((len(code), k), dtype=np.int64)
        last = np.full(len(code), 356, dtype=np.uint64)
        for i in range(k):
            c = code & np.uint64(3)
            if i > 0:
                scores[:, i] = np.where(c == last, penalty_s, penalty_d)
            else:
                scores[:, i] = penalty_d
            last = c
            code = code >> np.uint64(2)   # (Go: bases above bit 63 read as 0)
        i_last = k - window - 1
        if i_last < 0:
            i_last = 0
        if test_last_window:
            i_last = k - window
        hit = np.zeros(len(code), dtype=bool)
        s = np.zeros(len(code), dtype=np.int64)
        pre = np.zeros(len(code), dtype=np.int64)
        for i in range(i_last + 1):
            if i == 0:
                for j in range(window):
                    s = s + scores[:, j]
            else:
                s = s - pre + scores[:, i + window - 1]
            pre = scores[:, i]
            hit |= s >= threshold
        hits[a:a + step] = hit
    return hits


def model_grep_mask(values, queries):
    qs = set(np.asarray(queries).tolist())
    return np.fromiter((v in qs for v in np.asarray(values).tolist()), dtype=bool, count=len(values))


def model_canonical(codes, k):
    """kmers.Canonical: min(code, reverse complement)"""
    codes = np.ascontiguousarray(codes, dtype=np.uint64)
    c = ~codes
    rc = np.zeros(len(codes), dtype=np.uint64)
    for _ in range(k):
        rc = (rc << np.uint64(2)) | (c & np.uint64(3))
        c = c >> np.uint64(2)
    return np.minimum(codes, rc)


def _dev(x, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype).view({np.uint64: np.int64, np.uint32: np.int32}[dtype])).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype) if hasattr(t, "cpu") else np.asarray(t)


def distinct_kmers(O, genomes, name, k):
    bases, off = genomes(name)
    return np.unique(O.count_windows(bases, off, k))


@pytest.fixture(scope="module")
def mg31(env, genomes):
    return distinct_kmers(env[2], genomes, MG1655, 31)


def rand_codes(n, seed, k=31):
    v = splitmix64(np.arange(n, dtype=np.uint64) + np.uint64(seed << 32))
    return v >> np.uint64(64 - 2 * k) if k < 32 else v


# ---- filter ----------------------------------------------------------------------------------------------------------------
FILTER_TABLE = [  # genome, k, distinct canonical k-mers, hits at the defaults
    (MG1655, 31, 4_554_269, 2_148_606), (MG1655, 21, 4_543_891, 1_464_980), (MG1655, 7, 8_192, 308), (MG1655, 5, 512, 0),
    (AMUC, 31, 2_632_727, 1_687_008),
]


@pytest.mark.parametrize("name,k,distinct,hits", FILTER_TABLE)
def test_filter_genomes_defaults(env, genomes, name, k, distinct, hits):
    lib, ctx, O = env
    codes = distinct_kmers(O, genomes, name, k)
    assert len(codes) == distinct
    hit = model_filter(codes, k)
    print("%s k=%d: %d distinct, model hits %d" % (name, k, len(codes), int(hit.sum())))
    assert int(hit.sum()) == hits
    got = ctx.filter(codes, k)
    assert np.array_equal(got, codes[~hit])
    got = ctx.filter(codes, k, invert=True)
    assert np.array_equal(got, codes[hit])


def test_filter_quirk_is_pinned(env, mg31):
    """the last window position is never tested: 57,930 records of MG1655 would be hits if it were"""
    lib, ctx, O = env
    hit = model_filter(mg31, 31)
    hit_last = model_filter(mg31, 31, test_last_window=True)
    assert int(hit.sum()) == 2_148_606 and int(hit_last.sum()) == 2_206_536
    got = ctx.filter(mg31, 31, invert=True)
    assert len(got) == 2_148_606 and np.array_equal(got, mg31[hit])


def test_filter_t12_w5(env, mg31):
    lib, ctx, O = env
    hit = model_filter(mg31, 31, threshold=12, window=5)
    assert int(hit.sum()) == 996_823
    assert np.array_equal(ctx.filter(mg31, 31, threshold=12, window=5), mg31[~hit])


def test_filter_taxids_and_device(env, mg31):
    lib, ctx, O = env
    codes = mg31[:1_000_003][np.argsort(splitmix64(np.arange(1_000_003, dtype=np.uint64)))]  # unsorted
    tax = (splitmix64(codes) % np.uint64(100_000)).astype(np.uint32)
    hit = model_filter(codes, 31)
    gk, gt = ctx.filter(codes, 31, taxids=tax)
    assert np.array_equal(gk, codes[~hit]) and np.array_equal(gt, tax[~hit])
    dk, dt = ctx.filter(_dev(codes, np.uint64), 31, taxids=_dev(tax, np.uint32), invert=True)
    assert np.array_equal(_host(dk, np.uint64), codes[hit]) and np.array_equal(_host(dt, np.uint32), tax[hit])


def test_filter_hashed_k40(env, genomes):
    """a hashed file: 64-bit values, k = 40.  Bases 32 .. 39 read as 0, a run of eight equal bases: at the defaults EVERY record
    is a hit (as in the reference, which does not look at the hashed flag); -t 21 asks for base 31 to be 0 as well"""
    lib, ctx, O = env
    bases, off = genomes(AMUC)
    h = O.hash_iter(bases[: 400_000], 40, True, False)
    hit = model_filter(h, 40)
    assert hit.all()
    assert len(ctx.filter(h, 40)) == 0
    assert np.array_equal(ctx.filter(h, 40, invert=True), h)
    hit = model_filter(h, 40, threshold=21)
    assert 0 < int(hit.sum()) < len(h)
    assert np.array_equal(ctx.filter(h, 40, threshold=21), h[~hit])
    assert np.array_equal(ctx.filter(h, 40, threshold=21, invert=True), h[hit])


@pytest.mark.parametrize("k,t,w,s,d", [
    (31, 15, 7, 3, 1), (31, 0, 7, 3, 1), (31, 47, 40, 3, 1), (31, 45, 31, 3, 1), (31, 44, 30, 3, 1), (32, 15, 7, 3, 1), (1, 1, 1, 3, 1),
    (1, 2, 1, 3, 1), (31, 17, 7, 1, 3), (31, 9, 7, -1, 2), (31, 5, 7, -3, 2), (31, 7, 7, 1, 1), (31, 8, 7, 1, 1), (31, 0, 6, -3, -1),
    (33, 20, 9, 3, 1), (40, 21, 7, 3, 1), (64, 21, 7, 3, 1), (64, 22, 7, 3, 1), (47, 18, 5, 2, 4), (2, 4, 2, 3, 1), (3, 4, 2, 3, 1),
    (9, 16, 8, 3, 1),
])
def test_filter_parameters(env, k, t, w, s, d):
    """window above k, window = k and k - 1, penalty_s below penalty_d, negative penalties, equal penalties, k up to 64"""
    lib, ctx, O = env
    n = 200_001
    codes = rand_codes(n, 7 + k, k=min(k, 32))
    # low-complexity records among them: runs of one base
    codes[::5] &= np.uint64(0xFFFF)
    codes[1::7] |= np.uint64(0xFFFFFFFF) << np.uint64(max(2 * min(k, 32) - 32, 0)) if k >= 16 else np.uint64(0)
    if k > 32:
        codes = splitmix64(codes)
        codes[::3] >>= np.uint64(20)
    hit = model_filter(codes, k, threshold=t, window=w, penalty_s=s, penalty_d=d)
    print("k=%d t=%d w=%d s=%d d=%d: %d of %d hits" % (k, t, w, s, d, int(hit.sum()), n))
    assert np.array_equal(ctx.filter(codes, k, threshold=t, window=w, penalty_s=s, penalty_d=d), codes[~hit])
    assert np.array_equal(ctx.filter(codes, k, threshold=t, window=w, penalty_s=s, penalty_d=d, invert=True), codes[hit])


def test_filter_bad_arguments(env):
    lib, ctx, O = env
    codes = rand_codes(10, 1)
    for kw in (dict(k=0), dict(k=65), dict(k=31, window=0), dict(k=31, threshold=-1)):
        with pytest.raises(lib.UkmError) as e:
            ctx.filter(codes, **kw)
        assert e.value.code == (lib.ERR_K if kw["k"] in (0, 65) else lib.ERR_INVALID)


# ---- grep ------------------------------------------------------------------------------------------------------------------
def grep_case(n, nq, seed, dup_queries=False):
    """unsorted records with duplicates, about half of them drawn from the queries"""
    q = rand_codes(max(nq, 1), seed)[:nq]
    if dup_queries and nq:
        q = np.concatenate([q, q[:: 3], q[:7]])
    pool = rand_codes(n, seed + 1)
    pick = splitmix64(np.arange(n, dtype=np.uint64) + np.uint64(seed + 2))
    rec = pool.copy()
    if nq:
        from_q = (pick & np.uint64(1)) == 0
        rec[from_q] = q[(pick[from_q] >> np.uint64(1)) % np.uint64(len(q))]
    rec[n // 2:] = rec[: n - n // 2]  # every record of the first half once more
    return rec, q


def expect_route(lib_choice, nq):
    return 1 if (lib_choice != 0 and nq <= 2048) else 2


@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("nq", [0, 1, 1500, 1_000_000])
def test_grep_routes(env, route, nq):
    lib, ctx, O = env
    n = 300_001
    rec, q = grep_case(n, nq, 11 + nq % 97, dup_queries=nq > 1)
    tax = (splitmix64(np.arange(n, dtype=np.uint64)) % np.uint64(1 << 20)).astype(np.uint32)
    mask = model_grep_mask(rec, q)
    if nq:
        assert 0 < int(mask.sum()) < n
    ctx.set_option("grep_lds", route)
    try:
        for invert in (False, True):
            keep = ~mask if invert else mask
            got = ctx.grep(rec, q, invert=invert)
            assert np.array_equal(got, rec[keep])
            if nq:
                assert ctx.stat("grep_route") == expect_route(route, len(q))
            gk, gt = ctx.grep(rec, q, taxids=tax, invert=invert)
            assert np.array_equal(gk, rec[keep]) and np.array_equal(gt, tax[keep])   # pairwise: each record its own taxid
            dk, dt = ctx.grep(_dev(rec, np.uint64), _dev(q, np.uint64) if nq else q, taxids=_dev(tax, np.uint32), invert=invert)
            assert np.array_equal(_host(dk, np.uint64), rec[keep]) and np.array_equal(_host(dt, np.uint32), tax[keep])
    finally:
        ctx.set_option("grep_lds", None)


def test_grep_default_route(env):
    lib, ctx, O = env
    rec, q = grep_case(50_000, 100, 5)
    ctx.grep(rec, q)
    assert ctx.stat("grep_route") == 1
    rec, q = grep_case(50_000, 5000, 6)
    ctx.grep(rec, q)
    assert ctx.stat("grep_route") == 2


@pytest.mark.parametrize("route", [0, 1])
def test_grep_special_values(env, route):
    """codes 0 and 2^64 - 1 (the LDS table's empty mark) as records and as queries"""
    lib, ctx, O = env
    rec = np.array([0, 5, 2 ** 64 - 1, 7, 0, 2 ** 64 - 1, 9, 2 ** 63], dtype=np.uint64)
    ctx.set_option("grep_lds", route)
    try:
        for q in ([0], [2 ** 64 - 1], [0, 2 ** 64 - 1, 9], [1], [2 ** 63, 5]):
            q = np.array(q, dtype=np.uint64)
            mask = model_grep_mask(rec, q)
            assert np.array_equal(ctx.grep(rec, q), rec[mask])
            assert np.array_equal(ctx.grep(rec, q, invert=True), rec[~mask])
    finally:
        ctx.set_option("grep_lds", None)


@pytest.mark.parametrize("route", [0, 1])
def test_grep_canonical_k(env, genomes, route):
    lib, ctx, O = env
    bases, off = genomes(AMUC)
    raw = O.kmer_iter(bases[:300_000], 31, False, False)      # not canonical
    can = model_canonical(raw, 31)
    assert np.array_equal(can, O.kmer_iter(bases[:300_000], 31, True, False)) and not np.array_equal(can, raw)
    q = can[::211][:1800]
    mask = model_grep_mask(can, q)
    ctx.set_option("grep_lds", route)
    try:
        assert np.array_equal(ctx.grep(raw, q, canonical_k=31), can[mask])           # the canonical codes are written
        assert np.array_equal(ctx.grep(raw, q, canonical_k=31, invert=True), can[~mask])
        assert np.array_equal(ctx.grep(raw, np.empty(0, np.uint64), canonical_k=31, invert=True), can)
    finally:
        ctx.set_option("grep_lds", None)


def test_grep_by_taxid(env):
    lib, ctx, O = env
    n = 400_003
    rec = rand_codes(n, 21)
    tax = (splitmix64(np.arange(n, dtype=np.uint64) + np.uint64(99)) % np.uint64(3000)).astype(np.uint32)
    tax[::1000] = 4_000_000_000
    for qt in ([7], [7, 7, 2999, 0, 12], list(range(0, 3000, 3)), [4_000_000_000], [5000]):
        qt = np.array(qt, dtype=np.uint32)
        mask = model_grep_mask(tax, qt)
        for invert in (False, True):
            keep = ~mask if invert else mask
            gk, gt = ctx.grep(rec, query_taxids=qt, taxids=tax, invert=invert)
            assert np.array_equal(gk, rec[keep]) and np.array_equal(gt, tax[keep])
        dk, dt = ctx.grep(_dev(rec, np.uint64), query_taxids=_dev(qt, np.uint32), taxids=_dev(tax, np.uint32))
        assert np.array_equal(_host(dk, np.uint64), rec[mask]) and np.array_equal(_host(dt, np.uint32), tax[mask])
    # one taxid for the whole file: all or nothing
    qt = np.array([3, 562, 9], dtype=np.uint32)
    assert np.array_equal(ctx.grep(rec, query_taxids=qt, taxids=562), rec)
    assert len(ctx.grep(rec, query_taxids=qt, taxids=561)) == 0
    assert len(ctx.grep(rec, query_taxids=qt, taxids=562, invert=True)) == 0
    assert np.array_equal(ctx.grep(rec, query_taxids=qt, taxids=561, invert=True), rec)
    assert np.array_equal(ctx.grep(rec, query_taxids=np.empty(0, np.uint32), taxids=tax, invert=True)[0], rec)
    assert len(ctx.grep(rec, query_taxids=np.empty(0, np.uint32), taxids=tax)[0]) == 0


def test_grep_capacity_and_arguments(env):
    lib, ctx, O = env
    rec, q = grep_case(100_000, 1000, 31)
    need = int(model_grep_mask(rec, q).sum())
    import ctypes as C
    out = np.empty(need - 1, dtype=np.uint64)
    m = C.c_uint64()
    rc = ctx.L.ukm_grep(ctx.h, rec.ctypes.data, None, 0, len(rec), 0, q.ctypes.data, None, len(q), 0, out.ctypes.data, None, len(out), C.byref(m))
    assert rc == lib.ERR_CAPACITY and m.value == need
    out = np.empty(need, dtype=np.uint64)
    rc = ctx.L.ukm_grep(ctx.h, rec.ctypes.data, None, 0, len(rec), 0, q.ctypes.data, None, len(q), 0, out.ctypes.data, None, len(out), C.byref(m))
    assert rc == lib.OK and m.value == need
    qt = np.array([1], dtype=np.uint32)
    rc = ctx.L.ukm_grep(ctx.h, rec.ctypes.data, None, 0, len(rec), 0, q.ctypes.data, qt.ctypes.data, 1, 0, out.ctypes.data, None, len(out), C.byref(m))
    assert rc == lib.ERR_INVALID
    rc = ctx.L.ukm_grep(ctx.h, rec.ctypes.data, None, 0, len(rec), 0, None, None, 5, 0, out.ctypes.data, None, len(out), C.byref(m))
    assert rc == lib.ERR_INVALID
    rc = ctx.L.ukm_grep(ctx.h, rec.ctypes.data, None, 0, len(rec), 33, q.ctypes.data, None, len(q), 0, out.ctypes.data, None, len(out), C.byref(m))
    assert rc == lib.ERR_K
    with pytest.raises(lib.CapacityError):
        ctx.sample(rec, 1, 2, out=np.empty(10, dtype=np.uint64))


# ---- sizes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_sizes_small(env, n):
    lib, ctx, O = env
    rec, q = grep_case(n, 300, 41) if n else (np.empty(0, np.uint64), rand_codes(300, 41))
    tax = np.arange(n, dtype=np.uint32)
    mask = model_grep_mask(rec, q)
    for route in (0, 1):
        ctx.set_option("grep_lds", route)
        try:
            gk, gt = ctx.grep(rec, q, taxids=tax)
            assert np.array_equal(gk, rec[mask]) and np.array_equal(gt, tax[mask])
            assert np.array_equal(ctx.grep(rec, q, invert=True), rec[~mask])
        finally:
            ctx.set_option("grep_lds", None)
    hit = model_filter(rec, 31)
    assert np.array_equal(ctx.filter(rec, 31), rec[~hit])
    for start, window in ((1, 1), (1, 3), (2, 1), (n + 1, 1), (max(n, 1), 7), (5, 2048)):
        want = np.arange(start - 1, n, window)
        gk, gt = ctx.sample(rec, start, window, taxids=tax)
        assert np.array_equal(gk, rec[want]) and np.array_equal(gt, tax[want])
        assert np.array_equal(ctx.sample(rec, start, window), rec[want])


@pytest.mark.parametrize("force_ticket", [0, 1])
def test_sizes_many_tiles(env, force_ticket):
    """10,000,019 records: thousands of tiles, the last one partial; nothing kept, everything kept, about half kept"""
    lib, ctx, O = env
    n = 10_000_019
    rec, q = grep_case(n, 2000, 51)
    tax = (splitmix64(np.arange(n, dtype=np.uint64) + np.uint64(5)) >> np.uint64(40)).astype(np.uint32)
    mask = model_grep_mask(rec, q)
    absent = np.array([2 ** 63 + 1, 2 ** 63 + 3], dtype=np.uint64)   # (codes of 31 bases stay below 2^62)
    hit = model_filter(rec, 31)
    d_rec, d_tax = _dev(rec, np.uint64), _dev(tax, np.uint32)
    ctx.set_option("force_ticket", force_ticket)
    try:
        for route in (0, 1):
            ctx.set_option("grep_lds", route)
            dk, dt = ctx.grep(d_rec, _dev(q, np.uint64), taxids=d_tax)
            assert np.array_equal(_host(dk, np.uint64), rec[mask]) and np.array_equal(_host(dt, np.uint32), tax[mask])
            assert len(ctx.grep(d_rec, _dev(absent, np.uint64))) == 0                                    # nothing kept
            assert np.array_equal(_host(ctx.grep(d_rec, _dev(absent, np.uint64), invert=True), np.uint64), rec)  # everything
        ctx.set_option("grep_lds", None)
        dk, dt = ctx.filter(d_rec, 31, taxids=d_tax)
        assert np.array_equal(_host(dk, np.uint64), rec[~hit]) and np.array_equal(_host(dt, np.uint32), tax[~hit])
        assert np.array_equal(ctx.filter(rec, 31, invert=True), rec[hit])                                # host arrays
        assert len(ctx.filter(d_rec, 31, threshold=0)) == 0
        assert np.array_equal(_host(ctx.filter(d_rec, 31, threshold=1000), np.uint64), rec)
        qt = np.unique(tax[::3])[:100_000]
        tm = model_grep_mask(tax, qt)
        dk, dt = ctx.grep(d_rec, query_taxids=_dev(qt, np.uint32), taxids=d_tax)
        assert np.array_equal(_host(dk, np.uint64), rec[tm]) and np.array_equal(_host(dt, np.uint32), tax[tm])
        want = np.arange(6, n, 3)
        dk, dt = ctx.sample(d_rec, 7, 3, taxids=d_tax)
        assert np.array_equal(_host(dk, np.uint64), rec[want]) and np.array_equal(_host(dt, np.uint32), tax[want])
    finally:
        ctx.set_option("grep_lds", None)
        ctx.set_option("force_ticket", None)


def test_unaligned_device_views(env):
    """device arrays that start 8 / 4 bytes into a 16-byte line: the kernel's 16-byte loads must not be used"""
    lib, ctx, O = env
    n = 50_001
    rec, q = grep_case(n + 1, 500, 61)
    tax = np.arange(n + 1, dtype=np.uint32)
    mask = model_grep_mask(rec[1:], q)
    dk, dt = ctx.grep(_dev(rec, np.uint64)[1:], _dev(q, np.uint64), taxids=_dev(tax, np.uint32)[1:])
    assert np.array_equal(_host(dk, np.uint64), rec[1:][mask]) and np.array_equal(_host(dt, np.uint32), tax[1:][mask])


# ---- through the binary: cross-checks against existing commands -----------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    from unikmer_amd import build
    build.build()

    def run(*args):
        p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout.decode()
    return run


@pytest.fixture(scope="module")
def two_sets(cli, tmp_path_factory):
    d = tmp_path_factory.mktemp("select")
    a, b = str(d / "a"), str(d / "b")
    cli("count", "-k", 31, "-K", "-s", os.path.join(GOLDEN, MG1655), "-o", a)
    cli("count", "-k", 31, "-K", "-s", os.path.join(GOLDEN, IAI39), "-o", b)
    return d, a + ".unik", b + ".unik"


def view(cli, f):
    return cli("view", f).splitlines()


def test_cli_grep_matches_inter_and_diff(cli, two_sets):
    d, a, b = two_sets
    cli("inter", a, b, "-o", d / "i")
    cli("diff", a, b, "-o", d / "d")
    cli("grep", "-F", b, a, "-o", d / "gi")
    cli("grep", "-v", "-F", b, a, "-o", d / "gd")
    inter, diff = view(cli, str(d / "i.unik")), view(cli, str(d / "d.unik"))
    assert len(inter) > 1_000_000 and len(diff) > 100_000
    assert view(cli, str(d / "gi.unik")) == inter
    assert view(cli, str(d / "gd.unik")) == diff
    # -s -u over an unsorted concatenation gives the same set again
    cli("concat", str(d / "gi.unik"), str(d / "gi.unik"), "-o", d / "twice")
    cli("grep", "-F", b, str(d / "twice.unik"), "-u", "-o", d / "gu")
    assert view(cli, str(d / "gu.unik")) == inter


def test_cli_sample_filter(cli, two_sets):
    d, a, b = two_sets
    whole = view(cli, a)
    assert len(whole) == 4_554_269
    cli("sample", "-s", 1, "-w", 1, a, "-o", d / "s1")
    assert view(cli, str(d / "s1.unik")) == whole
    cli("sample", "-s", 5, "-w", 1000, a, "-o", d / "s2")
    assert view(cli, str(d / "s2.unik")) == whole[4::1000]
    cli("filter", a, "-o", d / "f")
    cli("filter", "-v", a, "-o", d / "fv")
    kept, dropped = view(cli, str(d / "f.unik")), view(cli, str(d / "fv.unik"))
    assert len(dropped) == 2_148_606 and len(kept) + len(dropped) == len(whole)
    assert sorted(kept + dropped) == sorted(whole) and set(kept).isdisjoint(dropped)


def test_cli_grep_degenerate_query(cli, two_sets):
    """-D: a degenerate query equals the union of its expansions; every -q is searched"""
    d, a, b = two_sets
    whole = view(cli, a)
    kmer = whole[123_456]
    two = "AG" if kmer[20] in "AG" else "CT"                 # R or Y, whichever stands for the k-mer's own base
    deg = kmer[:10] + "N" + kmer[11:20] + {"AG": "R", "CT": "Y"}[two] + kmer[21:]
    expansions = [kmer[:10] + x + kmer[11:20] + y + kmer[21:] for x in "ACGT" for y in two]
    cli("grep", "-D", "-q", deg, a, "-o", d / "g1")
    cli("grep", *sum((["-q", e] for e in expansions), []), a, "-o", d / "g2")
    g1, g2 = view(cli, str(d / "g1.unik")), view(cli, str(d / "g2.unik"))
    assert g1 == g2 and kmer in g1
    want = sorted(set(whole) & set(min(e, revcomp_text(e)) for e in expansions))
    assert sorted(g1) == want


def test_cli_sample_taxids_and_ignore_taxid(cli, tmp_path):
    """sample writes the taxids the reader hands out, also under -I (sample.go:114-122,136,147): -I only keeps a file with
    ONE taxid from getting the include-taxid flag"""
    kmers = ["ACGTACGTTGC", "CGTACGTTGCA", "AAAAAAAAAAA", "ACGTTGCATGC", "AACCGGTTAAC"]
    taxa = [9606, 562, 10090, 562, 7]
    text = "".join("%s\t%d\n" % kt for kt in zip(kmers, taxa))
    src = tmp_path / "taxed.txt"
    src.write_text(text)
    cli("dump", src, "-o", tmp_path / "taxed")
    taxed = str(tmp_path / "taxed.unik")
    rows = cli("view", "-t", taxed).splitlines()
    assert rows == ["%s\t%d" % kt for kt in zip(kmers, taxa)]
    for flags in ([], ["-I"]):
        cli("sample", *flags, "-s", 2, "-w", 2, taxed, "-o", tmp_path / "st")
        assert cli("view", "-t", str(tmp_path / "st.unik")).splitlines() == rows[1::2]
        cli("filter", *flags, "-t", 30, taxed, "-o", tmp_path / "ft")
        assert cli("view", "-t", str(tmp_path / "ft.unik")).splitlines() == rows
    plain = tmp_path / "plain.txt"
    plain.write_text("".join(k + "\n" for k in kmers))
    cli("dump", "-t", 562, plain, "-o", tmp_path / "glob")
    glob = str(tmp_path / "glob.unik")
    cli("sample", "-s", 1, "-w", 3, glob, "-o", tmp_path / "sg")
    assert cli("view", "-t", str(tmp_path / "sg.unik")).splitlines() == ["%s\t562" % k for k in kmers[0::3]]
    cli("sample", "-I", "-s", 1, "-w", 3, glob, "-o", tmp_path / "sgi")
    assert cli("view", str(tmp_path / "sgi.unik")).splitlines() == kmers[0::3]
    cli("sample", "-I", taxed, glob, "-o", tmp_path / "mix")             # -I: the inputs need not agree
    assert cli("view", "-t", str(tmp_path / "mix.unik")).splitlines() == rows + ["%s\t562" % k for k in kmers]


def revcomp_text(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))
