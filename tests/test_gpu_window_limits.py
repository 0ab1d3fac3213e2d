"""The window kernels of csrc/ukm_win_kernels.h and csrc/ukm_win_minimizer.h on both sides of each of their fixed-size LDS tables.

Three kernels keep a table of fixed size and hand the call to another path when an input does not fit it:
  * stripwin_kernel      SW_REC records under one tile of SW_NT x L positions   -> ENC_FLAG_OVERFLOW, window_kernel answers
  * nthash_strip_kernel  ST_CAP candidates in one tile of ST_NT x L positions   -> ENC_FLAG_OVERFLOW, window_kernel answers
  * minimizer_kernel     M_REC entries of the window-offset table under a tile  -> binary search in global memory instead
Every input here is placed exactly at such a limit.  The limits are READ FROM THE SOURCE when this module is imported (a
constant that moves takes the inputs with it; a pattern that no longer matches is an error, not a silently void test), and
every input comes with a shape proof: a test without the `gpu` mark that recomputes from the record offsets what the kernel
computes and asserts that the input lies where its GPU test says it does.  The GPU tests compare bit-exactly with the
oracle and assert, through the context's statistics "window_route" / "window_strip_declined" / "sort_fused_hist", which
kernel answered.  The minimizer kernel picks its branch per tile inside the kernel: those tests rest on their proof.
"""
import contextlib
import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


# ------------------------------------------------------------------------------------------ the limits, from the source
# (the window translation unit: the three headers with the device code and the source with the policies, as one text)
_SRC = ""
for _f in ("ukm_win_common.h", "ukm_win_kernels.h", "ukm_win_minimizer.h", "ukm_encode.hip"):
    with open(os.path.join(ROOT, "unikmer_amd", "csrc", _f)) as _fh:
        _SRC += _fh.read()


def _src_ints(pattern):
    m = re.findall(pattern, _SRC, flags=re.M)
    if len(m) != 1:
        raise RuntimeError("ukm_encode.hip and its headers: %d matches for %r: the limits this file stands on have moved" % (len(m), pattern))
    return tuple(int(x) for x in (m[0] if isinstance(m[0], tuple) else (m[0],)))


ENC_WT, = _src_ints(r"^#define ENC_WT (\d+)$")
MIN_MT, = _src_ints(r"^#define MIN_MT (\d+)\b")
M_REC, = _src_ints(r"^constexpr int M_REC = (\d+);")
MW_MAX, = _src_ints(r"^constexpr int MW_MAX = (\d+);")
SW_NT, = _src_ints(r"^constexpr int SW_NT = (\d+);")
SW_REC, = _src_ints(r"^constexpr int SW_REC = (\d+);")
ST_NT, = _src_ints(r"^constexpr int ST_NT = (\d+);")
ST_CAP, = _src_ints(r"^#define ST_CAP_N (\d+)$")
if len(re.findall(r"^constexpr int ST_CAP = ST_CAP_N;", _SRC, flags=re.M)) != 1:   # (the list has ST_CAP_N entries)
    raise RuntimeError("ukm_win_kernels.h: ST_CAP is no longer ST_CAP_N")
SW_L_K32, SW_L_K64 = _src_ints(r"int L = \(k <= 32\) \? (\d+) : (\d+);")  # stripwin_kernel's default strip lengths
ST_L_MAX, = _src_ints(r"L = std::min\((\d+), std::max\(64, atoi\(le\) / 64 \* 64\)\);")  # largest strip_l of the filter

ROUTE_WINDOW, ROUTE_STRIPWIN, ROUTE_NTSTRIP = 1, 2, 3


@pytest.fixture(scope="module")
def ctx():
    from unikmer_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def L():
    from unikmer_amd import lib
    return lib


@contextlib.contextmanager
def _opts(ctx, **kw):
    """options of the context for the calls inside the block (an option beats the environment)"""
    for key, v in kw.items():
        ctx.set_option(key, v)
    try:
        yield
    finally:
        for key in kw:
            ctx.set_option(key, None)


def _random_bases(n, seed, ragged_alphabet=False):
    rng = np.random.default_rng(seed)
    b = ACGT[rng.integers(0, 4, n)].copy()
    if ragged_alphabet:   # degenerate (IUPAC) and lower-case bases: legal for codes, zero seed / same seed for ntHash
        other = np.frombuffer(b"acgtunNRYKMSWBDHVU", dtype=np.uint8)
        at = rng.choice(n, n // 50, replace=False)
        b[at] = other[rng.integers(0, len(other), len(at))]
    return b


def _cuts(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.uint64)


def _long_records(a, b, size=3001):
    """record lengths that cover [a, b) with records of `size` bases and one last, longer one"""
    out = []
    while b - a > 2 * size:
        out.append(size)
        a += size
    if b > a:
        out.append(b - a)
    return out


def _records_per_tile(cuts, tile_pos):
    """nr of every tile, as stripwin_kernel computes it from tile_first_rec_kernel's table:
    tile_rec[t] = upper_bound(rec_off, min(t * tile_pos, total - 1)) - 1,  nr = tile_rec[t + 1] - tile_rec[t] + 1"""
    c = np.asarray(cuts).astype(np.int64)
    total = int(c[-1])
    ntiles = -(-total // tile_pos)
    pos = np.minimum(np.arange(ntiles + 1, dtype=np.int64) * tile_pos, total - 1)
    rec = np.searchsorted(c, pos, side="right") - 1
    return rec[1:] - rec[:-1] + 1


# ============================================================ 1. stripwin_kernel: SW_REC records under one tile
SW_L = 64                       # pinned with option win_strip_l
SW_TILE = SW_NT * SW_L
SW_TILES = 4
SW_WHERE = {"first": 0, "middle": SW_TILES // 2, "last": SW_TILES - 1}
SW_CODE_KS, SW_HASH_KS = (9, 16, 17, 31, 32), (31, 33, 64)
SW_NRS = (SW_REC - 1, SW_REC, SW_REC + 1)


@functools.lru_cache(maxsize=None)
def _sw_input(k, nr, where):
    """SW_TILES tiles of long records, but tile `where` touches exactly nr records: nr - 1 short ones from its first
    position on (records of exactly k bases, empty ones, ones shorter than k, a few longer ones) and one that runs on into
    the next tile (to the end of the array in the last tile).  Inputs for different nr differ in that tile only."""
    d = SW_WHERE[where]
    total = SW_TILES * SW_TILE - 37
    pat = [k, 0, k - 1, k + 1, 1, 2 * k, 0, k, k + 16, 3]   # (the first one is not empty: it holds the tile's first position)
    small = [pat[i % len(pat)] for i in range(nr - 1)]
    a = d * SW_TILE + sum(small)
    assert a < (d + 1) * SW_TILE - 64
    end = min((d + 1) * SW_TILE + 1000, total)
    lens = _long_records(0, d * SW_TILE) + small + [end - a] + _long_records(end, total)
    cuts = _cuts(lens)
    assert int(cuts[-1]) == total
    return _random_bases(total, 1000 + k, ragged_alphabet=True), cuts


@pytest.mark.parametrize("where", list(SW_WHERE))
def test_stripwin_record_table_shapes(where):
    """no GPU: tile `where` touches SW_REC - 1, SW_REC and SW_REC + 1 records, every other tile the same few in all three
    inputs; the dense tile holds empty records, records shorter than k and records of exactly k bases"""
    d = SW_WHERE[where]
    for k in sorted(set(SW_CODE_KS + SW_HASH_KS)):
        per = [_records_per_tile(_sw_input(k, nr, where)[1], SW_TILE) for nr in SW_NRS]
        assert all(len(p) == SW_TILES for p in per)
        for nr, p in zip(SW_NRS, per):
            assert p[d] == nr, (k, nr, p)
            rest = np.delete(p, d)
            assert np.array_equal(rest, np.delete(per[0], d)) and rest.max() < SW_REC // 4, (k, nr, p)
        c = _sw_input(k, SW_REC + 1, where)[1].astype(np.int64)
        lens = np.diff(c)
        inside = (c[:-1] >= d * SW_TILE) & (c[:-1] < (d + 1) * SW_TILE)
        assert {0, k - 1, k} <= set(lens[inside].tolist())
        assert c[np.argmax(inside)] == d * SW_TILE and lens[np.argmax(inside)] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("where", list(SW_WHERE))
def test_stripwin_record_table(ctx, O, where):
    """SW_REC - 1 and SW_REC records under one tile: stripwin_kernel answers; SW_REC + 1: it gives up and window_kernel
    rewrites the output.  Codes and ntHash, canonical and forward, the dense tile first / in the middle / last."""
    with _opts(ctx, win_strip=1, win_strip_l=SW_L):
        for hashed, ks in ((False, SW_CODE_KS), (True, SW_HASH_KS)):
            for k in ks:
                for nr in SW_NRS:
                    bases, cuts = _sw_input(k, nr, where)
                    for canonical in (True, False):
                        exp = O.count_windows(bases, cuts, k, hashed=hashed, canonical=canonical)
                        d0 = ctx.stat("window_strip_declined")
                        got = (ctx.nthash if hashed else ctx.encode_kmers)(bases, cuts, k, canonical=canonical)
                        what = (where, hashed, k, nr, canonical)
                        assert np.array_equal(got, exp), what
                        declines = nr > SW_REC
                        assert ctx.stat("window_route") == (ROUTE_WINDOW if declines else ROUTE_STRIPWIN), what
                        assert ctx.stat("window_strip_declined") == d0 + (1 if declines else 0), what


@pytest.mark.gpu
def test_stripwin_record_table_illegal_base(ctx, O, L):
    """an illegal byte is an error only inside an emitted window, whichever kernel answers: on the input whose dense tile
    makes the strip kernel give up, and on its neighbour that the strip kernel answers itself"""
    k, d = 31, SW_WHERE["middle"]
    with _opts(ctx, win_strip=1, win_strip_l=SW_L):
        for nr in (SW_REC, SW_REC + 1):
            declines = nr > SW_REC
            route = ROUTE_WINDOW if declines else ROUTE_STRIPWIN
            bases, cuts = _sw_input(k, nr, "middle")
            c = cuts.astype(np.int64)
            lens = np.diff(c)
            # ... inside a record shorter than k of the dense tile
            r = int(np.argmax((c[:-1] >= d * SW_TILE) & (lens > 0) & (lens < k)))
            assert d * SW_TILE <= c[r] < (d + 1) * SW_TILE and 0 < lens[r] < k
            bad = bases.copy()
            bad[c[r] + lens[r] // 2] = ord("*")
            d0 = ctx.stat("window_strip_declined")
            assert np.array_equal(ctx.encode_kmers(bad, cuts, k), O.count_windows(bad, cuts, k)), nr
            assert ctx.stat("window_route") == route and ctx.stat("window_strip_declined") == d0 + int(declines)
            # ... inside an emitted window of another tile
            assert lens[0] > 2 * k
            bad = bases.copy()
            bad[k + 5] = ord("*")
            d0 = ctx.stat("window_strip_declined")
            with pytest.raises(L.IllegalBaseError):
                ctx.encode_kmers(bad, cuts, k)
            assert ctx.stat("window_route") == route and ctx.stat("window_strip_declined") == d0 + int(declines)
            # (ntHash knows no illegal base: the byte has the zero seed)
            assert np.array_equal(ctx.nthash(bad, cuts, k), O.count_windows(bad, cuts, k, hashed=True)), nr
            assert ctx.stat("window_route") == route


# ============================================================ 2. ukm_count through a strip launch that gave up
COUNT_K = 31
COUNT_BASES = (1 << 23) + 200_000


@functools.lru_cache(maxsize=None)
def _count_input(dense):
    """long records, >= 2^23 windows, a stretch that occurs twice (so that -d is not empty); dense: SW_REC records of 40
    bases cut into the middle, from a tile's first position on, so that this one tile touches SW_REC + 1 records"""
    n = COUNT_BASES
    bases = _random_bases(n, 2)
    bases[5_000_000:5_040_000] = bases[1_000_000:1_040_000]
    marks = {0, 3_000_003, 6_100_000, n}
    if dense:
        tile = SW_NT * SW_L_K32
        start = (n // 2) // tile * tile
        marks |= {start + 40 * i for i in range(SW_REC + 1)}
    cuts = np.array(sorted(marks), dtype=np.uint64)
    cuts = np.insert(cuts, 2, cuts[2])   # an empty record
    return bases, cuts


def test_count_declined_strip_shapes():
    """no GPU: both inputs satisfy the strip kernel's own size rule and the fused histogram's (>= 2^23 windows, k >= 17, a
    tile of <= 65,535 positions); without the dense tile no tile is near the table's size, with it exactly one tile touches
    SW_REC + 1 records"""
    tile = SW_NT * SW_L_K32
    assert COUNT_K >= 17 and COUNT_K <= 32 and tile <= 65535
    for dense in (False, True):
        bases, cuts = _count_input(dense)
        lens = np.diff(cuts.astype(np.int64))
        nwin = int(np.maximum(lens - (COUNT_K - 1), 0).sum())
        assert (1 << 23) <= nwin < (1 << 32) and len(bases) >= (1 << 23) and len(lens) * 80 <= len(bases)
        nr = _records_per_tile(cuts, tile)
        if dense:
            assert np.count_nonzero(nr > SW_REC) == 1 and nr.max() == SW_REC + 1
            assert np.count_nonzero(lens == 40) == SW_REC
        else:
            assert nr.max() <= 3


@pytest.mark.gpu
def test_count_through_declined_strip_launch(O, L):
    """ukm_count on a context of its own (the sort's latches are sticky): the strip kernel counts the sort's first histogram
    while it writes the windows; when one tile makes it give up, the partial histogram is zeroed, window_kernel rewrites the
    windows and the sort is told that nobody counted"""
    c = L.Context(0)
    try:
        modes = (L.UNIQUE, L.REPEATED, L.SINGLETON)
        sorted_windows = {}
        for dense, ms in ((False, modes), (True, modes), (False, modes[:1])):   # (the last: the context still fuses)
            bases, cuts = _count_input(dense)
            if dense not in sorted_windows:
                sorted_windows[dense] = O.sort_u64(O.count_windows(bases, cuts, COUNT_K))
            srt = sorted_windows[dense]
            assert len(srt) >= 1 << 23
            for mode in ms:
                exp = O.unique(srt, mode=mode)
                assert len(exp) > 0
                f0, d0 = c.stat("sort_fused_hist"), c.stat("window_strip_declined")
                got = c.count(bases, cuts, COUNT_K, mode=mode)
                assert np.array_equal(got, exp), (dense, mode)
                assert c.stat("window_route") == (ROUTE_WINDOW if dense else ROUTE_STRIPWIN), (dense, mode)
                assert c.stat("window_strip_declined") == d0 + int(dense), (dense, mode)
                assert c.stat("sort_fused_hist") == f0 + int(not dense), (dense, mode)
    finally:
        c.close()


# ============================================================ 3. minimizer_kernel: M_REC table entries under one tile
MIN_KW = ((5, 3), (5, 1), (5, 2), (23, 5), (64, 9))
MIN_LAYOUTS = ("fixed", "edge", "zero_runs", "mixed")


def _min_slices(cuts, k, circular):
    """(r_lo, r_hi) of every tile of MIN_MT windows, as minimizer_kernel computes them from the window offsets:
    r_lo = tile_rec[t], r_hi = min(tile_rec[t + 2] + 2, n_rec + 1); the tile's slice of the table is off[r_lo .. r_hi]"""
    lens = np.diff(np.asarray(cuts).astype(np.int64))
    nwin = np.where(lens < k, 0, lens if circular else lens - k + 1)
    off = np.concatenate([[0], np.cumsum(nwin)])
    total, n_rec = int(off[-1]), len(lens)
    ntiles = -(-total // MIN_MT)
    pos = np.minimum(np.arange(ntiles + 3, dtype=np.int64) * MIN_MT, total - 1)
    rec = np.searchsorted(off, pos, side="right") - 1
    return rec[:ntiles], np.minimum(rec[2:ntiles + 2] + 2, n_rec + 1)


def _min_entries(cuts, k, circular):
    """r_hi - r_lo of every tile: what minimizer_kernel compares with M_REC"""
    r_lo, r_hi = _min_slices(cuts, k, circular)
    return r_hi - r_lo


@functools.lru_cache(maxsize=None)
def _min_input(layout, k, w):
    """record lengths in terms of window counts (a linear record of nwin >= 1 windows has k - 1 + nwin bases)"""
    def rec(nwin):
        return k - 1 + nwin
    tiny = [rec(w - 1), rec(w), rec(w + 1)]                  # no group / one group / two groups (w = 1: no window at all)
    if layout == "fixed":
        lens = [rec(w + 1)] * 3000                           # (k, w) = (5, 3): 8 bases
    elif layout == "edge":
        lens = [tiny[i % 3] for i in range(3000)]
    elif layout == "zero_runs":
        zero = [0, k - 1, 1]
        # Records without a window have no extent in window offsets: a run of them sits AT one offset.  600 of them at the
        # offset where tile 2 starts: tile_rec skips them (the record that holds a tile's first window has windows), so
        # the slices of tiles 0 and 1 hold the whole run and the slice of tile 2 begins right behind it.  300 more behind the
        # record that holds the first window of tile 3: r_hi = tile_rec + 2 of tile 1 points INTO that run, its slice ends
        # with the run's first two records and leaves the others out.  40 at the very end.
        lens = ([rec(2 * MIN_MT)] + [zero[i % 3] for i in range(600)] + [rec(MIN_MT + MIN_MT // 2)] + [zero[i % 3] for i in range(300)]
                + [rec(3000)] + [zero[i % 3] for i in range(40)])
    else:
        # One launch with tiles on both branches.  A block of D tiny records between two long ones, the first of which
        # ends one window behind a tile's first: that tile's slice is the long record, the block and the two entries
        # behind it, D + 3 entries: exactly M_REC, then exactly M_REC + 1.  Then a dense block far beyond the table.
        def block(n):
            return [tiny[i % 3] for i in range(n)]
        def windows(ls):
            return sum(max(x - k + 1, 0) for x in ls)
        b1, b2 = block(M_REC - 3), block(M_REC - 2)
        assert windows(b2) <= 2 * MIN_MT - 1
        lens = ([rec(3 * MIN_MT + 1)] + b1 + [rec(6 * MIN_MT - windows(b1))] + b2 + [rec(5 * MIN_MT)]
                + [x for i in range(500) for x in (tiny[i % 3], k - 1, 0)] + [rec(700)])
    cuts = _cuts(lens)
    return _random_bases(int(cuts[-1]), 3000 + 7 * k + w), cuts


@pytest.mark.parametrize("k,w", MIN_KW)
def test_minimizer_record_table_shapes(k, w):
    """no GPU: read as linear records the inputs hold tiles with exactly M_REC table entries, with M_REC + 1 and with more
    than 2 * M_REC; `mixed` and `zero_runs` have tiles on both branches in one launch; a run of records without a window ends
    exactly where a tile starts; read as circular records the layouts of tiny records still leave the table"""
    e = {name: _min_entries(_min_input(name, k, w)[1], k, False) for name in MIN_LAYOUTS}
    mixed = e["mixed"]
    assert mixed[3] == M_REC, mixed
    assert np.count_nonzero(mixed == M_REC + 1) >= 1 and mixed.max() > 2 * M_REC and mixed.min() <= 3, mixed
    assert max(e["fixed"].max(), e["edge"].max()) > M_REC
    assert e["edge"].max() > 2 * M_REC or e["zero_runs"].max() > 2 * M_REC
    z = e["zero_runs"]
    assert z.max() > 2 * M_REC and z.min() <= M_REC, z
    zcuts = _min_input("zero_runs", k, w)[1]
    lens = np.diff(zcuts.astype(np.int64))
    assert lens[0] - k + 1 == 2 * MIN_MT and np.all(lens[1:601] < k)       # the first run sits at window offset 2 * MIN_MT ...
    r_lo, r_hi = _min_slices(zcuts, k, False)
    assert r_lo[0] == 0 and r_hi[0] == 603 and r_lo[2] == 601              # ... wholly inside tile 0's slice, in front of tile 2's
    assert lens[601] >= k and np.all(lens[602:902] < k) and lens[902] >= k  # the second run: records 602 .. 901
    assert r_lo[1] == 0 and r_hi[1] == 603 and 602 < r_hi[1] < 901          # the slice of tile 1 ends inside it
    if k == 5:   # (a circular record has as many windows as bases: only the smallest k keeps M_REC records under a tile)
        for name in ("fixed", "edge"):
            assert _min_entries(_min_input(name, k, w)[1], k, True).max() > M_REC, name
    # nwin in {w - 1, w, w + 1}
    lens = np.diff(_min_input("edge", k, w)[1].astype(np.int64))
    assert set(np.maximum(lens - k + 1, 0).tolist()) == {w - 1, w, w + 1}


def _oracle_minimizer_records(O, bases, cuts, k, w, circular):
    hs, ps = [], []
    for r in range(len(cuts) - 1):
        seq = bases[int(cuts[r]):int(cuts[r + 1])]
        try:
            h, p = O.minimizer(seq, k, w, circular=circular)
        except ValueError:     # ErrShortSeq: record skipped (count.go:323-328)
            continue
        hs.append(h)
        ps.append(p)
    if not hs:
        return np.empty(0, np.uint64), np.empty(0, np.uint64)
    return np.concatenate(hs), np.concatenate(ps)


def _check_minimizer(ctx, O, bases, cuts, k, w, circulars=(False, True), max_hash=0):
    for circular in circulars:
        exp, epos = _oracle_minimizer_records(O, bases, cuts, k, w, circular)
        got, gpos = ctx.minimizer(bases, cuts, k, w, circular=circular, with_pos=True)
        assert np.array_equal(got, exp) and np.array_equal(gpos, epos), (k, w, circular)
        assert ctx.stat("window_route") == ROUTE_WINDOW      # (the inner ntHash pass of a small input)
        assert np.array_equal(ctx.minimizer(bases, cuts, k, w, circular=circular), exp), (k, w, circular)
        if max_hash:
            keep = exp <= np.uint64(max_hash)
            got, gpos = ctx.minimizer(bases, cuts, k, w, circular=circular, max_hash=max_hash, with_pos=True)
            assert np.array_equal(got, exp[keep]) and np.array_equal(gpos, epos[keep]), (k, w, circular, "max_hash")


@pytest.mark.gpu
@pytest.mark.parametrize("k,w", MIN_KW)
def test_minimizer_record_table(ctx, O, k, w):
    """hashes and positions against the oracle, record by record, on tiles whose slice of the window-offset table fits LDS
    exactly, misses it by one entry and misses it by far; linear and circular, with and without positions and max_hash"""
    for name in MIN_LAYOUTS:
        bases, cuts = _min_input(name, k, w)
        _check_minimizer(ctx, O, bases, cuts, k, w, max_hash=O.max_hash(3))


# ============================================================ 4. minimizer_kernel: every shape of the sparse table
SPARSE_K = 7
SPARSE_WS = sorted(set(range(1, 67)) | {x for t in range(1, MW_MAX.bit_length()) for x in range((1 << t) - 1, (1 << t) + 3) if x <= MW_MAX} | {MW_MAX})


@functools.lru_cache(maxsize=None)
def _sparse_input():
    low = b"A" * 700 + b"AC" * 400 + b"T" * 500 + b"ACG" * 300 + b"GA" * 350 + b"C" * 300
    head = np.concatenate([np.frombuffer(low, dtype=np.uint8), _random_bases(6000 - len(low), 41)])
    dense = [7 + i % 14 for i in range(300)]
    cuts = _cuts([len(head)] + dense)
    tail = _random_bases(int(cuts[-1]) - len(head), 42)
    tail[:600] = ord("G")    # ties inside the short records too
    return np.concatenate([head, tail]), cuts


def test_minimizer_sparse_table_shapes():
    """no GPU: every w up to 66, both sides of every power of two up to MW_MAX and MW_MAX itself; the long record has a group
    for every one of them, and equal hashes next to each other (the leftmost-minimum rule decides)"""
    bases, cuts = _sparse_input()
    assert int(cuts[1]) == 6000 and int(cuts[1]) - SPARSE_K + 1 >= MW_MAX + 1
    assert SPARSE_WS[0] == 1 and SPARSE_WS[-1] == MW_MAX and set(range(1, 67)) <= set(SPARSE_WS)
    for t in range(1, MW_MAX.bit_length()):
        assert {x for x in range((1 << t) - 1, (1 << t) + 3) if x <= MW_MAX} <= set(SPARSE_WS)
    assert _min_entries(cuts, SPARSE_K, False).max() > M_REC


@pytest.mark.gpu
def test_minimizer_sparse_table(ctx, O, L):
    bases, cuts = _sparse_input()
    for w in SPARSE_WS:
        _check_minimizer(ctx, O, bases, cuts, SPARSE_K, w, circulars=(False,))
    for w in (2, 3, 64, 65, MW_MAX):
        _check_minimizer(ctx, O, bases, cuts, SPARSE_K, w, circulars=(True,))
    with pytest.raises(L.UkmError) as e:
        ctx.minimizer(bases, cuts, SPARSE_K, MW_MAX + 1)
    assert e.value.code == L.ERR_INVALID


# ============================================================ 5. nthash_strip_kernel: ST_CAP candidates in one tile
CAP_K = 31
CAP_L = 256                       # pinned with option strip_l
CAP_TILE = ST_NT * CAP_L
CAP_TILES = 3
CAP_MS = (ST_CAP - 1, ST_CAP, ST_CAP + 1)


@functools.lru_cache(maxsize=None)
def _small_hash_kmer():
    """the 31-mer with the smallest canonical ntHash among 400,000 random windows, and that hash"""
    from oracle import oracle as O
    pool = _random_bases(400_000 + CAP_K - 1, 5)
    h = O.count_windows(pool, np.array([0, len(pool)], dtype=np.uint64), CAP_K, hashed=True)
    i = int(np.argmin(h))
    return pool[i:i + CAP_K].copy(), int(h[i])


@functools.lru_cache(maxsize=None)
def _cap_input(m, with_cuts):
    """three tiles of random bases; in the middle one a stretch of m copies of the 31-mer `u`: with max_hash = hash(u) the
    middle tile lists m candidates.  with_cuts: ten record boundaries inside ten of the copies: those ten stay listed (the
    list is filled before a candidate is checked against the record table) and are dropped afterwards."""
    u, hu = _small_hash_kmer()
    n = CAP_TILES * CAP_TILE
    bases = _random_bases(n, 77)
    s = CAP_TILE + 1003
    bases[s:s + CAP_K * m] = np.tile(u, m)
    marks = [0, 1000, 1000, 1010, CAP_TILE - 5, n]
    if with_cuts:
        marks += [s + CAP_K * (100 * j + 50) + 15 for j in range(10)]
    return bases, np.array(sorted(marks), dtype=np.uint64), hu


def _hits(bases, max_hash, k=CAP_K):
    """positions of the candidates: the whole base array hashed as ONE record"""
    from oracle import oracle as O
    h = O.count_windows(bases, np.array([0, len(bases)], dtype=np.uint64), k, hashed=True)
    return np.nonzero(h <= np.uint64(max_hash))[0]


def test_nthash_strip_candidate_list_shapes():
    """no GPU: the middle tile lists ST_CAP - 1, ST_CAP and ST_CAP + 1 candidates, the other tiles next to none; the cuts
    variant lists the same and loses exactly ten of them to record boundaries"""
    from oracle import oracle as O
    _, hu = _small_hash_kmer()
    assert hu < (1 << 64) // 200_000
    for with_cuts in (False, True):
        for m in CAP_MS if not with_cuts else CAP_MS[1:]:
            bases, cuts, mh = _cap_input(m, with_cuts)
            pos = _hits(bases, mh)
            per = np.bincount(pos // CAP_TILE, minlength=CAP_TILES)
            assert per.tolist() == [0, m, 0], (m, with_cuts, per)     # (no candidate in the random background)
            valid = len(O.count_windows(bases, cuts, CAP_K, hashed=True, max_hash=mh))
            assert valid == m - (10 if with_cuts else 0), (m, with_cuts)
    # one lane: a run of one base, max_hash its hash: every window is a candidate, ST_CAP of them in the first lane's strip
    assert ST_L_MAX == ST_CAP, "the one-lane input needs a strip as long as the list"
    for nw in CAP_MS:
        bases, cuts, mh = _one_lane_input(nw)
        pos = _hits(bases, mh)
        assert len(pos) == nw and pos.max() // ST_L_MAX <= 1 and len(bases) <= ST_NT * ST_L_MAX


@functools.lru_cache(maxsize=None)
def _one_lane_input(nw):
    from oracle import oracle as O
    bases = np.full(nw + CAP_K - 1, ord("A"), dtype=np.uint8)
    cuts = np.array([0, len(bases)], dtype=np.uint64)
    return bases, cuts, int(O.count_windows(bases[:CAP_K], np.array([0, CAP_K], dtype=np.uint64), CAP_K, hashed=True)[0])


def _check_strip_filter(ctx, O, bases, cuts, mh, declines, what):
    exp = O.count_windows(bases, cuts, CAP_K, hashed=True, max_hash=mh)
    d0 = ctx.stat("window_strip_declined")
    got = ctx.nthash(bases, cuts, CAP_K, max_hash=mh)
    assert np.array_equal(got, exp), what
    assert ctx.stat("window_route") == (ROUTE_WINDOW if declines else ROUTE_NTSTRIP), what
    assert ctx.stat("window_strip_declined") == d0 + int(declines), what
    return len(exp)


@pytest.mark.gpu
def test_nthash_strip_candidate_list(ctx, O):
    """ST_CAP - 1 and ST_CAP candidates in one tile: the strip kernel answers (a full list, every slot used); ST_CAP + 1: it
    gives up.  The list counts candidates before they are checked against the records: ST_CAP listed of which ten are not
    valid stays with the strip kernel and returns the others in window order; ST_CAP + 1 listed gives up although fewer than
    ST_CAP are valid."""
    with _opts(ctx, nthash_strip=1, strip_l=CAP_L):
        for m in CAP_MS:
            bases, cuts, mh = _cap_input(m, False)
            assert _check_strip_filter(ctx, O, bases, cuts, mh, m > ST_CAP, ("plain", m)) == m
        for m in CAP_MS[1:]:
            bases, cuts, mh = _cap_input(m, True)
            assert _check_strip_filter(ctx, O, bases, cuts, mh, m > ST_CAP, ("cuts", m)) == m - 10
        # the full list once more with ticketed tile ids
        bases, cuts, mh = _cap_input(ST_CAP, False)
        with _opts(ctx, force_ticket=1):
            _check_strip_filter(ctx, O, bases, cuts, mh, False, ("ticket", ST_CAP))
    with _opts(ctx, nthash_strip=1, strip_l=ST_L_MAX):
        for nw in CAP_MS:
            bases, cuts, mh = _one_lane_input(nw)
            assert _check_strip_filter(ctx, O, bases, cuts, mh, nw > ST_CAP, ("one lane", nw)) == nw


# ============================================================ 6. every k
EVERY_N = 70_000


@functools.lru_cache(maxsize=None)
def _every_k_input():
    """ragged records: every length from 0 to 130 once, in order, then three long ones; IUPAC and lower-case bases"""
    lens = list(range(131))
    rest = EVERY_N - sum(lens)
    lens += [20_000, 20_000, rest - 40_000]
    return _random_bases(EVERY_N, 6, ragged_alphabet=True), _cuts(lens)


EVERY_FILTER_L = 64     # pinned with option strip_l
EVERY_SCALE = 50


@functools.lru_cache(maxsize=None)
def _every_k_filter_candidates(k):
    """the most candidates one tile of nthash_strip_kernel lists at --scale EVERY_SCALE"""
    from oracle import oracle as O
    pos = _hits(_every_k_input()[0], O.max_hash(EVERY_SCALE), k)
    return int(np.bincount(pos // (ST_NT * EVERY_FILTER_L)).max()) if len(pos) else 0


def test_every_k_shapes():
    """no GPU: the input spans many tiles of window_kernel and several of stripwin_kernel at both default strip lengths,
    and no strip tile touches more records than the table holds (forced on, the strip kernel answers)"""
    bases, cuts = _every_k_input()
    lens = np.diff(cuts.astype(np.int64))
    assert len(bases) == EVERY_N == int(cuts[-1]) and lens[:131].tolist() == list(range(131)) and lens.min() >= 0
    assert EVERY_N > 8 * ENC_WT
    for strip_l in (SW_L_K32, SW_L_K64):
        nr = _records_per_tile(cuts, SW_NT * strip_l)
        assert len(nr) >= 3 and nr.max() <= SW_REC, (strip_l, nr)
    assert len(set(bases.tolist()) - set(b"ACGT")) >= 10
    # the Scaled filter: at the pinned strip length no tile lists more candidates than the list holds, whatever k is
    most = [_every_k_filter_candidates(k) for k in range(1, 65)]
    assert 0 < max(most) <= ST_CAP, most


# ============================================================ the proofs notice an input that is one step off its limit
def _without_cut(builder, pick):
    """the builder's input with one record boundary taken out (two records merged); pick(*args, cuts) -> index or None"""
    def build(*a):
        out = builder(*a)
        i = pick(*a, out[1])
        return out if i is None else (out[0], np.delete(out[1], i)) + tuple(out[2:])
    return build


def test_shape_proofs_reject_inputs_one_step_off(monkeypatch):
    """no GPU: each shape proof above fails when its input is moved one record (one candidate, one w) off its limit"""
    import sys
    me = sys.modules[__name__]
    # 1. the SW_REC input with two records of its dense tile merged: SW_REC - 1 records
    monkeypatch.setattr(me, "_sw_input", _without_cut(_sw_input, lambda k, nr, where, cuts:
                        int(np.searchsorted(cuts, SW_WHERE[where] * SW_TILE)) + 1 if nr == SW_REC else None))
    with pytest.raises(AssertionError):
        test_stripwin_record_table_shapes("middle")
    monkeypatch.undo()
    # 2. ukm_count's dense input with one 40-base record fewer: SW_REC records under that tile, no decline
    monkeypatch.setattr(me, "_count_input", _without_cut(_count_input, lambda dense, cuts:
                        int(np.argmax(np.diff(cuts.astype(np.int64)) == 40)) + 1 if dense else None))
    with pytest.raises(AssertionError):
        test_count_declined_strip_shapes()
    monkeypatch.undo()
    # 3. `mixed` with one tiny record fewer in its first block: M_REC - 1 entries where the proof wants M_REC
    monkeypatch.setattr(me, "_min_input", _without_cut(_min_input, lambda layout, k, w, cuts: 3 if layout == "mixed" else None))
    with pytest.raises(AssertionError):
        test_minimizer_record_table_shapes(5, 3)
    monkeypatch.undo()
    # 4. the sparse table without w = MW_MAX
    monkeypatch.setattr(me, "SPARSE_WS", [w for w in SPARSE_WS if w != MW_MAX])
    with pytest.raises(AssertionError):
        test_minimizer_sparse_table_shapes()
    monkeypatch.undo()
    # 5. the ST_CAP input with one more copy of the 31-mer: ST_CAP + 1 candidates
    cap_input = _cap_input
    monkeypatch.setattr(me, "_cap_input", lambda m, with_cuts: cap_input(m + 1 if (m == ST_CAP and not with_cuts) else m, with_cuts))
    with pytest.raises(AssertionError):
        test_nthash_strip_candidate_list_shapes()
    monkeypatch.undo()
    # 6. the every-k input with 150 more records under its first strip tile
    bases, cuts = _every_k_input()
    more = np.sort(np.concatenate([cuts, np.arange(9000, 9000 + 150 * 20, 20, dtype=np.uint64)]))
    monkeypatch.setattr(me, "_every_k_input", lambda: (bases, more))
    with pytest.raises(AssertionError):
        test_every_k_shapes()
    monkeypatch.undo()
    # ... and every one of them passes again on the inputs as they are
    test_stripwin_record_table_shapes("middle")
    test_count_declined_strip_shapes()
    test_minimizer_record_table_shapes(5, 3)
    test_minimizer_sparse_table_shapes()
    test_nthash_strip_candidate_list_shapes()
    test_every_k_shapes()


@pytest.mark.gpu
@pytest.mark.parametrize("hashed", [False, True], ids=["codes", "nthash"])
def test_every_k(ctx, O, hashed):
    """k = 1 .. 32 (codes) / 1 .. 64 (ntHash), canonical and forward: linear records through window_kernel and through
    stripwin_kernel, circular records through window_kernel"""
    bases, cuts = _every_k_input()
    fn = ctx.nthash if hashed else ctx.encode_kmers
    for k in range(1, (64 if hashed else 32) + 1):
        for canonical in (True, False):
            for circular in (False, True):
                exp = O.count_windows(bases, cuts, k, hashed=hashed, canonical=canonical, circular=circular)
                what = (k, canonical, circular)
                d0 = ctx.stat("window_strip_declined")
                with _opts(ctx, win_strip=0):
                    assert np.array_equal(fn(bases, cuts, k, canonical=canonical, circular=circular), exp), what
                    assert ctx.stat("window_route") == ROUTE_WINDOW, what
                if not circular:
                    with _opts(ctx, win_strip=1):
                        assert np.array_equal(fn(bases, cuts, k, canonical=canonical), exp), what
                        assert ctx.stat("window_route") == ROUTE_STRIPWIN, what
                assert ctx.stat("window_strip_declined") == d0, what


@pytest.mark.gpu
def test_every_k_scaled_filter(ctx, O):
    """the Scaled filter at --scale 50 for every k through window_kernel and through nthash_strip_kernel (pinned strip length: the
    proof counts the candidates of every tile, the list holds them for every k)"""
    bases, cuts = _every_k_input()
    mh = O.max_hash(EVERY_SCALE)
    for k in range(1, 65):
        exp = O.count_windows(bases, cuts, k, hashed=True, max_hash=mh)
        d0 = ctx.stat("window_strip_declined")
        with _opts(ctx, nthash_strip=0):
            assert np.array_equal(ctx.nthash(bases, cuts, k, max_hash=mh), exp), k
            assert ctx.stat("window_route") == ROUTE_WINDOW and ctx.stat("window_strip_declined") == d0, k
        with _opts(ctx, nthash_strip=1, strip_l=EVERY_FILTER_L):
            assert np.array_equal(ctx.nthash(bases, cuts, k, max_hash=mh), exp), k
            assert ctx.stat("window_route") == ROUTE_NTSTRIP and ctx.stat("window_strip_declined") == d0, k
