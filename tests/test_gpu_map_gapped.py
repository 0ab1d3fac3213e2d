"""ukm_map_gapped on the GPU: `unikmer map` with -x / -X / --circular.

Every expected value comes from tests/map_model.py -- model_map_gapped, the loop of map.go:298-490 with its per-record reset,
over G / B / M classes from the CPU oracle's kmer_iter / hash_iter -- never from the library under test.  Every call is made
with host inputs and with torch device inputs.  The run kernel's tile is 2048 stream positions, the run-indexed kernels' tile
256 runs: the shapes straddle both.
"""
import ctypes as C
import re

import numpy as np
import pytest

import map_model as M

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
GAPS = [(1, 1), (2, 3), (3, 255), (7, 2), (100000, 1)]


@pytest.fixture(scope="module")
def env():
    from unikmer_amd import lib
    from oracle import oracle
    ctx = lib.Context(0)
    yield lib, ctx, oracle
    ctx.close()


def _rows(*cols):
    return [tuple(int(v) for v in row) for row in zip(*cols)]


def _dev(x, dtype, pad=0):
    """a device tensor with the content of x; pad = 1: at an odd offset (one item) inside a larger allocation"""
    import torch
    a = np.ascontiguousarray(x, dtype=dtype).view({np.uint64: np.int64, np.uint32: np.int32, np.uint8: np.uint8}[dtype])
    t = torch.empty(len(a) + pad, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    t[pad:] = torch.from_numpy(a).cuda()
    return t[pad:]


def _host(t, dtype):
    return t.cpu().numpy().view(dtype) if hasattr(t, "cpu") else t


def _offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return off


def _records(seed, lens, k, plant=False):
    """random records; plant: a piece of record 0 reappears inside the later records and twice in record 0"""
    rng = np.random.default_rng(seed)
    recs = [ACGT[rng.integers(0, 4, n)].copy() for n in lens]
    if plant:
        piece = recs[0][10:10 + 3 * k].copy()
        recs[0][200:200 + len(piece)] = piece
        for r in recs[1:]:
            if len(r) > 100 + len(piece):
                r[50:50 + len(piece)] = piece
    return np.concatenate(recs), _offsets(lens)


class Call:
    """one genome and one set on the host and on the device; both must give what the model gives"""

    def __init__(self, ctx, bases, off, goff, k, codes, pad=0):
        self.ctx, self.k = ctx, k
        self.host = (bases, off, goff, codes)
        self.dev = (_dev(bases, np.uint8, pad), _dev(off, np.uint64, pad), _dev(goff, np.uint64, pad), _dev(codes, np.uint64, pad))

    def run(self, where, **kw):
        b, o, g, s = self.host if where == "host" else self.dev
        out = self.ctx.map_gapped(b, o, g, self.k, s, **kw)
        assert hasattr(out[0], "cpu") == (where == "dev")
        return _rows(_host(out[0], np.uint32), _host(out[1], np.uint64), _host(out[2], np.uint64))

    def both(self, **kw):
        h = self.run("host", **kw)
        assert self.run("dev", **kw) == h, kw
        return h


def _want(cls, off, k, circular, min_len, x, X):
    lens = [int(b - a) for a, b in zip(off[:-1], off[1:])]
    return M.model_map_gapped(cls, lens, k, circular, min_len, x, X)


# ---- 1. random classes ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(9, False, False), (31, False, True), (51, True, False)], ids=["k9", "k31planted", "k51hashed"])
def random_genome(request, env):
    lib, ctx, O = env
    k, hashed, plant = request.param
    lens = [3000, 17, 4, 2048 + k - 1, 6000, k, k - 1, 9000]
    bases, off = _records(100 + k, lens, k, plant)
    wins = {c: M.windows(O, bases, off, k, hashed, c) for c in (False, True)}
    allw = np.unique(np.array([c for w in wins[True] if w is not None for c in w], dtype=np.uint64))
    codes = allw[np.random.default_rng(k).random(len(allw)) < 0.8]
    n_rec = len(lens)
    groupings = {"per_record": (np.arange(n_rec + 1, dtype=np.uint64), list(range(n_rec))),
                 "one_genome": (np.array([0, n_rec], dtype=np.uint64), [0] * n_rec)}
    cls = {(g, c, a): M.classes(wins[c], gof, set(codes.tolist()), a)
           for g, (goff, gof) in groupings.items() for c in (False, True) for a in (False, True)}
    return k, hashed, bases, off, codes, groupings, cls


def test_random_classes(env, random_genome):
    lib, ctx, O = env
    k, hashed, bases, off, codes, groupings, cls = random_genome
    if k == 9:   # the records' own repeats give multiple-mapped windows; misses of length 1-3 abound everywhere
        assert sum(c.count("B") for c in cls["per_record", False, False] if c) > 100
    assert sum(len(re.findall("GM{1,3}G", c)) for c in cls["per_record", False, True] if c) > 1000
    regions = 0
    for g, (goff, gof) in groupings.items():
        call = Call(ctx, bases, off, goff, k, codes)
        for circular in (False, True):
            for allow in (False, True):
                for x, X in GAPS:
                    for min_len in (1, k, 3 * k):
                        want = _want(cls[g, circular, allow], off, k, circular, min_len, x, X)
                        regions += len(want)
                        kw = dict(hashed=hashed, circular=circular, allow_multi=allow, min_len=min_len, max_gap_size=x, max_gap_num=X)
                        for route in (0, 1):
                            ctx.set_option("map_sorted", route)
                            try:
                                got = call.both(**kw)
                            finally:
                                ctx.set_option("map_sorted", None)
                            assert got == want, (g, kw, route)
    assert regions > 10_000


def test_without_gaps_on_linear_records_it_is_ukm_map(env, random_genome):
    """6. x = 0 (X = 0 and X = 5): all three output arrays equal Context.map's"""
    lib, ctx, O = env
    k, hashed, bases, off, codes, groupings, cls = random_genome
    for g, (goff, gof) in groupings.items():
        for allow in (False, True):
            for min_len in (1, k, 3 * k):
                ref = ctx.map(bases, off, goff, k, codes, hashed=hashed, allow_multi=allow, min_len=min_len)
                assert _rows(*ref) == _want(cls[g, False, allow], off, k, False, min_len, 0, 0)
                for X in (0, 5):
                    got = ctx.map_gapped(bases, off, goff, k, codes, hashed=hashed, allow_multi=allow, min_len=min_len, max_gap_num=X)
                    assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, ref)), (g, allow, min_len, X)


# ---- 2. one long chain across tiles --------------------------------------------------------------------------------------
@pytest.mark.parametrize("planted", [False, True], ids=["one_chain", "head_on_tile_start"])
def test_one_long_chain_across_tiles(env, planted):
    lib, ctx, O = env
    k, nw = 31, 5000
    bases, off = _records(7, [nw + k - 1], k)
    wins = M.windows(O, bases, off, k)
    keep = list(range(0, nw, 2))
    if planted:
        keep.remove(512)                      # windows 511..513 miss: run 256 (window 514) heads a second chain
    codes = np.unique(np.array([wins[0][i] for i in keep], dtype=np.uint64))
    cls = M.classes(wins, [0], set(codes.tolist()), True)
    runs = [m.start() for m in re.finditer("G+", cls[0])]
    assert cls[0].count("G") == len(runs) == len(keep) and (not planted or (runs[256] == 514 and runs[255] == 510))
    goff = np.array([0, 1], dtype=np.uint64)
    call = Call(ctx, bases, off, goff, k, codes)
    for X in (1, 2, 6, 255, 256, 4000):
        want = _want(cls, off, k, False, 1, 1, X)
        chains = [256, len(runs) - 256] if planted else [len(runs)]
        assert len(want) == sum(-(-c // (X + 1)) for c in chains)
        assert call.both(allow_multi=True, min_len=1, max_gap_size=1, max_gap_num=X) == want, X


# ---- 3. record boundaries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trim", [(0, 0), (1, 0), (0, 1), (1, 1)], ids=["GG", "MG", "GM", "MM"])
def test_no_region_spans_two_records(env, trim):
    lib, ctx, O = env
    k = 21
    bases, off = _records(13, [700, 500], k)
    wins = M.windows(O, bases, off, k)
    n0 = len(wins[0])
    a0, a1 = n0 - 50, n0 - 1 - trim[0]        # record 0 ends in G (or in one M)
    b0, b1 = trim[1], 49                      # record 1 begins in G (or in one M)
    codes = np.unique(np.array(wins[0][a0:a1 + 1] + wins[1][b0:b1 + 1], dtype=np.uint64))
    cls = M.classes(wins, [0, 1], set(codes.tolist()), True)
    assert cls[0].endswith("G" * 10 + "M" * trim[0]) and cls[1].startswith("M" * trim[1] + "G" * 10)
    call = Call(ctx, bases, off, np.arange(3, dtype=np.uint64), k, codes)
    for x, X in ((2, 3), (5, 1), (100000, 255)):
        want = _want(cls, off, k, False, 1, x, X)
        assert want == [(0, a0, a1 + k), (1, b0, b1 + k)]
        assert call.both(allow_multi=True, min_len=1, max_gap_size=x, max_gap_num=X) == want, (x, X)


# ---- 4. a multiple-mapped window inside a small gap --------------------------------------------------------------------------
def test_multiple_mapped_window_inside_a_small_gap(env):
    lib, ctx, O = env
    k, p = 15, 300
    bases, off = _records(17, [2000], k)
    bases = bases.copy()
    bases[1300:1300 + k] = bases[p + 3:p + 3 + k]          # window p + 3 reappears as window 1300
    bases[1299] = ACGT[(bytes(ACGT).index(bases[p + 2]) + 1) % 4]     # ... and only that window
    wins = M.windows(O, bases, off, k)
    assert wins[0][p + 3] == wins[0][1300] and wins[0][p + 2] != wins[0][1299]
    codes = np.unique(np.array([wins[0][p + i] for i in (0, 1, 3, 5, 6)], dtype=np.uint64))
    goff = np.array([0, 1], dtype=np.uint64)
    call = Call(ctx, bases, off, goff, k, codes)
    for allow, pattern, regions in ((False, "GGMBMGG", [(0, p, p + 1 + k), (0, p + 5, p + 6 + k)]), (True, "GGMGMGG", [(0, p, p + 6 + k)])):
        cls = M.classes(wins, [0], set(codes.tolist()), allow)
        assert cls[0][p - 1:p + 8] == "M" + pattern + "M"
        want = _want(cls, off, k, False, k + 1, 3, 5)
        assert want == regions
        assert call.both(allow_multi=allow, min_len=k + 1, max_gap_size=3, max_gap_num=5) == want, allow


# ---- 5. circular -----------------------------------------------------------------------------------------------------------
def test_circular(env):
    lib, ctx, O = env
    k = 19
    lens = [400, k, k - 1, 300]
    bases, off = _records(19, lens, k)
    wins = M.windows(O, bases, off, k, circular=True)
    assert [None if w is None else len(w) for w in wins] == [400, k, None, 300]
    goff = np.arange(5, dtype=np.uint64)
    everything = np.unique(np.array([c for w in wins if w is not None for c in w], dtype=np.uint64))
    # wholly covered records: one region (0, L) each -- the record of exactly k bases too, none for the one of k - 1
    call = Call(ctx, bases, off, goff, k, everything)
    cls = M.classes(wins, [0, 1, 2, 3], set(everything.tolist()), True)
    for x, X, min_len in ((0, 0, 1), (0, 0, k), (3, 2, 1), (3, 2, 2 * k)):
        want = _want(cls, off, k, True, min_len, x, X)
        assert want == [(0, 0, 400), (1, 0, k), (3, 0, 300)]
        assert call.both(circular=True, allow_multi=True, min_len=min_len, max_gap_size=x, max_gap_num=X) == want
    # an uncovered stretch in the middle of record 0: the head region, and one that starts behind the stretch and ends past L
    a, b = 150, 180
    part = np.setdiff1d(everything, np.array(wins[0][a:b + 1], dtype=np.uint64))
    call = Call(ctx, bases, off, goff, k, part)
    cls = M.classes(wins, [0, 1, 2, 3], set(part.tolist()), True)
    assert cls[0] == "G" * a + "M" * (b - a + 1) + "G" * (400 - b - 1)
    for min_len in (1, k, 2 * k):                          # (1 < k: nothing is emitted behind the circular `break`)
        want = _want(cls, off, k, True, min_len, 2, 2)
        assert want == [(0, 0, a - 1 + k), (0, b + 1, 400 + a - 1 + k), (1, 0, k), (3, 0, 300)]
        assert call.both(circular=True, allow_multi=True, min_len=min_len, max_gap_size=2, max_gap_num=2) == want
    # a gap the chain may cross: the whole circle again, clipped to L
    assert call.both(circular=True, allow_multi=True, min_len=1, max_gap_size=b - a + 1, max_gap_num=1) == \
        _want(cls, off, k, True, 1, b - a + 1, 1) == [(0, 0, 400), (1, 0, k), (3, 0, 300)]
    # short runs everywhere, multiple-mapped windows counted among the circular windows, min_len below k
    rng = np.random.default_rng(23)
    bases2 = bases.copy()
    r3 = int(off[3])
    bases2[r3 + 285:r3 + 300] = bases2[r3 + 100:r3 + 115]  # a repeat that wraps: windows 285.. of record 3 = its windows 100..
    bases2[r3:r3 + 10] = bases2[r3 + 115:r3 + 125]
    wins2 = M.windows(O, bases2, off, k, circular=True)
    assert wins2[3][285:292] == wins2[3][100:107]
    every2 = np.unique(np.array([c for w in wins2 if w is not None for c in w], dtype=np.uint64))
    sparse = every2[rng.random(len(every2)) < 0.7]
    call = Call(ctx, bases2, off, goff, k, sparse)
    for allow in (False, True):
        cls = M.classes(wins2, [0, 1, 2, 3], set(sparse.tolist()), allow)
        assert allow or "B" in cls[3][285:292]
        for x, X in ((0, 0), (1, 1), (3, 2)):
            for min_len in (1, 5, k, 2 * k):
                want = _want(cls, off, k, True, min_len, x, X)
                assert call.both(circular=True, allow_multi=allow, min_len=min_len, max_gap_size=x, max_gap_num=X) == want, (allow, x, X, min_len)


# ---- 7. contracts ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(env):
    lib, ctx, O = env
    k = 23
    bases, off = _records(29, [4000, 30, 2500], k)
    wins = M.windows(O, bases, off, k)
    allw = np.unique(np.array([c for w in wins if w is not None for c in w], dtype=np.uint64))
    codes = allw[np.random.default_rng(2).random(len(allw)) < 0.8]
    goff = np.arange(4, dtype=np.uint64)
    cls = M.classes(wins, [0, 1, 2], set(codes.tolist()), False)
    want = _want(cls, off, k, False, k, 2, 2)
    assert len(want) > 100
    return k, bases, off, goff, codes, want


def _raw(lib, ctx, arrs, k, cap, outs, x=2, X=2, min_len=None):
    ptr = [lib._ptr(a, dt)[0] for a, dt in zip(arrs, (np.uint8, np.uint64, np.uint64, np.uint64))]
    po = [lib._ptr(o, dt)[0] for o, dt in zip(outs, (np.uint32, np.uint64, np.uint64))]
    n = C.c_uint64()
    rc = ctx.L.ukm_map_gapped(ctx.h, ptr[0], ptr[1], len(arrs[1]) - 1, ptr[2], len(arrs[2]) - 1, k, 0, 0, ptr[3], len(arrs[3]), 0,
                              k if min_len is None else min_len, x, X, po[0], po[1], po[2], cap, C.byref(n))
    return rc, n.value


def test_capacity_one_short(env, small):
    lib, ctx, O = env
    k, bases, off, goff, codes, want = small
    cap = len(want) - 1
    with pytest.raises(lib.CapacityError) as e:
        ctx.map_gapped(bases, off, goff, k, codes, min_len=k, max_gap_size=2, max_gap_num=2, out_cap=cap)
    assert e.value.needed == len(want)
    host = (bases, off, goff, codes)
    dev = tuple(_dev(a, dt) for a, dt in zip(host, (np.uint8, np.uint64, np.uint64, np.uint64)))
    for arrs, mk in ((host, lambda dt: np.full(cap + 8, 0xA5, dtype=dt)), (dev, lambda dt: _dev(np.full(cap + 8, 0xA5, dtype=dt), dt))):
        outs = [mk(np.uint32), mk(np.uint64), mk(np.uint64)]
        rc, n = _raw(lib, ctx, arrs, k, cap, outs)
        assert rc == lib.ERR_CAPACITY and n == len(want)
        for o, dt in zip(outs, (np.uint32, np.uint64, np.uint64)):
            assert np.all(_host(o, dt)[cap:] == 0xA5)
        # and with room for all of them: exactly n entries, nothing behind
        outs = [mk(np.uint32), mk(np.uint64), mk(np.uint64)]
        rc, n = _raw(lib, ctx, arrs, k, cap + 1, outs)
        assert rc == 0 and n == len(want)
        assert _rows(*[_host(o, dt)[:n] for o, dt in zip(outs, (np.uint32, np.uint64, np.uint64))]) == want
        for o, dt in zip(outs, (np.uint32, np.uint64, np.uint64)):
            assert np.all(_host(o, dt)[n:] == 0xA5)


def test_invalid_arguments_and_ukm_maps_errors(env, small):
    lib, ctx, O = env
    k, bases, off, goff, codes, want = small
    outs = [np.zeros(16, np.uint32), np.zeros(16, np.uint64), np.zeros(16, np.uint64)]
    arrs = (bases, off, goff, codes)
    for kw in (dict(x=1, X=0), dict(x=1 << 31, X=1), dict(x=1, X=1 << 31), dict(x=0, X=1 << 31), dict(min_len=0)):
        rc, n = _raw(lib, ctx, arrs, k, 16, outs, **kw)
        assert rc == lib.ERR_INVALID, kw
    big = (1 << 31) - 1                                                         # the largest legal values
    wins = M.windows(O, bases, off, k)
    assert _rows(*ctx.map_gapped(bases, off, goff, k, codes, min_len=k, max_gap_size=big, max_gap_num=big)) == \
        _want(M.classes(wins, [0, 1, 2], set(codes.tolist()), False), off, k, False, k, big, big)
    with pytest.raises(lib.UnsortedError):
        ctx.map_gapped(bases, off, goff, k, codes[::-1].copy(), max_gap_size=2, max_gap_num=2)
    bad = bases.copy()
    bad[100] = ord("*")
    with pytest.raises(lib.IllegalBaseError):
        ctx.map_gapped(bad, off, goff, k, codes, max_gap_size=2, max_gap_num=2)
    with pytest.raises(lib.UkmError) as e:
        ctx.map_gapped(bases, off, goff, 33, codes, max_gap_size=2, max_gap_num=2)
    assert e.value.code == lib.ERR_K
    assert len(ctx.map_gapped(bases, off, goff, k, np.empty(0, np.uint64), max_gap_size=2, max_gap_num=2)[0]) == 0


def test_device_buffers_at_odd_offsets(env, small):
    """bases + 1 byte, the 8-byte arrays + 1 element inside a larger allocation; circular as well (the stream offsets are
    computed from a device rec_off)"""
    lib, ctx, O = env
    k, bases, off, goff, codes, want = small
    call = Call(ctx, bases, off, goff, k, codes, pad=1)
    assert call.dev[0].data_ptr() % 2 == 1 and call.dev[1].data_ptr() % 16 == 8
    assert call.run("dev", min_len=k, max_gap_size=2, max_gap_num=2) == want
    wins = M.windows(O, bases, off, k, circular=True)
    cls = M.classes(wins, [0, 1, 2], set(codes.tolist()), False)
    assert call.run("dev", circular=True, min_len=k, max_gap_size=2, max_gap_num=2) == _want(cls, off, k, True, k, 2, 2)


def test_same_result_after_an_unrelated_large_call(env, small):
    """every workspace word the call reads it has written itself (tests/test_gpu_workspace.py states the rule)"""
    lib, ctx, O = env
    k, bases, off, goff, codes, want = small
    kw = dict(min_len=k, max_gap_size=2, max_gap_num=2)
    wins = M.windows(O, bases, off, k, circular=True)
    wantc = _want(M.classes(wins, [0, 1, 2], set(codes.tolist()), False), off, k, True, k, 2, 2)
    assert _rows(*ctx.map_gapped(bases, off, goff, k, codes, **kw)) == want
    assert _rows(*ctx.map_gapped(bases, off, goff, k, codes, circular=True, **kw)) == wantc
    rng = np.random.default_rng(31)
    files = [np.unique(rng.integers(0, 1 << 63, 2_000_000, dtype=np.uint64)) for _ in range(3)]
    assert len(ctx.union(files)) > 5_000_000
    assert _rows(*ctx.map_gapped(bases, off, goff, k, codes, **kw)) == want
    assert _rows(*ctx.map_gapped(bases, off, goff, k, codes, circular=True, **kw)) == wantc
