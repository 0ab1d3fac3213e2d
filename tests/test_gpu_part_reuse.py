"""The partition cache of the public 2-way set operation (ukm_setops.hip): a call on the same
(A, B, |A|, |B|, tile size) as the call before it VERIFIES the cached merge-path table against the inputs as they are now
instead of searching again.  The contract: results never depend on the cache, only time does.

Every case goes through the C ABI (lib.Context is its ctypes binding) on device-resident buffers and compares element for
element with the CPU oracle.  The statistics "setop_part_hits" / "setop_part_stale" say which way a call went.

Sizes: the cache applies from 4 * PART_COARSE = 256 tiles; a plain tile is 512 * 19 = 9728 merged records, so
|A| = |B| = 1.5e6 gives 309 plain tiles (838 with per-record taxids, 489 in the multiset re-run, which never caches).
"""
import functools

import numpy as np
import pytest

from conftest import splitmix64, synth_tree

pytestmark = pytest.mark.gpu

U64, U32 = np.uint64, np.uint32
SEED = 0x70617274
N = 1_500_000
TILE = 512 * 19             # ukm_setop_kernels.h: SETOP_NT x SETOP_VT
MIN_TILES = 4 * 64          # 4 * PART_COARSE
OP_UNION, OP_INTER, OP_DIFF = 0, 1, 2
BASE = U64(1) << U64(32)    # every code lies above 2^32: room for a whole set BELOW the other one


@functools.lru_cache(None)
def _oracle():
    from oracle import oracle as O
    child, parent = synth_tree(5, 8)
    return O, O.Taxonomy(child, parent), child, parent


@functools.lru_cache(None)
def _sets(n=N):
    """two sorted sets of exactly n codes over one universe: a third only in A, a third only in B, a third in both"""
    nu = int(n * 1.52)
    j = np.arange(nu, dtype=U64)
    U = BASE + np.cumsum(U64(2) + (splitmix64(U64(SEED) ^ j) & U64((1 << 24) - 1)), dtype=U64)
    m = splitmix64(U64(SEED + 1) ^ j) % U64(3)
    A, B = U[m != 1][:n], U[m != 0][:n]
    assert len(A) == n and len(B) == n
    return A, B


@functools.lru_cache(None)
def _ref(op):
    O = _oracle()[0]
    A, B = _sets()
    return {OP_UNION: O.union, OP_INTER: O.inter, OP_DIFF: O.diff}[op]([A, B])


def _want(op, A, B):
    O = _oracle()[0]
    return {OP_UNION: O.union, OP_INTER: O.inter, OP_DIFF: O.diff}[op]([A, B])


def merge_path(A, B, tile):
    """mp[t] = how many records of A are among the first min(t * tile, |A| + |B|) of the merged order, A before B on ties"""
    pos = np.arange(len(A), dtype=np.int64) + np.searchsorted(B, A, side="left")   # place of A[i] in the merged order
    n = len(A) + len(B)
    d = np.minimum(np.arange((n + tile - 1) // tile + 1, dtype=np.int64) * tile, n)
    return np.searchsorted(pos, d, side="left")


@pytest.fixture(scope="module")
def lib():
    from unikmer_amd import lib as L
    return L


class Pair:
    """device copies of two sets, a context of their own, and the two counters"""

    def __init__(self, L, A, B):
        import torch
        self.torch = torch
        self.L = L
        self.dev = torch.device("cuda", 0)
        self.ctx = L.Context(0, stream=torch.cuda.current_stream(self.dev).cuda_stream)
        self.A, self.B = self.up(A), self.up(B)
        self.out = torch.empty(len(A) + len(B), dtype=torch.int64, device=self.dev)

    def up(self, x, dtype=np.int64):
        return self.torch.from_numpy(np.ascontiguousarray(x).view(dtype).copy()).to(self.dev)

    def write(self, dst, x):
        """new contents IN PLACE: the same pointer, the same size"""
        assert len(x) == dst.numel()
        dst.copy_(self.up(x))
        self.torch.cuda.synchronize()

    def run(self, op, a=None, b=None, **kw):
        r = self.ctx.setop2(op, self.A if a is None else a, self.B if b is None else b, out=self.out, **kw)
        if isinstance(r, tuple):
            return r[0].cpu().numpy().view(U64), r[1].cpu().numpy().view(U32)
        return r.cpu().numpy().view(U64)

    def counters(self):
        return self.ctx.stat("setop_part_hits"), self.ctx.stat("setop_part_stale")

    def close(self):
        self.ctx.close()


@pytest.fixture
def pair(lib):
    p = Pair(lib, *_sets())
    yield p
    p.close()


def test_sizes_are_what_the_cases_assume():
    A, B = _sets()
    assert (len(A) + len(B) + TILE - 1) // TILE >= MIN_TILES
    assert (len(A) + len(B) + TILE - 1) // TILE < MIN_TILES + 64      # ... and no larger than they need to be


def test_hits(pair):
    """union, inter, diff of one pair: one search, two verified reuses"""
    assert pair.counters() == (0, 0)
    for op in (OP_UNION, OP_INTER, OP_DIFF):
        assert np.array_equal(pair.run(op), _ref(op))
    assert pair.counters() == (2, 0)


def test_hits_with_ticketed_tiles(lib, monkeypatch):
    """the same under UKM_FORCE_TICKET=1 (tile ids from the atomic counter), a grossly stale table included"""
    monkeypatch.setenv("UKM_FORCE_TICKET", "1")
    A, B = _sets()
    p = Pair(lib, A, B)
    try:
        for op in (OP_UNION, OP_INTER, OP_DIFF):
            assert np.array_equal(p.run(op), _ref(op))
        assert p.counters() == (2, 0)
        A2 = np.arange(1, len(A) + 1, dtype=U64)
        p.write(p.A, A2)
        assert np.array_equal(p.run(OP_UNION), _want(OP_UNION, A2, B))
        assert p.counters() == (2, 1)
    finally:
        p.close()


def test_stale_grossly(pair):
    """A rewritten in place with a set that lies entirely below B: every boundary but the ends is wrong"""
    A, B = _sets()
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))
    A2 = np.arange(1, len(A) + 1, dtype=U64)
    assert A2[-1] < B[0]
    pair.write(pair.A, A2)
    got = pair.run(OP_INTER)
    assert pair.counters() == (0, 1)
    assert np.array_equal(got, _want(OP_INTER, A2, B)) and len(got) == 0
    assert np.array_equal(pair.run(OP_UNION), _want(OP_UNION, A2, B))
    assert pair.counters() == (1, 1)         # the table of the repeated search serves the next call
    assert np.array_equal(pair.run(OP_DIFF), A2)
    assert pair.counters() == (2, 1)


def test_stale_by_one(pair):
    """single keys of A changed in place at three tile boundaries: each boundary moves by exactly one record"""
    A, B = _sets()
    mp = merge_path(A, B, TILE)
    A2 = A.copy()
    moved = []
    for t0 in (len(mp) // 4, len(mp) // 2, 3 * len(mp) // 4):
        for t in range(t0, t0 + 20):
            a, b = int(mp[t]), t * TILE - int(mp[t])
            # A[a] comes down to A[a-1] + 1: if that is below B[b-1], A[a] now lies in front of the boundary
            v = A[a - 1] + U64(1)
            if 0 < a < len(A) - 1 and 0 < b < len(B) and v < B[b - 1] and v < A[a]:
                A2[a] = v
                moved.append(t)
                break
    assert len(moved) == 3
    assert np.all(A2[1:] > A2[:-1])
    mp2 = merge_path(A2, B, TILE)
    delta = mp2 - mp
    assert np.array_equal(np.nonzero(delta)[0], np.array(moved)) and np.all(delta[moved] == 1)

    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))
    pair.write(pair.A, A2)
    assert np.array_equal(pair.run(OP_INTER), _want(OP_INTER, A2, B))
    assert pair.counters() == (0, 1)
    assert np.array_equal(pair.run(OP_UNION), _want(OP_UNION, A2, B))
    assert np.array_equal(pair.run(OP_DIFF), _want(OP_DIFF, A2, B))
    assert pair.counters() == (2, 1)


def test_smaller_na_is_a_miss(pair):
    """the same pointers with a smaller |A|: another key -- the table in the slot, whose splits lie beyond the new |A|, is
    never looked at.  A third of |A| leaves fewer than 256 tiles (no cache at all, the slot stays), three quarters do not"""
    A, B = _sets()
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))
    n3 = len(A) // 3
    a3 = pair.A[:n3]
    assert a3.data_ptr() == pair.A.data_ptr()
    for op in (OP_INTER, OP_DIFF, OP_UNION):
        assert np.array_equal(pair.run(op, a=a3), _want(op, A[:n3], B))
    assert pair.counters() == (0, 0)
    assert np.array_equal(pair.run(OP_INTER), _ref(OP_INTER))     # the whole of A again: the slot still holds its table
    assert pair.counters() == (1, 0)
    n4 = 3 * len(A) // 4
    a4 = pair.A[:n4]
    assert (n4 + len(B) + TILE - 1) // TILE >= MIN_TILES
    assert np.array_equal(pair.run(OP_INTER, a=a4), _want(OP_INTER, A[:n4], B))
    assert pair.counters() == (1, 0)                              # a miss that takes the slot
    assert np.array_equal(pair.run(OP_DIFF, a=a4), _want(OP_DIFF, A[:n4], B))
    assert pair.counters() == (2, 0)
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))     # and back: a miss again
    assert pair.counters() == (2, 0)


def test_swapped_arguments_are_a_miss(pair):
    A, B = _sets()
    assert np.array_equal(pair.run(OP_DIFF), _ref(OP_DIFF))
    assert np.array_equal(pair.run(OP_DIFF, a=pair.B, b=pair.A), _want(OP_DIFF, B, A))
    assert pair.counters() == (0, 0)
    assert np.array_equal(pair.run(OP_UNION, a=pair.B, b=pair.A), _ref(OP_UNION))
    assert pair.counters() == (1, 0)


def test_multiset_rerun_never_hits(pair):
    """duplicated runs written in place: the plain pass of each call may use the cache (one attempt per call), the re-run on
    (code, rank) pairs never does"""
    A, B = _sets()
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))
    A2 = A.copy()
    A2[7::7] = A2[6::7][:len(A2[7::7])]            # every seventh code twice ...
    i = np.arange(21, len(A2) - 1, 21)
    A2[i + 1] = A2[i] = A2[i - 1]                  # ... and runs of three and more
    assert np.all(A2[1:] >= A2[:-1]) and np.any(A2[1:] == A2[:-1])
    pair.write(pair.A, A2)
    for k, op in enumerate((OP_INTER, OP_DIFF, OP_UNION, OP_INTER)):
        assert np.array_equal(pair.run(op), _want(op, A2, B))
        h, s = pair.counters()
        assert h + s == k + 1 and s <= 1


def test_unsorted_input(pair, lib):
    A, B = _sets()
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))
    A2 = A.copy()
    A2[len(A) // 2: len(A) // 2 + 20_000] = A2[len(A) // 2: len(A) // 2 + 20_000][::-1].copy()   # two tiles' worth, reversed
    pair.write(pair.A, A2)
    with pytest.raises(lib.UnsortedError):
        pair.run(OP_INTER)
    pair.write(pair.A, A)
    for op in (OP_INTER, OP_UNION, OP_DIFF):
        assert np.array_equal(pair.run(op), _ref(op))


def test_capacity_on_a_hit(pair, lib):
    torch = pair.torch
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))
    need = len(_ref(OP_INTER))
    SENT = -0x5A5A5A5A5A5A5A5B
    for cap in (need - 1, need // 2, 0):
        buf = torch.full((need + 4 * TILE,), SENT, dtype=torch.int64, device=pair.dev)
        h0, s0 = pair.counters()
        with pytest.raises(lib.CapacityError) as e:
            if cap:
                pair.ctx.setop2(OP_INTER, pair.A, pair.B, out=buf[:cap])
            else:   # the size query: NULL output, out_cap 0
                n = lib.C.c_uint64()
                lib._check(pair.ctx.L.ukm_setop2(pair.ctx.h, OP_INTER, pair.A.data_ptr(), None, len(pair.A), pair.B.data_ptr(), None,
                                                 len(pair.B), 0, None, None, 0, lib.C.byref(n)), n.value)
        assert e.value.needed == need
        assert pair.counters() == (h0 + 1, s0)
        assert bool((buf[cap:] == SENT).all())
    assert np.array_equal(pair.run(OP_INTER), _ref(OP_INTER))


def test_taxid_routes(pair):
    """per-record taxids run on tiles of their own size (another key), one taxid per file on the plain tiles"""
    O, tax, child, parent = _oracle()
    A, B = _sets()
    T = len(child)
    ta = (U64(1) + splitmix64(U64(SEED + 2) ^ A) % U64(T)).astype(U32)
    tb = (U64(1) + splitmix64(U64(SEED + 3) ^ B) % U64(T)).astype(U32)
    pair.ctx.taxonomy_load(child, parent)
    dta, dtb = pair.up(ta, np.int32), pair.up(tb, np.int32)
    fa, fb = int(T - 3), int(T - 700)
    outt = pair.torch.empty(len(A) + len(B), dtype=pair.torch.int32, device=pair.dev)
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))
    for op, fn in ((OP_UNION, O.union), (OP_INTER, O.inter), (OP_DIFF, O.diff)):
        wk, wt = fn([A, B], [ta, tb], tax)
        gk, gt = pair.run(op, a_taxids=dta, b_taxids=dtb, out_taxids=outt)
        assert np.array_equal(gk, wk) and np.array_equal(gt, wt)
    for op, fn in ((OP_UNION, O.union), (OP_INTER, O.inter), (OP_DIFF, O.diff)):
        wk, wt = fn([A, B], [np.full(len(A), fa, U32), np.full(len(B), fb, U32)], tax)
        gk, gt = pair.run(op, a_taxids=fa, b_taxids=fb, out_taxids=outt)
        assert np.array_equal(gk, wk) and np.array_equal(gt, wt)
    h0, s0 = pair.counters()
    assert h0 >= 2 and s0 == 0
    assert np.array_equal(pair.run(OP_INTER), _ref(OP_INTER))      # the plain call behind them: the per-file calls' key
    assert pair.counters() == (h0 + 1, 0)


def test_tiny_inputs_never_hit(lib):
    n = 1_000_000
    assert (2 * n + TILE - 1) // TILE < MIN_TILES
    A, B = _sets()
    A, B = A[:n], B[:n]
    p = Pair(lib, A, B)
    try:
        for op in (OP_UNION, OP_INTER, OP_DIFF, OP_UNION):
            assert np.array_equal(p.run(op), _want(op, A, B))
        assert p.counters() == (0, 0)
    finally:
        p.close()


def test_knob_turns_reuse_off(pair, monkeypatch):
    monkeypatch.setenv("UKM_SETOP_PART_REUSE", "0")
    for op in (OP_UNION, OP_INTER, OP_DIFF):
        assert np.array_equal(pair.run(op), _ref(op))
    assert pair.counters() == (0, 0)
    monkeypatch.delenv("UKM_SETOP_PART_REUSE")
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))    # (the calls above left no table behind: a miss)
    assert np.array_equal(pair.run(OP_INTER), _ref(OP_INTER))
    assert pair.counters() == (1, 0)


def test_back_off_after_two_stale_hits_in_a_row(pair):
    """a caller that refills fixed buffers with same-sized batches: after two stale hits in a row the context stops trying"""
    A, B = _sets()
    A2 = np.arange(1, len(A) + 1, dtype=U64)
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))
    pair.write(pair.A, A2)
    assert np.array_equal(pair.run(OP_UNION), _want(OP_UNION, A2, B))
    assert pair.counters() == (0, 1)
    pair.write(pair.A, A)
    assert np.array_equal(pair.run(OP_INTER), _ref(OP_INTER))
    assert pair.counters() == (0, 2)
    for op in (OP_UNION, OP_INTER, OP_DIFF):                       # unchanged inputs: would hit, but nobody tries
        assert np.array_equal(pair.run(op), _ref(op))
    pair.write(pair.A, A2)
    assert np.array_equal(pair.run(OP_DIFF), A2)
    assert pair.counters() == (0, 2)
