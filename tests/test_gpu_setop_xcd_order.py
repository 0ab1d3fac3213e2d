"""The tile order of the set operation's table passes (unikmer_amd/csrc/ukm_setop_order.h; DESIGN.md sections 4.1 and 4.12):
a pass that takes its tiles' offsets from the cached match counts launches 8 * ceil(ntiles / 8) workgroups, and workgroup b
runs tile (b % 8) * chunk + b / 8, so that neighbouring tiles share an L2.  Results never depend on the order, nor on where
the hardware runs a workgroup: every case goes through the C ABI on device-resident buffers, compares element for element
with the CPU oracle, and runs with UKM_SETOP_XCD_ORDER=1 and =0.

Fixture and helpers are those of test_gpu_part_reuse.py / test_gpu_offset_reuse.py.  The partition cache needs 256 tiles of
9728 records, so the shapes are the smallest at which the order can go wrong: 256, 257, 263, 264 and 309 tiles (grids of 256,
264, 264, 264 and 312 workgroups: a count divisible by 8, idle workgroups in the last chunk, a partial last tile), a last
tile of ONE record, and all of B behind all of A (whole chunks of one input only).  The cases run with UKM_SETOP_OFFS_OPS=7
-- union, inter and diff from the table -- except the default-policy sequence.
"""
import functools

import numpy as np
import pytest

from test_gpu_part_reuse import OP_DIFF, OP_INTER, OP_UNION, TILE, U64, Pair, _ref, _sets, _want
from test_gpu_offset_reuse import counters, raised_matches, straddling
from conftest import oracle_by_value_ranges

pytestmark = pytest.mark.gpu

OPS = (OP_UNION, OP_INTER, OP_DIFF)
SENT = -0x5A5A5A5A5A5A5A5B
# name -> |A| + |B|; |A| = half of it, rounded down
SHAPES = {
    "256": 256 * TILE,                  # grid 256: no idle workgroup, a full last tile
    "257": 256 * TILE + 5000,           # grid 264: 7 idle workgroups, a partial last tile
    "257-one": 256 * TILE + 1,          # ... whose last tile holds a single record
    "263": 263 * TILE - 1234,           # grid 264: one idle workgroup
    "264": 264 * TILE,                  # grid 264: divisible by 8 with chunk 33
    "309": 3_000_000,                   # grid 312: the fixture as the other modules use it
}


def ntiles_of(n):
    return (n + TILE - 1) // TILE


def chunk_of(ntiles):
    return (ntiles + 7) // 8


def shape_sets(name):
    A, B = _sets()
    n = SHAPES[name]
    na = n // 2
    return A[:na], B[:n - na]


@functools.lru_cache(None)
def shape_ref(name, op):
    """the oracle's result, computed once for both orders"""
    r = _want(op, *shape_sets(name))
    r.setflags(write=False)
    return r


@pytest.fixture(scope="module")
def lib():
    from unikmer_amd import lib as L
    return L


@pytest.fixture(autouse=True)
def all_three_operations_from_the_table(monkeypatch):
    monkeypatch.setenv("UKM_SETOP_OFFS_OPS", "7")


@pytest.fixture(params=("1", "0"), ids=("xcd-order", "block-order"))
def order(request, monkeypatch):
    monkeypatch.setenv("UKM_SETOP_XCD_ORDER", request.param)
    return request.param


@pytest.fixture
def pair(lib, order):
    p = Pair(lib, *_sets())
    yield p
    p.close()


def test_shapes_are_what_the_cases_assume():
    want = {"256": (256, 256), "257": (257, 264), "257-one": (257, 264), "263": (263, 264), "264": (264, 264), "309": (309, 312)}
    for name, n in SHAPES.items():
        t = ntiles_of(n)
        assert (t, 8 * chunk_of(t)) == want[name]
        A, B = shape_sets(name)
        assert len(A) + len(B) == n
    assert SHAPES["257-one"] - 256 * TILE == 1
    A, B = _sets()
    assert len(A) + len(B) == SHAPES["309"]


@pytest.mark.parametrize("name", list(SHAPES))
def test_chunk_boundaries_straddle_a_matched_pair(name):
    """the union's offset of a chunk's FIRST tile carries the straddle term: chosen on the CPU so that it is exercised"""
    A, B = shape_sets(name)
    t = ntiles_of(len(A) + len(B))
    s = straddling(A, B)
    on_chunk = [int(b) for b in s if 0 < b < t and b % chunk_of(t) == 0]
    assert on_chunk, "no boundary t with t %% %d == 0 among the %d that straddle a matched pair" % (chunk_of(t), len(s))


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_shape_from_the_table(lib, order, name):
    """the first call searches and records the counts; union, inter and diff then run from the table"""
    A, B = shape_sets(name)
    p = Pair(lib, A, B)
    try:
        assert np.array_equal(p.run(OP_UNION), shape_ref(name, OP_UNION))
        assert counters(p) == (0, 0, 0, 0)
        for k, op in enumerate(OPS):
            p.out.fill_(SENT)
            want = shape_ref(name, op)
            assert np.array_equal(p.run(op), want)
            assert counters(p) == (k + 1, 0, k + 1, 0)
            assert bool((p.out[len(want):] == SENT).all())       # nothing behind the result
    finally:
        p.close()


def test_all_of_b_behind_all_of_a(lib, order):
    """the first chunks are tiles of A alone, the last ones of B alone, and one tile in between holds the end of A"""
    A, _ = shape_sets("257")
    nb = SHAPES["257"] - len(A)
    B = A[-1] + U64(1) + np.arange(nb, dtype=U64) * U64(3)
    p = Pair(lib, A, B)
    try:
        assert np.array_equal(p.run(OP_INTER), np.empty(0, dtype=U64))
        for op, want in ((OP_UNION, np.concatenate((A, B))), (OP_INTER, np.empty(0, dtype=U64)), (OP_DIFF, A)):
            assert np.array_equal(p.run(op), want)
        assert counters(p) == (3, 0, 3, 0)
        # ... and the other way round: every record of the intersection's and the difference's output from A's tiles
        assert np.array_equal(p.run(OP_DIFF, a=p.B, b=p.A), B)
        assert np.array_equal(p.run(OP_UNION, a=p.B, b=p.A), np.concatenate((A, B)))
        assert np.array_equal(p.run(OP_INTER, a=p.B, b=p.A), np.empty(0, dtype=U64))
        assert counters(p) == (5, 0, 5, 0)
    finally:
        p.close()


def test_counts_changed_partition_intact(pair):
    """matched keys of A raised in place: the table pass raises FLAG_OFFS, the look-back pass repairs it"""
    A, B = _sets()
    A2, _ = raised_matches(A, B)
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))
    pair.write(pair.A, A2)
    assert np.array_equal(pair.run(OP_INTER), _want(OP_INTER, A2, B))
    assert counters(pair) == (1, 0, 0, 1)                     # the partition held; the offsets did not
    assert np.array_equal(pair.run(OP_DIFF), _want(OP_DIFF, A2, B))
    assert counters(pair) == (2, 0, 1, 1)                     # the repeated pass left fresh counts: a hit again
    assert np.array_equal(pair.run(OP_UNION), _want(OP_UNION, A2, B))
    assert counters(pair) == (3, 0, 2, 1)


def test_stale_partition_runs_no_tile(pair):
    """the same key, other contents: STALE -> SEARCH.  The new intersection is empty, so a tile run from the bad table --
    whichever workgroup it was dealt to -- would be the only writer of the output buffer"""
    A, B = _sets()
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))
    assert np.array_equal(pair.run(OP_INTER), _ref(OP_INTER))
    assert counters(pair) == (1, 0, 1, 0)
    A2 = np.arange(1, len(A) + 1, dtype=U64)
    assert A2[-1] < B[0]
    pair.write(pair.A, A2)
    pair.out.fill_(SENT)
    got = pair.run(OP_INTER)
    assert len(got) == 0 and counters(pair) == (1, 1, 1, 0)
    assert bool((pair.out == SENT).all())
    assert np.array_equal(pair.run(OP_UNION), _want(OP_UNION, A2, B))     # the fresh table and counts serve the next calls
    assert np.array_equal(pair.run(OP_DIFF), A2)
    assert counters(pair) == (3, 1, 3, 0)


@pytest.mark.parametrize("op", OPS, ids=("union", "inter", "diff"))
def test_capacity_one_short(pair, lib, op):
    torch = pair.torch
    first = OP_INTER if op == OP_UNION else OP_UNION
    assert np.array_equal(pair.run(first), _ref(first))
    want = _ref(op)
    need = len(want)
    buf = torch.full((need + 4 * TILE,), SENT, dtype=torch.int64, device=pair.dev)
    with pytest.raises(lib.CapacityError) as e:
        pair.ctx.setop2(op, pair.A, pair.B, out=buf[:need - 1])
    assert e.value.needed == need
    assert counters(pair) == (1, 0, 1, 0)
    assert bool((buf[need - 1:] == SENT).all())                           # the guard words behind the capacity
    assert np.array_equal(pair.run(op), want)


UNION_MIN_TILES = 2048      # ukm_setops.hip: SETOP_OFFS_UNION_MIN_TILES


@pytest.mark.parametrize("ntiles", (UNION_MIN_TILES - 1, UNION_MIN_TILES))
def test_union_takes_the_table_from_the_threshold(lib, monkeypatch, ntiles):
    """the default plan on both sides of the threshold: below it the union of a cached pair keeps its look-back, from it
    upward it runs from the table (in XCD order, the default for the union); inter does at either size"""
    monkeypatch.delenv("UKM_SETOP_OFFS_OPS")
    monkeypatch.delenv("UKM_SETOP_XCD_ORDER", raising=False)
    n = ntiles * TILE - 17
    assert ntiles_of(n) == ntiles
    A, B = _sets(UNION_MIN_TILES * TILE // 2)             # (one pair of sets for both sizes)
    A, B = A[:n // 2], B[:n - n // 2]
    table = 1 if ntiles >= UNION_MIN_TILES else 0
    p = Pair(lib, A, B)
    try:
        # (2 x 1e7 codes: the oracle's own loops over every record, by value ranges in parallel)
        want = oracle_by_value_ranges(lambda ks, ts: _want(OP_UNION, *ks), [A, B])
        assert np.array_equal(p.run(OP_UNION), want)
        assert counters(p) == (0, 0, 0, 0)
        assert np.array_equal(p.run(OP_UNION), want)
        assert counters(p) == (1, 0, table, 0)
        assert np.array_equal(p.run(OP_INTER), oracle_by_value_ranges(lambda ks, ts: _want(OP_INTER, *ks), [A, B], kind="inter"))
        assert counters(p) == (2, 0, table + 1, 0)
    finally:
        p.close()


def test_default_policy_counters(lib, monkeypatch):
    """without UKM_SETOP_OFFS_OPS and with the order on: the union keeps its look-back, inter and diff run from the table"""
    monkeypatch.delenv("UKM_SETOP_OFFS_OPS")
    monkeypatch.setenv("UKM_SETOP_XCD_ORDER", "1")
    A, B = _sets()
    p = Pair(lib, A, B)
    try:
        for k, (op, offs) in enumerate(((OP_UNION, 0), (OP_INTER, 1), (OP_DIFF, 2), (OP_UNION, 2), (OP_INTER, 3))):
            assert np.array_equal(p.run(op), _ref(op))
            assert counters(p) == (k, 0, offs, 0)
        A2, _ = raised_matches(A, B)
        p.write(p.A, A2)
        assert np.array_equal(p.run(OP_UNION), _want(OP_UNION, A2, B))
        assert counters(p) == (5, 0, 3, 0)
        assert np.array_equal(p.run(OP_DIFF), _want(OP_DIFF, A2, B))
        assert counters(p) == (6, 0, 3, 1)
        assert np.array_equal(p.run(OP_INTER), _want(OP_INTER, A2, B))
        assert counters(p) == (7, 0, 4, 1)
    finally:
        p.close()
