"""Tile offsets from the cached match counts (ukm_setop_kernels.h: the TABLE instantiation of setop_tile_kernel; DESIGN.md
sections 4.1 and 4.12).  A plain-key union / inter / diff that hits the partition cache while the slot's match counts MP
are valid runs WITHOUT the look-back: its tiles' output offsets come from MP (inter MP[t], diff a_t - MP[t], union
d_t - MP[t] + s_t), every tile checks its own count against its step of the table, and a pass that finds a difference
runs again with the look-back.  The contract is the partition cache's: results never depend on the cache, only time does.

Every case goes through the C ABI on device-resident buffers and compares element for element with the CPU oracle; the
statistics "setop_offs_hits" / "setop_offs_stale" (beside "setop_part_hits" / "setop_part_stale") say which way a call
went.  Fixture, sizes and helpers are those of test_gpu_part_reuse.py: |A| = |B| = 1.5e6, 309 plain tiles.

By default the union keeps its look-back (it gained nothing from the table at 2 x 1e9: profiles/offs_reuse_notes.md) and
only inter and diff take their offsets from the counts.  The cases here run with UKM_SETOP_OFFS_OPS=7 -- all three operations
from the table, the union's straddle term included -- except test_default_policy.
"""
import itertools

import numpy as np
import pytest

from test_gpu_part_reuse import (OP_DIFF, OP_INTER, OP_UNION, SEED, TILE, U32, U64, Pair, _oracle, _ref, _sets, _want,
                                 merge_path)
from conftest import splitmix64

pytestmark = pytest.mark.gpu

OPS = (OP_UNION, OP_INTER, OP_DIFF)


@pytest.fixture(scope="module")
def lib():
    from unikmer_amd import lib as L
    return L


@pytest.fixture(autouse=True)
def all_three_operations_from_the_table(monkeypatch):
    monkeypatch.setenv("UKM_SETOP_OFFS_OPS", "7")


@pytest.fixture
def pair(lib):
    p = Pair(lib, *_sets())
    yield p
    p.close()


def counters(p):
    """(partition hits, partition stale, offset hits, offset stale)"""
    return (p.ctx.stat("setop_part_hits"), p.ctx.stat("setop_part_stale"), p.ctx.stat("setop_offs_hits"),
            p.ctx.stat("setop_offs_stale"))


def boundaries(A, B):
    """(mp, d): the merge-path split and the diagonal of every tile boundary"""
    mp = merge_path(A, B, TILE).astype(np.int64)
    n = len(A) + len(B)
    d = np.minimum(np.arange(len(mp), dtype=np.int64) * TILE, n)
    return mp, d


def straddling(A, B):
    """boundaries t with A[a_t - 1] == B[b_t]: a matched pair whose A record is the last of a tile and whose B record the
    first of the next one"""
    mp, d = boundaries(A, B)
    b = d - mp
    ok = (mp > 0) & (b < len(B))
    s = np.zeros(len(mp), dtype=bool)
    s[ok] = A[mp[ok] - 1] == B[b[ok]]
    return np.nonzero(s)[0]


def raised_matches(A, B, how_many=300):
    """A with `how_many` of its matched keys raised by one in place: keys strictly inside tiles (their place in the merged
    order is at least 8 records from a boundary) whose raised value is in neither set"""
    jb = np.searchsorted(B, A, side="left")
    matched = (jb < len(B)) & (B[np.minimum(jb, len(B) - 1)] == A)
    pos = np.arange(len(A), dtype=np.int64) + jb          # A before B on ties
    inside = (pos % TILE >= 8) & (pos % TILE < TILE - 8)
    up = A + U64(1)
    jb1 = np.searchsorted(B, up, side="left")
    free = B[np.minimum(jb1, len(B) - 1)] != up
    free[:-1] &= up[:-1] < A[1:]
    cand = np.nonzero(matched & inside & free)[0]
    assert len(cand) >= how_many
    pick = cand[np.linspace(0, len(cand) - 1, how_many).astype(np.int64)]
    A2 = A.copy()
    A2[pick] += U64(1)
    assert np.all(A2[1:] > A2[:-1])
    return A2, pick


def test_three_operations_one_look_back(pair):
    """union, inter, diff in turn on a fresh context: one search and one look-back pass, two passes from the table"""
    assert counters(pair) == (0, 0, 0, 0)
    for op in OPS:
        assert np.array_equal(pair.run(op), _ref(op))
    assert counters(pair) == (2, 0, 2, 0)


def test_default_policy(pair, monkeypatch):
    """without the knob: the union records the counts like any other pass but always runs with the look-back itself"""
    monkeypatch.delenv("UKM_SETOP_OFFS_OPS")
    for k, (op, offs) in enumerate(((OP_UNION, 0), (OP_INTER, 1), (OP_DIFF, 2), (OP_UNION, 2), (OP_INTER, 3))):
        assert np.array_equal(pair.run(op), _ref(op))
        assert counters(pair) == (k, 0, offs, 0)
    A, B = _sets()
    A2, _ = raised_matches(A, B)
    pair.write(pair.A, A2)
    assert np.array_equal(pair.run(OP_UNION), _want(OP_UNION, A2, B))     # (the look-back notices nothing, and need not)
    assert counters(pair) == (5, 0, 3, 0)
    assert np.array_equal(pair.run(OP_DIFF), _want(OP_DIFF, A2, B))
    assert counters(pair) == (6, 0, 3, 1)
    assert np.array_equal(pair.run(OP_INTER), _want(OP_INTER, A2, B))
    assert counters(pair) == (7, 0, 4, 1)


def test_fixture_has_straddling_matches():
    A, B = _sets()
    s = straddling(A, B)
    ntiles = (len(A) + len(B) + TILE - 1) // TILE
    assert len(s) >= 10, "%d of %d boundaries straddle a matched pair" % (len(s), ntiles)


@pytest.mark.parametrize("order", list(itertools.permutations(OPS)), ids=lambda o: "".join("UID"[op] for op in o))
def test_every_first_operation(lib, order):
    """whichever operation records the counts, the other two -- and then the first itself -- are right from the table
    (the union's offsets need the straddle term of a quarter of the boundaries)"""
    p = Pair(lib, *_sets())
    try:
        for op in order + (order[0],):
            assert np.array_equal(p.run(op), _ref(op))
        assert counters(p) == (3, 0, 3, 0)
    finally:
        p.close()


def test_counts_changed_partition_intact(pair):
    A, B = _sets()
    A2, pick = raised_matches(A, B)
    assert np.array_equal(merge_path(A2, B, TILE), merge_path(A, B, TILE))
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))
    pair.write(pair.A, A2)
    assert np.array_equal(pair.run(OP_INTER), _want(OP_INTER, A2, B))
    assert counters(pair) == (1, 0, 0, 1)                     # the partition held; the offsets did not
    assert np.array_equal(pair.run(OP_DIFF), _want(OP_DIFF, A2, B))
    assert counters(pair) == (2, 0, 1, 1)                     # the repeated pass left fresh counts: a hit again
    assert np.array_equal(pair.run(OP_UNION), _want(OP_UNION, A2, B))
    assert counters(pair) == (3, 0, 2, 1)


def test_back_off_after_two_offset_stale_passes_in_a_row(pair):
    A, B = _sets()
    A2, _ = raised_matches(A, B)
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))
    pair.write(pair.A, A2)
    assert np.array_equal(pair.run(OP_UNION), _want(OP_UNION, A2, B))
    assert counters(pair) == (1, 0, 0, 1)
    pair.write(pair.A, A)
    assert np.array_equal(pair.run(OP_DIFF), _ref(OP_DIFF))
    assert counters(pair) == (2, 0, 0, 2)
    for k, op in enumerate(OPS):                              # unchanged inputs: would hit, but nobody tries
        assert np.array_equal(pair.run(op), _ref(op))
        assert counters(pair) == (3 + k, 0, 0, 2)             # (the partition cache itself goes on)
    pair.write(pair.A, A2)
    assert np.array_equal(pair.run(OP_INTER), _want(OP_INTER, A2, B))
    assert counters(pair) == (6, 0, 0, 2)


@pytest.mark.parametrize("op", OPS, ids=("union", "inter", "diff"))
def test_capacity_on_a_table_pass(pair, lib, op):
    torch = pair.torch
    first = OP_INTER if op == OP_UNION else OP_UNION
    assert np.array_equal(pair.run(first), _ref(first))
    need = len(_ref(op))
    SENT = -0x5A5A5A5A5A5A5A5B
    for k, cap in enumerate((need - 1, need // 2, 0)):
        buf = torch.full((need + 4 * TILE,), SENT, dtype=torch.int64, device=pair.dev)
        with pytest.raises(lib.CapacityError) as e:
            if cap:
                pair.ctx.setop2(op, pair.A, pair.B, out=buf[:cap])
            else:   # the size query: NULL output, out_cap 0
                n = lib.C.c_uint64()
                lib._check(pair.ctx.L.ukm_setop2(pair.ctx.h, op, pair.A.data_ptr(), None, len(pair.A), pair.B.data_ptr(), None,
                                                 len(pair.B), 0, None, None, 0, lib.C.byref(n)), n.value)
        assert e.value.needed == need
        assert counters(pair) == (k + 1, 0, k + 1, 0)
        assert bool((buf[cap:] == SENT).all())
    assert np.array_equal(pair.run(op), _ref(op))


def test_duplicates_written_in_place(pair):
    """the table pass sees the duplicates like any other: the result comes from the re-run on (code, rank) pairs"""
    A, B = _sets()
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))
    A2 = A.copy()
    A2[7::7] = A2[6::7][:len(A2[7::7])]            # every seventh code twice ...
    i = np.arange(21, len(A2) - 1, 21)
    A2[i + 1] = A2[i] = A2[i - 1]                  # ... and runs of three and more
    assert np.all(A2[1:] >= A2[:-1]) and np.any(A2[1:] == A2[:-1])
    pair.write(pair.A, A2)
    for op in (OP_INTER, OP_DIFF, OP_UNION, OP_INTER):
        assert np.array_equal(pair.run(op), _want(op, A2, B))
    pair.write(pair.A, A)
    for op in OPS + OPS:
        assert np.array_equal(pair.run(op), _ref(op))


def test_unsorted_stretch_written_in_place(pair, lib):
    A, B = _sets()
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))
    A2 = A.copy()
    A2[len(A) // 2: len(A) // 2 + 20_000] = A2[len(A) // 2: len(A) // 2 + 20_000][::-1].copy()   # two tiles' worth, reversed
    pair.write(pair.A, A2)
    for op in (OP_INTER, OP_DIFF):
        with pytest.raises(lib.UnsortedError):
            pair.run(op)
    pair.write(pair.A, A)
    for op in OPS + OPS:
        assert np.array_equal(pair.run(op), _ref(op))
    assert counters(pair)[3] == 0                  # (disorder beside a wrong count: no second pass, the call fails anyway)


def test_ticketed_look_back_beside_the_table(lib, monkeypatch):
    """UKM_FORCE_TICKET=1: the look-back passes take their tile ids from the counter; the table passes have none to take"""
    monkeypatch.setenv("UKM_FORCE_TICKET", "1")
    A, B = _sets()
    p = Pair(lib, A, B)
    try:
        for op in OPS:
            assert np.array_equal(p.run(op), _ref(op))
        assert counters(p) == (2, 0, 2, 0)
        A2, _ = raised_matches(A, B)
        p.write(p.A, A2)
        assert np.array_equal(p.run(OP_UNION), _want(OP_UNION, A2, B))
        assert counters(p) == (3, 0, 2, 1)
        assert np.array_equal(p.run(OP_DIFF), _want(OP_DIFF, A2, B))
        assert counters(p) == (4, 0, 3, 1)
    finally:
        p.close()


def test_knob_turns_offset_reuse_off(pair, monkeypatch):
    monkeypatch.setenv("UKM_SETOP_OFFS_REUSE", "0")
    for op in OPS + OPS:
        assert np.array_equal(pair.run(op), _ref(op))
    assert counters(pair) == (5, 0, 0, 0)
    monkeypatch.delenv("UKM_SETOP_OFFS_REUSE")
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))    # (the calls above recorded nothing: this one does)
    assert counters(pair) == (6, 0, 0, 0)
    assert np.array_equal(pair.run(OP_INTER), _ref(OP_INTER))
    assert counters(pair) == (7, 0, 1, 0)


def test_taxid_calls_never_use_the_table(pair):
    """per-record taxids run on tiles of their own size, one taxid per file on the plain tiles with the taxid epilogue:
    neither is a plain-key pass"""
    O, tax, child, parent = _oracle()
    A, B = _sets()
    T = len(child)
    ta = (U64(1) + splitmix64(U64(SEED + 2) ^ A) % U64(T)).astype(U32)
    tb = (U64(1) + splitmix64(U64(SEED + 3) ^ B) % U64(T)).astype(U32)
    pair.ctx.taxonomy_load(child, parent)
    dta, dtb = pair.up(ta, np.int32), pair.up(tb, np.int32)
    fa, fb = int(T - 3), int(T - 700)
    outt = pair.torch.empty(len(A) + len(B), dtype=pair.torch.int32, device=pair.dev)
    assert np.array_equal(pair.run(OP_UNION), _ref(OP_UNION))      # valid counts in the slot
    for op, fn in ((OP_UNION, O.union), (OP_INTER, O.inter), (OP_DIFF, O.diff)):
        wk, wt = fn([A, B], [np.full(len(A), fa, U32), np.full(len(B), fb, U32)], tax)
        gk, gt = pair.run(op, a_taxids=fa, b_taxids=fb, out_taxids=outt)
        assert np.array_equal(gk, wk) and np.array_equal(gt, wt)
    assert counters(pair)[1:] == (0, 0, 0) and counters(pair)[0] == 3
    assert np.array_equal(pair.run(OP_INTER), _ref(OP_INTER))      # ... which a plain call behind them still finds
    assert counters(pair) == (4, 0, 1, 0)
    for op, fn in ((OP_UNION, O.union), (OP_INTER, O.inter), (OP_DIFF, O.diff)):
        wk, wt = fn([A, B], [ta, tb], tax)
        gk, gt = pair.run(op, a_taxids=dta, b_taxids=dtb, out_taxids=outt)
        assert np.array_equal(gk, wk) and np.array_equal(gt, wt)
    assert counters(pair)[2:] == (1, 0)
    for op in OPS:
        assert np.array_equal(pair.run(op), _ref(op))
    assert counters(pair)[3] == 0
