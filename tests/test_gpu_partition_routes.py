"""Every route into the merge-path partition of the 2-way set operation (ukm_setops.hip), at the
smallest shapes that reach it: the single-level wave kernel, the fused kernel, the coarse wave kernel + the fine kernel
(UKM_SETOP_FUSED_PART=0, and a chained link of many tiles), with and without ranks.

A tile is 512 x 19 = 9728 merged records of plain keys, 512 x 12 = 6144 with ranks; the fused and the two-level partition
start at 4 * PART_COARSE = 256 tiles, a chained link goes two-level at 2048.  Inputs are arithmetic progressions (no
sorting on the host); expected values come from numpy for sets and from the CPU oracle for multisets and folds.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U64 = np.uint64
TILE = 512 * 19
TILE_RANK = 512 * 12
MIN_TILES = 4 * 64            # 4 * PART_COARSE
LINK_TWO_LEVEL_TILES = 2048   # SETOP_LINK_SMALL_TILES
FOLD_MAX_FIRST = 1 << 24      # ukm_nway.hip: a larger first file goes to the chained links, not to the range fold
OP_UNION, OP_INTER, OP_DIFF = 0, 1, 2

SINGLE = [1, TILE, TILE + 1, (MIN_TILES - 1) * TILE]
TWO_LEVEL = [MIN_TILES * TILE, MIN_TILES * TILE + 1, 2_515_000]
RATIOS = [1, 1000]


@functools.lru_cache(None)
def _sets(total, ratio):
    """two sorted sets, |A| + |B| = total, |A| : |B| = 1 : ratio; every 5th (1 : 1000: every 3rd) record of A is in B, and at
    1 : 1000 A's few records are spread over the whole of B's range"""
    na = max(total // (1 + ratio), 1) if total > 1 else 1
    nb = total - na
    step = 3 * ratio + (1 if ratio > 1 else 0)       # (3, or 3001: about `ratio` records of B between two of A)
    A = np.arange(na, dtype=U64) * U64(step) + U64(10)
    B = np.arange(nb, dtype=U64) * U64(5 if ratio == 1 else 3) + U64(10)
    return A, B


@functools.lru_cache(None)
def _want(total, ratio):
    A, B = _sets(total, ratio)
    return {OP_UNION: np.union1d(A, B), OP_INTER: np.intersect1d(A, B, assume_unique=True),
            OP_DIFF: np.setdiff1d(A, B, assume_unique=True)}


@pytest.fixture(scope="module")
def lib():
    from unikmer_amd import lib as L
    return L


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ctx(lib):
    import torch
    c = lib.Context(0, stream=torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream)
    yield c
    c.close()


def _up(x):
    import torch
    return torch.from_numpy(x.view(np.int64)).to(torch.device("cuda", 0))


def _check_all_ops(ctx, total, ratio):
    """union, inter and diff of one pair on device buffers (what the partition cache needs to be eligible)"""
    A, B = _sets(total, ratio)
    assert len(A) + len(B) == total
    dA, dB = _up(A), _up(B)
    want = _want(total, ratio)
    stale = ctx.stat("setop_part_stale")
    for op in (OP_UNION, OP_INTER, OP_DIFF):
        got = ctx.setop2(op, dA, dB).cpu().numpy().view(U64)
        assert np.array_equal(got, want[op]), (total, ratio, op)
    assert ctx.stat("setop_part_stale") == stale     # (a table the search has just made holds at every boundary)


def test_shapes_are_what_the_cases_assume():
    tiles = lambda n, tile=TILE: (n + tile - 1) // tile
    assert [tiles(n) for n in SINGLE] == [1, 1, 2, MIN_TILES - 1]
    assert [tiles(n) for n in TWO_LEVEL] == [MIN_TILES, MIN_TILES + 1, MIN_TILES + 3]
    assert tiles(2_515_000, TILE_RANK) == 410
    for total in TWO_LEVEL:
        A, B = _sets(total, 1000)
        assert len(B) > 900 * len(A) and A[-1] > B[-1] // 2 and len(np.intersect1d(A, B)) > len(A) // 10
        A, B = _sets(total, 1)
        assert abs(len(A) - len(B)) <= 1 and len(np.intersect1d(A, B)) > len(A) // 10


@pytest.mark.parametrize("total", SINGLE)
def test_single_level(ctx, total):
    """below 256 tiles: one wave per boundary, every boundary searched over the whole inputs"""
    hits = ctx.stat("setop_part_hits")
    _check_all_ops(ctx, total, 1)
    assert ctx.stat("setop_part_hits") == hits       # (no cache below the threshold)


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("total", TWO_LEVEL)
def test_fused(ctx, total, ratio):
    """from 256 tiles: a workgroup per coarse segment -- a last segment that ends on the last diagonal, one of one tile, one
    of three; at 1 : 1000 the legal range of most diagonals is cut by |A|.  The union searches; inter and diff verify its
    table boundary by boundary (the partition cache)."""
    hits = ctx.stat("setop_part_hits")
    _check_all_ops(ctx, total, ratio)
    assert ctx.stat("setop_part_hits") == hits + 2


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("total", TWO_LEVEL)
def test_two_level_without_the_fused_kernel(ctx, total, ratio, monkeypatch):
    """UKM_SETOP_FUSED_PART=0: the coarse wave kernel and the fine kernel, and no partition cache"""
    monkeypatch.setenv("UKM_SETOP_FUSED_PART", "0")
    hits = ctx.stat("setop_part_hits")
    _check_all_ops(ctx, total, ratio)
    assert ctx.stat("setop_part_hits") == hits


@functools.lru_cache(None)
def _multisets():
    """the 1 : 1 pair of 2 515 000 records less two runs, with a run of one value inserted into each: 4 and 3 rank tiles long"""
    ra, rb = 4 * TILE_RANK + 100, 3 * TILE_RANK + 7
    A, B = _sets(2_515_000 - ra - rb, 1)
    v = A[len(A) // 2 // 5 * 5]
    assert v == B[np.searchsorted(B, v)]            # the value is in both sets
    A = np.insert(A, np.searchsorted(A, v), np.full(ra, v, U64))
    B = np.insert(B, np.searchsorted(B, v), np.full(rb, v, U64))
    assert len(A) + len(B) == 2_515_000
    return A, B


@pytest.mark.parametrize("fused", ["1", "0"])
def test_ranks(ctx, O, fused, monkeypatch):
    """multisets: inter and diff run again on (code, rank) pairs, 410 tiles -- through the fused kernel, and through the
    coarse and fine kernels"""
    monkeypatch.setenv("UKM_SETOP_FUSED_PART", fused)
    A, B = _multisets()
    assert np.array_equal(ctx.setop2(OP_INTER, A, B), O.inter([A, B]))
    assert np.array_equal(ctx.setop2(OP_DIFF, A, B), O.diff([A, B]))


@functools.lru_cache(None)
def _chain():
    """a first file of 2049 plain tiles (with the second one), too large for the range fold; three later files of a few
    thousand records each"""
    n0 = LINK_TWO_LEVEL_TILES * TILE
    first = np.arange(n0, dtype=U64) * U64(3) + U64(10)
    later = [np.arange(4000 + 500 * i, dtype=U64) * U64(3000 + 1500 * i) + U64(10) for i in range(3)]   # (in all: 10 + 18000 m)
    assert n0 > FOLD_MAX_FIRST and (n0 + len(later[0]) + TILE - 1) // TILE > LINK_TWO_LEVEL_TILES
    assert all(x[-1] < first[-1] for x in later)
    return [first] + later


@pytest.mark.parametrize("op", ["inter", "diff"])
def test_chained_links_two_level(ctx, O, op):
    """inter / diff over four files whose first is too large for the range fold: one link per file, each with the first
    file's size as its bound -- the coarse and fine kernels with |A| read on the device (after an inter: a few records)"""
    ss = _chain()
    got = getattr(ctx, op)(ss)
    assert np.array_equal(got, getattr(O, op)(ss))
    assert 0 < len(got) < len(ss[0])


def test_chained_links_single_level(ctx, O, monkeypatch):
    """the same fold with a first file of four tiles and the range fold off: every link through the single-level wave kernel, which
    also clears the link's status lines"""
    monkeypatch.setenv("UKM_NO_FOLD", "1")
    ss = [x[:3 * TILE + 5] if i == 0 else x for i, x in enumerate(_chain())]
    for op in ("inter", "diff"):
        got = getattr(ctx, op)(ss)
        assert np.array_equal(got, getattr(O, op)(ss))
        assert 0 < len(got) < len(ss[0])
