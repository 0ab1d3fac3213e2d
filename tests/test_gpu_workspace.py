"""No call may depend on what the workspace arena held before it.

Every kernel family takes its control words -- look-back status lines, ticket counters, result and flag words, histograms,
bucket counters, miss lists -- from the context's arena (ws_alloc), and a call is right only if each word is initialised
before its first read.  A block fresh from hipMalloc is usually zero, and ws_reset_top hands the next call the same block
at the same offsets, so a forgotten clear reads the plausible leftovers of an identical earlier call: no test that runs
on one warmed context can see it.  Option "ws_poison"  fills every arena block with one byte before each
top-level call and whenever a block is created.  This module runs

  - the whole case table of test_gpu_capacity.py (one case per entry point, pinned route and taxid form; the oracle's
    arrays bit for bit through attempt(), which also checks the guards, last_route() and the case's verify) under the
    four patterns, in a fresh context, after reserve / trim / a failed call, and ticketed,
  - the shapes that table lacks: ukm_setop2 at 256 tiles and more (the fused and the un-fused two-level partition), the
    sort's host-histogram, bucket and fused-histogram routes, the k-way merge at fan-in 4 / 8 / 16, ukm_lca,
    ukm_partition_points; each also as a STALE TWIN (the same call on other values of identical
    lengths first, poisoning off: the first call's control words and partition points are in place at the same addresses
    and are wrong for the second); ukm_shard_splitters on one rank, which can only show that it runs,
  - the context plumbing that changes where work runs: pinned memory and the transfer stream, a borrowed stream.

Every shape that is meant to reach a path has a CPU-only twin that evaluates the reference alone and asserts from the
sources' constants (the table below) that the shape gets there.
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

from conftest import splitmix64, synth_tree
from test_gpu_capacity import (CASES, NAMES, TILED, Case, attempt, SEED, U32, U64, OP_UNION, OP_INTER, OP_DIFF, PLAIN, UNIQUE,
                               ROUTE_KWAY, TILE_SETOP, TILE_SETOP_TAX, TILE_SETOP_RANK, _oracle, _universe, _taxids, _dup,
                               _big_merge, _stable, _o2, _kt)

# ---- constants of the sources -----------------------------------------------------------------------------------------------
PART_COARSE = 64                    # ukm_setop_part.h: SETOP_PART_COARSE; two-level partition from 4 x PART_COARSE tiles
TWO_LEVEL_TILES = 4 * PART_COARSE
SORT_LOCAL_MIN = 1 << 23            # ukm_sort_plan.h: the bucket route from this n (key_bits >= 32, option sort_local not 0)
SORT_FUSED_MIN = 1 << 24            #               the fused-histogram general route from this n; below: host histograms
LS_TOP_MIN, LS_BUCKET_AVG = 12, 1400  #             ls_plan: the smallest top-bit count with n >> topb <= 1400 (topb <= 16 here)
LS_CLASS_MAX = 256 * 16             #               LS_NT x the largest LS_CLASS_KPT: a bucket beyond it is oversized
LS_MAX_BIG = 8192                   #               oversized buckets the route gathers; more, or more than n / 4 keys: it gives up
KWAY_TOP2_MIN = 1 << 20             # ukm_kway.hip: a merge's two-child top level runs through the 2-way tile kernel from this N
PATTERNS = (0x00, 0x55, 0xAA, 0xFF)
MB = 1 << 20


def ls_topb(n):
    """ls_plan of ukm_sort_plan.h for n < 2^27"""
    assert (n >> 16) <= 2048
    topb = LS_TOP_MIN
    while topb < 16 and (n >> topb) > LS_BUCKET_AVG:
        topb += 1
    return topb


# ---- contexts and states --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    from unikmer_amd import lib as L
    ctx = L.Context(0)
    ctx.taxonomy_load(*synth_tree(5, 8))
    yield ctx, L
    ctx.close()


@contextlib.contextmanager
def options(ctx, opts):
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        yield
    finally:
        for k in opts:
            ctx.set_option(k, None)


def poisoned(ctx):
    """after a call with ws_poison set: the hook ran, over everything the context holds"""
    filled, held = ctx.stat("ws_poisoned_bytes"), ctx.stat("workspace_bytes")
    assert filled >= held > 0, "ws_poison filled %d bytes of a workspace of %d" % (filled, held)


def patterns(ctx, call):
    for byte in PATTERNS:
        with options(ctx, {"ws_poison": byte}):
            call()
            poisoned(ctx)


def stale_twin(ctx, other, real, reserve):
    """one reserved block, the same call on other values of identical lengths, then the real data, poisoning off"""
    assert ctx.get_option("ws_poison") is None
    ctx.trim()
    ctx.reserve(reserve)
    other()
    real()
    assert ctx.stat("workspace_blocks") == 1 and ctx.stat("workspace_bytes") == reserve, "the arena grew: not the same addresses"


def run_case(ctx, L, case, place="device", extra=None):
    with options(ctx, dict(case.opts, **(extra or {}))):
        attempt(ctx, L, case, len(case.expected()[0]), place)


# ---- 2. the case table under every workspace state ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_patterns(env, name):
    """0x00 is what a fresh block usually holds; in a look-back status word 0xAA decodes as LB_INCL | garbage (a finished
    prefix that is wrong), 0x55 as LB_AGG | garbage (a published aggregate that is wrong); 0xFF is the probe tables' empty
    mark, a full ticket counter and the k-way merge's padding key"""
    ctx, L = env
    case = CASES[name]
    patterns(ctx, lambda: run_case(ctx, L, case))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_fresh_context(name):
    """A new context per case, host outputs: inputs and outputs are staged through the arena, which is created inside the
    call, block by block, every block poisoned before it is handed out.  Every case stages at least its outputs, so the
    arena of every case grows inside the call (152 of 152 on the MI355X), which is asserted."""
    from unikmer_amd import lib as L
    case = CASES[name]
    ctx = L.Context(0)
    try:
        ctx.taxonomy_load(*synth_tree(5, 8))
        before = ctx.stat("workspace_blocks")
        with options(ctx, dict(case.opts, ws_poison=0xAA)):
            attempt(ctx, L, case, len(case.expected()[0]), "host")
            poisoned(ctx)
        assert ctx.stat("workspace_blocks") > before == 0, "the call created no block: nothing was staged through the arena"
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", TILED)
def test_after_reserve_trim_and_failed_call(env, name):
    """the tiled launches keep control words alive across a retry: after a reserve (one large poisoned block), after a trim
    (the next call builds the arena anew) and straight after a call that failed at out_cap = 1"""
    ctx, L = env
    case = CASES[name]
    need = len(case.expected()[0])
    with options(ctx, dict(case.opts, ws_poison=0xAA)):
        ctx.reserve(256 * MB)
        assert ctx.stat("workspace_bytes") >= 256 * MB
        attempt(ctx, L, case, need, "device")
        poisoned(ctx)
        ctx.trim()
        assert ctx.stat("workspace_bytes") == 0 and ctx.stat("workspace_blocks") == 0
        attempt(ctx, L, case, need, "device")
        poisoned(ctx)
        attempt(ctx, L, case, 1, "device")       # (asserts UKM_ERR_CAPACITY with the size that is needed)
        attempt(ctx, L, case, need, "device")
        poisoned(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TILED)
def test_ticketed(env, name):
    """the ticketed instantiations read the ticket counter out of the same head"""
    ctx, L = env
    with options(ctx, {"ws_poison": 0xAA}):
        run_case(ctx, L, CASES[name], extra={"force_ticket": 1})
        poisoned(ctx)


@pytest.mark.gpu
def test_poison_option_values_and_statistics():
    from unikmer_amd import lib as L
    ctx = L.Context(0)
    try:
        assert ctx.get_option("ws_poison") is None
        assert ctx.stat("workspace_blocks") == 0 and ctx.stat("ws_poisoned_bytes") == 0
        for bad in (-1, 256):
            with pytest.raises(L.UkmError) as e:
                ctx.set_option("ws_poison", bad)
            assert e.value.code == L.ERR_INVALID and ctx.get_option("ws_poison") is None
        x = np.arange(1000, dtype=U64)
        assert np.array_equal(ctx.setop2(OP_INTER, x, x), x)
        assert ctx.stat("ws_poisoned_bytes") == 0 and ctx.stat("workspace_blocks") == 1     # unset: nothing is filled
        ctx.set_option("ws_poison", 0xAA)
        assert ctx.get_option("ws_poison") == 0xAA
        assert np.array_equal(ctx.setop2(OP_INTER, x, x), x)
        assert ctx.stat("ws_poisoned_bytes") == ctx.stat("workspace_bytes") > 0
        ctx.reserve(200 * MB)                      # a block it creates is filled, and counted on top of the last call's
        assert ctx.stat("workspace_bytes") == 200 * MB and ctx.stat("ws_poisoned_bytes") == (64 + 200) * MB
        assert np.array_equal(ctx.setop2(OP_INTER, x, x), x)
        assert ctx.stat("ws_poisoned_bytes") == 200 * MB
        ctx.set_option("ws_poison", None)
        assert np.array_equal(ctx.setop2(OP_INTER, x, x), x)
        assert ctx.stat("ws_poisoned_bytes") == 200 * MB                                  # (the last call that filled)
    finally:
        ctx.close()


# ---- 3a. ukm_setop2 at 256 tiles and more ----------------------------------------------------------------------------------------
BIG_SET = 1_300_000           # records a side: both sets are cut to this length, so that the twin has the same lengths
BIG_UNIVERSE = {4: 1_740_000, 3: 1_960_000}     # three quarters / two thirds of it in each set: BIG_SET and a few thousand


def _big_sets(form, seed):
    """The real data (seed SEED) as _sets() of the capacity module: a quarter of the universe only in A, a quarter only
    in B, half in both.  Any other seed, the stale twin: another universe, and a third each only in A, only in B and in
    both -- sets of the same lengths whose records interleave differently and that share fewer codes, so that
    partition points, the tiles' output counts and every look-back prefix differ from the real call's."""
    parts = 4 if seed == SEED else 3
    U = _universe(BIG_UNIVERSE[parts], 22, seed)
    m = splitmix64(U64(seed + 1) ^ np.arange(len(U), dtype=U64)) % U64(parts)
    A, B = U[(m == 0) | (m >= 2)][:BIG_SET], U[(m == 1) | (m >= 2)][:BIG_SET]
    assert len(A) == len(B) == BIG_SET
    if form == "dup":
        A, B = _dup(A), _dup(B)
    ta = tb = None
    if form == "rec":
        ta, tb = _taxids(A ^ np.arange(len(A), dtype=U64), 1), _taxids(B ^ np.arange(len(B), dtype=U64), 2)
    return A, B, ta, tb


@functools.lru_cache(None)
def big_setop(op, form, seed=SEED):
    def expect(O, tax, A, B, ta, tb):
        tl = None if ta is None else [ta, tb]
        return (O.union, O.inter, O.diff)[op]([A, B], tl, tax)
    return Case("big-setop2-%s-%s-%x" % (("union", "inter", "diff")[op], form, seed), data=lambda: _big_sets(form, seed),
                call=lambda ctx, L, outs, A, B, ta, tb: ctx.setop2(op, A, B, ta, tb, **_o2(outs)), expect=expect,
                bound=lambda A, B, ta, tb: len(A) + len(B) if op == OP_UNION else len(A), dtypes=_kt(form == "rec"))


BIG_FORMS = ("plain", "rec", "dup")   # dup: the multiset re-run with ranks (VT_RANK = 12), after a folded first pass for union
BIG_OPS = (OP_UNION, OP_INTER, OP_DIFF)


def _tile_counts(A, B, tile):
    """(records of B below every record of A, records of A in front of every tile's diagonal = the merge-path partition
    points, distinct codes in every `tile` merged records = the union's per-tile output counts)"""
    both = np.concatenate([A, B])
    order = np.argsort(both, kind="stable")        # (A first on ties, as the merge path has it)
    merged = both[order]
    from_a = np.concatenate([[0], np.cumsum(order < len(A))])
    first = np.concatenate([[0], np.cumsum(np.concatenate([[True], merged[1:] != merged[:-1]]))])
    diags = np.minimum(np.arange(0, len(merged) + tile, tile), len(merged))
    return np.searchsorted(B, A, side="left"), from_a[diags], np.diff(first[diags])


@pytest.mark.parametrize("form", BIG_FORMS)
def test_big_setop2_oracle_only(form):
    """no GPU: whatever tile the route takes (19, 12 or 7 records per thread), both sets together span the two-level
    partition's 4 x PART_COARSE tiles -- before and, for the multiset form, after its duplicates are folded.  The stale
    twin's other values have the same lengths but interleave differently: the cross ranks of the two sets differ, and so
    does the number of output records of every tile and every prefix of them, for every tile size, so a partition table, a status line or a
    prefix left over from the twin is a WRONG one for the real call"""
    assert TILE_SETOP == max(TILE_SETOP, TILE_SETOP_TAX, TILE_SETOP_RANK)
    A, B, ta, tb = big_setop(OP_UNION, form).data()
    A2, B2, _, _ = big_setop(OP_UNION, form, SEED + 99).data()
    assert (len(A2), len(B2)) == (len(A), len(B)) and not np.array_equal(A, A2)
    for tile in (TILE_SETOP, TILE_SETOP_RANK, TILE_SETOP_TAX):
        (rank, mp, per_tile), (rank2, mp2, per_tile2) = _tile_counts(A, B, tile), _tile_counts(A2, B2, tile)
        # Both pairs of sets are equally dense, so both merge paths follow the diagonal and differ by the noise of the
        # memberships only: some hundreds of records at a diagonal a million records in, so that a cross rank or a
        # partition point of the twin equals the real one about once in some hundreds -- nine in ten must differ
        assert (rank != rank2).mean() > 0.9 and (mp != mp2)[1:-1].mean() > 0.9, (form, tile)
        assert len(per_tile) == len(per_tile2) >= TWO_LEVEL_TILES and (per_tile != per_tile2)[:-1].all(), (form, tile)
        assert (np.cumsum(per_tile) != np.cumsum(per_tile2)).all(), (form, tile)
    for x, y in ((A, B), (np.unique(A), np.unique(B))):
        assert len(x) + len(y) >= TWO_LEVEL_TILES * TILE_SETOP, (form, len(x), len(y))
    assert (len(np.unique(A)) < len(A)) == (form == "dup")
    for op in BIG_OPS:
        c = big_setop(op, form)
        exp = c.expected()
        assert 2 <= len(exp[0]) <= c.bound and all(len(e) == len(exp[0]) for e in exp)
        assert np.all(exp[0][1:] >= exp[0][:-1]) and (form == "dup" or np.all(exp[0][1:] > exp[0][:-1]))   # (inter keeps a multiset's copies)


@pytest.mark.gpu
@pytest.mark.parametrize("ticket", [0, 1])
@pytest.mark.parametrize("fused", [None, 0])
@pytest.mark.parametrize("form", BIG_FORMS)
@pytest.mark.parametrize("op", BIG_OPS)
def test_big_setop2(env, op, form, fused, ticket):
    """fused unset: setop_partition_fused_kernel clears the head and word 0 of every status line itself and the first
    attempt skips ukm_lb_ctl_zero; fused = 0: the memset and the un-fused two-level partition.  Which partition ran is
    not observable from the host (there is no statistic for it): that the shape reaches the two-level forms rests on the
    CPU twin's arithmetic, that option setop_fused_part selects between them on run_setop_pass reading it."""
    ctx, L = env
    case, other = big_setop(op, form), big_setop(op, form, SEED + 99)
    opts = {"force_ticket": ticket}
    if fused is not None:
        opts["setop_fused_part"] = fused
    with options(ctx, opts):
        patterns(ctx, lambda: run_case(ctx, L, case))
        stale_twin(ctx, lambda: run_case(ctx, L, other), lambda: run_case(ctx, L, case), 512 * MB)


# ---- 3b. ukm_sort_u64 / ukm_sort_pairs ---------------------------------------------------------------------------------------------
LS_CLASS_KPT = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16)   # ukm_sort_plan.h; x LS_NT = 256 keys: the size classes of the bucket kernel
LS_MIN_BITS = 8 * 2 + 16            #               two top passes + two digits for the buckets' own passes: narrower keys are declined
ROUTE_HOST_HIST, ROUTE_FUSED, ROUTE_BUCKETS, ROUTE_CHUNKED = 1, 2, 3, 4   # enum SortRoute: the values of the statistic "sort_route"
LS_FAN_MIN = 3                      #               size classes that must occur for the launches to fan out over the side streams
SORT_ROWS = {   # name: (n, shape of the keys, options)
    "host-hist": (100_003, "even", {}),
    # (sort_counting = 1: the buckets' counting step whatever earlier sorts of the context met -- a context that saw most
    #  buckets fall back to the digit passes skips the attempt for its next 15 sorts)
    "buckets": (1 << 23, "even", {"sort_counting": 1}),      # the bucket route at its threshold
    "crowded": (1 << 23, "crowded", {"sort_counting": 1}),   # the oversized-bucket gather + a nested general sort
    "digit-passes": (1 << 23, "even", {"sort_counting": 0}),
    "fan": (1 << 23, "sloped", {"sort_counting": 1}),        # buckets of every size up to twice the average: side streams
    "no-fan": (1 << 23, "sloped", {"sort_counting": 1, "sort_fan": 0}),   # the same classes on one stream
    "fused-hist": (1 << 24, "even", {"sort_local": 0}),
    # keys narrower than declared: the OR word of the first histogram narrows them (key_bits = 64 only: a narrower
    # declaration is taken at its word)
    "narrow-64": (1 << 23, "even", {"sort_counting": 1}),    # 40 bits: still two top passes + two digits, the route goes on
    "too-narrow-64": (1 << 23, "even", {}),                  # 30 bits: declined, and below SORT_FUSED_MIN the host histograms answer
    "gives-up": (1 << 23, "16-buckets", {}),                 # every key in 16 buckets: the classify verdict hands the call back
}
SORT_WIDTH = {"narrow-64": 40, "too-narrow-64": 30}          # row: bits the keys really have (default: as declared)
SORT_BITS = {"narrow-64": (64,), "too-narrow-64": (64,)}     # row: the declared widths it runs at (default: 62 and 64)
CROWDED = ((5, 600_000), (77, 200_000))     # (bucket, keys): as test_sort_top16_then_lds_buckets, at n = 2^23


def sort_input(row, bits, seed):
    n, shape, _ = SORT_ROWS[row]
    bits = SORT_WIDTH.get(row, bits)
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << bits, n, dtype=U64)
    if shape == "sloped":                   # the density rises with the value: bucket b holds n (2 b + 1) / buckets^2 keys
        x = np.maximum(x, rng.integers(0, 1 << bits, n, dtype=U64))
    if shape == "crowded":
        low = bits - ls_topb(n)
        at = 0
        for bucket, count in CROWDED:
            x[at:at + count] = (x[at:at + count] & U64((1 << low) - 1)) | U64(bucket << low)
            at += count
        x = x[rng.permutation(n)]
    if shape == "16-buckets":               # the top bits of every key: 1 0 .. 0 1 1, then four free bucket bits
        low = bits - ls_topb(n) + 4
        x = (x & U64((1 << low) - 1)) | U64(((1 << (bits - low - 1)) | 3) << low)
    m = len(x[1::7])
    x[::7][:m] = x[1::7]                    # equal keys: what the stability of a pair sort is about
    x[3] |= U64(1 << (bits - 1))            # (neither written nor copied above) the OR of all keys is exactly `bits` wide
    return x


def check_sort_path(row, bits, sorted_keys):
    """from the bucket counts of the reference sort: which route the sources' constants send this input through.
    Returns what every sort of the row leaves in the statistics: ("sort_route", the rise of "sort_bucket_declined",
    "sort_oversized_buckets")."""
    n, shape, opts = SORT_ROWS[row]
    general = ROUTE_HOST_HIST if n < SORT_FUSED_MIN else ROUTE_FUSED
    if n < SORT_LOCAL_MIN:
        assert general == ROUTE_HOST_HIST
        return general, 0, 0
    if opts.get("sort_local") == 0:
        assert general == ROUTE_FUSED
        return general, 0, 0
    assert n == SORT_LOCAL_MIN and bits >= 32
    width = SORT_WIDTH.get(row, bits)
    assert width == bits or bits == 64                  # (only key_bits = 64 makes the sort look at the keys' OR)
    assert int(sorted_keys[-1]) >> (width - 1) == 1     # the OR of all keys is `width` wide: 64 stays, narrower keys narrow it
    topb = ls_topb(n)
    assert topb <= 16
    if width < LS_MIN_BITS:
        return general, 1, 0
    counts = np.bincount((sorted_keys >> U64(width - topb)).astype(np.int64), minlength=1 << topb)
    big = counts > LS_CLASS_MAX
    if shape == "16-buckets":
        assert (counts > 0).sum() == 16 and big.sum() == 16
        assert counts[big].sum() > n // 4               # the route gives up (and its later attempts stop at the sample)
        return general, 1, 0
    if shape == "crowded":
        assert big.sum() == len(CROWDED) and all(big[b] for b, _ in CROWDED)
        assert big.sum() <= LS_MAX_BIG and counts[big].sum() <= n // 4       # the route does not give up
    else:
        assert not big.any()
    classes = np.unique(np.searchsorted(np.array(LS_CLASS_KPT) * 256, counts[(counts > 0) & ~big], side="left"))
    if shape == "sloped":
        assert len(classes) >= LS_FAN_MIN + 3, classes     # (well beyond the minimum: the launches go round the three streams twice)
    return ROUTE_BUCKETS, 0, int(big.sum())


# what check_sort_path must find for the rows: (sort_route, sort_bucket_declined per sort, sort_oversized_buckets)
SORT_STATS = {"host-hist": (1, 0, 0), "fused-hist": (2, 0, 0), "buckets": (3, 0, 0), "digit-passes": (3, 0, 0), "fan": (3, 0, 0),
              "no-fan": (3, 0, 0), "crowded": (3, 0, len(CROWDED)), "narrow-64": (3, 0, 0), "too-narrow-64": (1, 1, 0),
              "gives-up": (1, 1, 0)}


SORT_CASES = [(row, bits) for row in SORT_ROWS for bits in SORT_BITS.get(row, (62, 64))]


@pytest.mark.parametrize("row,bits", SORT_CASES)
def test_sort_shapes_oracle_only(row, bits):
    x = sort_input(row, bits, 5)
    s = np.sort(x)
    assert len(np.unique(s)) < len(s)
    assert check_sort_path(row, bits, s) == SORT_STATS[row]
    assert check_sort_path(row, bits, np.sort(sort_input(row, bits, 6))) == SORT_STATS[row]     # (the stale twin's first call)
    assert len(sort_input(row, bits, 6)) == len(x) and not np.array_equal(sort_input(row, bits, 6), x)


@pytest.mark.gpu
@pytest.mark.parametrize("row,bits", SORT_CASES)
def test_sort(row, bits):
    """keys against np.sort, pairs against np.argsort(kind="stable").  A context of its own per row: the sort keeps
    state from one call to the next (SortPolicy: skew_seen, counting_skip), and a row must not inherit another row's.
    After every sort the statistics show the route that check_sort_path derives from the sources' constants (the CPU twin
    test_sort_shapes_oracle_only pins them to SORT_STATS)."""
    import torch
    from unikmer_amd import lib as L
    n, _, opts = SORT_ROWS[row]
    x = sort_input(row, bits, 5)
    order = np.argsort(x, kind="stable")
    up = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    xd, expd, orderd = up(x), up(x[order]), torch.from_numpy(order.astype(np.int32)).cuda()
    od = up(sort_input(row, bits, 6))
    route, declines, oversized = check_sort_path(row, bits, x[order])
    assert (route, declines, oversized) == SORT_STATS[row]
    del x, order

    def routed(call):
        declined = ctx.stat("sort_bucket_declined")
        call()
        assert ctx.stat("sort_route") == route, (row, bits, ctx.stat("sort_route"))
        assert ctx.stat("sort_bucket_declined") == declined + declines, (row, bits)
        assert ctx.stat("sort_oversized_buckets") == oversized, (row, bits, ctx.stat("sort_oversized_buckets"))

    def keys(src, exp=None):
        w = src.clone()
        torch.cuda.synchronize()
        routed(lambda: ctx.sort_u64(w, bits))
        assert exp is None or torch.equal(w, exp), (row, bits, "keys")

    def pairs(src, exp=None):
        w, v = src.clone(), torch.arange(n, dtype=torch.int32, device=src.device)
        torch.cuda.synchronize()
        routed(lambda: ctx.sort_pairs(w, v, bits))
        assert exp is None or (torch.equal(w, exp) and torch.equal(v, orderd)), (row, bits, "pairs")

    ctx = L.Context(0)
    try:
        with options(ctx, opts):
            for fn in (keys, pairs):
                patterns(ctx, lambda: fn(xd, expd))
                stale_twin(ctx, lambda: fn(od), lambda: fn(xd, expd), 1024 * MB)
        if row == "gives-up":       # the context stays usable: evenly spread keys pass its sample and take the bucket route
            even = np.random.default_rng(7).integers(0, 1 << bits, n, dtype=U64)
            w = up(even)
            declined = ctx.stat("sort_bucket_declined")
            ctx.sort_u64(w, bits)
            assert torch.equal(w, up(np.sort(even))), (row, bits, "even keys afterwards")
            assert ctx.stat("sort_route") == ROUTE_BUCKETS and ctx.stat("sort_bucket_declined") == declined
    finally:
        ctx.close()


@pytest.mark.gpu
def test_sort_fresh_context_grows_block_by_block():
    """host arrays of 2^23 pairs: the keys fill the first 64 MB block, the taxids open a second one, the scratch copies a
    third -- every block is poisoned when it is created, in the middle of the call"""
    from unikmer_amd import lib as L
    x = sort_input("buckets", 62, 5)
    order = np.argsort(x, kind="stable")
    k, v = x.copy(), np.arange(len(x), dtype=U32)
    ctx = L.Context(0)
    try:
        with options(ctx, {"ws_poison": 0xAA}):
            ctx.sort_pairs(k, v, 62)
            poisoned(ctx)
            # (ws_poisoned_bytes: the blocks the call created AND the one block they were consolidated into when it ended)
            assert ctx.stat("workspace_blocks") == 1 and ctx.stat("ws_poisoned_bytes") > ctx.stat("workspace_bytes") > 64 * MB
        assert np.array_equal(k, x[order]) and np.array_equal(v, order.astype(U32))
    finally:
        ctx.close()


# ---- 3c. the k-way merge at every fan-in ----------------------------------------------------------------------------------------
def _merge_streams(seed):
    real = _big_merge()
    if seed is None:
        return list(real)
    rng = np.random.default_rng(seed)
    return [np.sort(rng.integers(0, 1 << 22, len(f)).astype(U64)) for f in real]


@functools.lru_cache(None)
def kway_case(which, k, seed=None):
    opts = {"kway": 1, "srmerge": 0, "punion": 0, "place": 0, "kway_k": k}
    data = lambda: (_merge_streams(seed),)
    if which == "union":
        return Case("kway%d-union-%s" % (k, seed), data=data, call=lambda ctx, L, outs, files: ctx.union(files, **_o2(outs)),
                    expect=lambda O, tax, files: O.union(files), bound=lambda files: sum(len(f) for f in files), dtypes=[U64], opts=opts,
                    route=ROUTE_KWAY)
    return Case("kway%d-merge-%s" % (k, seed), data=data, call=lambda ctx, L, outs, files: ctx.merge_k(files, mode=PLAIN, **_o2(outs)),
                expect=lambda O, tax, files: _stable(files, None), bound=lambda files: 2 * sum(len(f) for f in files), dtypes=[U64],
                opts=opts, route=ROUTE_KWAY)


def test_kway_shapes_oracle_only():
    """no GPU: 12 streams are more than 8, so that kway_k = 16 is taken (pick_k) and 4 / 8 need two levels; 2^20 records
    or more, so that the merge's two-child top level at fan-in 8 is the 2-way tile kernel"""
    files = _merge_streams(None)
    assert len(files) == 12 > 8 and sum(len(f) for f in files) >= KWAY_TOP2_MIN
    assert [len(f) for f in _merge_streams(9)] == [len(f) for f in files]
    u, m = kway_case("union", 4).expected()[0], kway_case("merge", 4).expected()[0]
    assert np.array_equal(u, np.unique(m)) and len(m) == sum(len(f) for f in files) and len(u) < len(m)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [4, 8, 16])
@pytest.mark.parametrize("which", ["union", "merge"])
def test_kway_fan_in(env, which, k):
    """fan-in 16 is a 512-thread, 70 KB instantiation of its own"""
    ctx, L = env
    case, other = kway_case(which, k), kway_case(which, k, 9)
    assert ctx.get_option("kway_k") is None
    patterns(ctx, lambda: run_case(ctx, L, case))
    stale_twin(ctx, lambda: run_case(ctx, L, other), lambda: run_case(ctx, L, case), 256 * MB)


# ---- 3d. ukm_lca, ukm_partition_points, ukm_shard_splitters -----------------------------------------------------------------------
def _lca_pairs(seed):
    T = _oracle()[2]
    rng = np.random.default_rng(seed)
    return rng.integers(0, T + 50, 20000).astype(U32), rng.integers(0, T + 50, 20000).astype(U32)   # includes 0 and unknown ids


def _partition_input(seed, at):
    """the size test_gpu_parity.py uses; splitters at and just behind record at[0], at record at[1], at the last record, behind all"""
    A = _universe(75_000, 22, seed)
    return A, np.array([0, A[at[0]], A[at[0]] + U64(1), A[at[1]], A[-1], 2**63], dtype=U64)


PARTITION_REAL, PARTITION_TWIN = (SEED, (10, 41_234)), (SEED + 5, (5_000, 70_000))


def test_small_calls_oracle_only():
    tax = _oracle()[1]
    a, b = _lca_pairs(3)
    exp = np.array([tax.lca(x, y) for x, y in zip(a[:2000], b[:2000])], dtype=U32)
    assert (exp != 0).any() and (exp == 0).any()
    (A, sp), (A2, sp2) = _partition_input(*PARTITION_REAL), _partition_input(*PARTITION_TWIN)
    cuts, cuts2 = np.searchsorted(A, sp, side="left"), np.searchsorted(A2, sp2, side="left")
    assert cuts.tolist() == [0, 10, 11, 41_234, len(A) - 1, len(A)]
    # the stale twin: as many cuts over as many records, every inner one different -- a cut left over from it is wrong
    assert len(A2) == len(A) and len(cuts2) == len(cuts) and (cuts2 != cuts)[1:4].all()


@pytest.mark.gpu
def test_lca(env):
    ctx, L = env
    tax = _oracle()[1]
    (a, b), (a2, b2) = _lca_pairs(3), _lca_pairs(4)
    exp = np.array([tax.lca(x, y) for x, y in zip(a, b)], dtype=U32)
    real = lambda: np.testing.assert_array_equal(ctx.lca(a, b), exp)
    patterns(ctx, real)
    stale_twin(ctx, lambda: ctx.lca(a2, b2), real, 64 * MB)


@pytest.mark.gpu
def test_partition_points(env):
    ctx, L = env
    (A, sp), (A2, sp2) = _partition_input(*PARTITION_REAL), _partition_input(*PARTITION_TWIN)
    exp = np.searchsorted(A, sp, side="left").astype(U64)
    real = lambda: np.testing.assert_array_equal(ctx.partition_points(A, sp), exp)
    patterns(ctx, real)
    stale_twin(ctx, lambda: ctx.partition_points(A2, sp2), real, 64 * MB)


@pytest.mark.gpu
def test_shard_splitters_one_rank():
    """A communicator of one rank, the only size one device allows.  The boundaries of one rank are [0, top] whatever
    the samples are, and neither the samples nor the gathered words can be read from the host: this test covers only that
    the sampling kernel and the gather run to the end under every pattern and return the fixed answer.  It cannot fail
    because a sample was read from uninitialised workspace; what the boundaries of several ranks are made of is checked
    on the host by the shard_splitters_plan tests of test_dist_gloo.py."""
    from unikmer_amd import lib as L
    rng = np.random.default_rng(3)
    keys = np.unique(rng.integers(0, 1 << 62, 300_000, dtype=U64))
    files = [keys, np.empty(0, U64), keys[::2].copy()]
    ctx = L.Context(0)
    try:
        ctx.comm_init(1, 0, L.Context.comm_unique_id())
        def real():
            assert ctx.shard_splitters(files, 62) == [0, 1 << 62]
        patterns(ctx, real)
        ctx.comm_destroy()
    finally:
        ctx.close()


# ---- 4. context plumbing that changes where the work runs -----------------------------------------------------------------------
def _pinned(ctx, nbytes, dtype=np.uint8):
    p = ctx.host_alloc(nbytes)
    return p, np.frombuffer((ctypes.c_uint8 * nbytes).from_address(p), dtype=dtype)


CHUNK, CHUNK_K = 150_000, 31


def _chunks():
    rng = np.random.default_rng(21)
    return [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, CHUNK)] for _ in range(3)]


def _chunk_counts(O):
    off = np.array([0, CHUNK], dtype=U64)
    return [O.unique(O.sort_u64(O.count_windows(c, off, CHUNK_K))) for c in _chunks()]


def test_async_copy_oracle_only():
    exp = _chunk_counts(_oracle()[0])
    assert all(2 <= len(e) <= CHUNK - CHUNK_K + 1 and np.all(e[1:] > e[:-1]) for e in exp)
    assert not np.array_equal(exp[0], exp[1])


@pytest.mark.gpu
def test_device_and_pinned_memory_round_trip(env):
    ctx, L = env
    n = 1 << 16
    src = np.arange(n, dtype=U64)
    d = ctx.dev_alloc(8 * n)
    p, back = _pinned(ctx, 8 * n, U64)
    try:
        back[:] = 0
        ctx.copy(d, src.ctypes.data, 8 * n)          # pageable host -> device, synchronous
        ctx.copy_async(p, d, 8 * n)                  # device -> pinned host, on the transfer stream
        ctx.copy_sync()
        assert np.array_equal(back, src)
    finally:
        ctx.host_free(p)
        ctx.dev_free(d)


@pytest.mark.gpu
def test_async_copy_double_buffering(env):
    """The header's idiom: copy_async(chunk i + 1); compute(chunk i); copy_fence -- two pinned chunks of bases, two device
    buffers, the distinct k-mers of every chunk copied back with copy_async + copy_sync.  A smoke test of the documented
    ordering (transfers start behind the compute issued so far; compute issued behind a fence starts behind the
    transfers), not a proof of it: a missing wait may still win its race."""
    import torch
    ctx, L = env
    O = _oracle()[0]
    chunks, exp = _chunks(), _chunk_counts(O)
    off = torch.tensor([0, CHUNK], dtype=torch.int64, device="cuda")
    dev = [torch.empty(CHUNK, dtype=torch.uint8, device="cuda") for _ in range(2)]
    out = torch.empty(CHUNK, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    pins = [_pinned(ctx, CHUNK) for _ in range(2)]
    rp, res = _pinned(ctx, 8 * CHUNK, U64)
    try:
        with options(ctx, {"ws_poison": 0xAA}):
            pins[0][1][:] = chunks[0]
            ctx.copy_async(dev[0].data_ptr(), pins[0][0], CHUNK)
            ctx.copy_fence()
            for i in range(len(chunks)):
                if i + 1 < len(chunks):
                    if i + 1 >= 2:
                        ctx.copy_sync()              # the pinned source of chunk i - 1 is free again
                    pins[(i + 1) % 2][1][:] = chunks[i + 1]
                    ctx.copy_async(dev[(i + 1) % 2].data_ptr(), pins[(i + 1) % 2][0], CHUNK)
                got = ctx.count(dev[i % 2], off, CHUNK_K, mode=UNIQUE, out=out)
                poisoned(ctx)
                ctx.copy_fence()
                res[:] = 0
                ctx.copy_async(rp, out.data_ptr(), 8 * len(got))
                ctx.copy_sync()
                assert np.array_equal(res[:len(got)], exp[i]), i
    finally:
        ctx.copy_sync()
        for p, _ in pins:
            ctx.host_free(p)
        ctx.host_free(rp)


@pytest.mark.gpu
def test_borrowed_stream(env):
    """A context on a borrowed stream: the producer -- torch.sort of 2^24 int64 -- is enqueued on that stream immediately
    before setop2 reads its output, with no host synchronisation in between.  Compared with the same call after
    torch.cuda.synchronize() and with the oracle.  A smoke test of the documented ordering ("work the caller enqueued on
    that stream before a ukm_* call is ordered before the call's kernels"), not a proof of it."""
    import torch
    from unikmer_amd import lib as L
    O = _oracle()[0]
    n = 1 << 24
    a = np.random.default_rng(12).permutation(n) * 5     # int64, distinct: sorted, it is the set of the multiples of 5 below 5 n
    b = np.arange(0, 5 * n, 21, dtype=U64)
    exp = O.inter([np.arange(n, dtype=U64) * U64(5), b])
    assert np.array_equal(exp, np.arange(0, 5 * n, 105, dtype=U64))
    st = torch.cuda.Stream()
    ctx = L.Context(0, stream=st.cuda_stream)
    try:
        with options(ctx, {"ws_poison": 0xAA}):
            ad = torch.from_numpy(a).cuda()
            bd = torch.from_numpy(b.view(np.int64)).cuda()
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                s2 = torch.sort(ad).values          # the producer: nothing between it and the call
                got = ctx.setop2(OP_INTER, s2, bd)
            poisoned(ctx)
            torch.cuda.synchronize()
            again = ctx.setop2(OP_INTER, s2, bd)
            assert np.array_equal(got.cpu().numpy().view(U64), exp)
            assert torch.equal(got, again)
        ctx.set_stream(0)                           # HIP's default stream of the device: still a valid stream to borrow
        torch.cuda.synchronize()
        assert np.array_equal(ctx.setop2(OP_INTER, s2, bd).cpu().numpy().view(U64), exp)
    finally:
        ctx.close()
