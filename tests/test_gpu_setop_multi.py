"""ukm_setop2_multi on the GPU: union, inter and diff of one pair from a single pass.

Every expected array comes from the CPU oracle (oracle.union / inter / diff) and is additionally compared with the
separate ctx.setop2 calls.  Fused cases must show "setop_multi_fused" going up by one, every other case
"setop_multi_split".  TILE (test_setop_multi_cpu.py, checked against the source there) is the kernel's tile; the shapes
sit on its edges: one record round a tile, a partial last tile, the 256 tiles from which the partition runs in two
levels, tiles that hold records of one input only, and the two shapes that aim at the straddle term of the union's offset.
"""
import contextlib
import functools

import numpy as np
import pytest

from conftest import splitmix64, synth_tree
from test_setop_multi_cpu import TILE, U64, straddle_sets

U32 = np.uint32
OP_UNION, OP_INTER, OP_DIFF = 0, 1, 2
UID = (OP_UNION, OP_INTER, OP_DIFF)
COMBOS = {"UI": (OP_UNION, OP_INTER), "UD": (OP_UNION, OP_DIFF), "ID": (OP_INTER, OP_DIFF), "UID": UID}
G64 = 0xA5A5A5A5A5A5A5A5
GUARD = 64
PART_COARSE = 64                 # ukm_setop_part.h: the partition runs in two levels (one fused launch) from 4 x 64 tiles
CACHE_STATS = ("setop_part_hits", "setop_part_stale", "setop_offs_hits", "setop_offs_stale")


# ---- data ------------------------------------------------------------------------------------------------------------------------
def universe(n, seed):
    j = np.arange(n, dtype=U64)
    return (U64(1) << U64(32)) + np.cumsum(U64(2) + (splitmix64(U64(seed) ^ j) & U64((1 << 20) - 1)), dtype=U64)


def thirds(total, overlap, seed=0x6D75):
    """two sorted sets with (at most a record less than) `total` records together: overlap 0 = disjoint, 1/3 = a third
    of A is in B too, in random order (the benchmark's mix: |A n B| = |A| / 3 = |B| / 3), 1 = the same set twice"""
    if overlap == 1:
        A = universe(total // 2, seed)
        return A, A.copy()
    U = universe(total, seed)
    m = splitmix64(U64(seed + 1) ^ np.arange(len(U), dtype=U64)) % U64(5)
    if overlap == 0:
        return U[m < 2], U[m >= 2]
    # both: m == 2.  |A| + |B| = |U| + |both|: cut U so that the sum is `total`
    both = np.cumsum(m == 2)
    n = int(np.searchsorted(np.arange(1, len(U) + 1) + both, total, side="right"))
    U, m = U[:n], m[:n]
    return U[m <= 2], U[m >= 2]


def sized(total):
    """overlap 1/3 with |A| + |B| = total exactly"""
    A, B = thirds(total + 8, 1 / 3)
    while len(A) + len(B) > total:
        if len(A) >= len(B):
            A = A[:-1]
        else:
            B = B[:-1]
    assert len(A) + len(B) == total
    return A, B


def e():
    return np.empty(0, dtype=U64)


SHAPES = {
    "both-empty": lambda: (e(), e()),
    "a-empty": lambda: (e(), universe(1000, 1)),
    "b-empty": lambda: (universe(1000, 2), e()),
    "one-each-equal": lambda: (np.array([77], U64), np.array([77], U64)),
    "one-each-different": lambda: (np.array([77], U64), np.array([78], U64)),
    "a-equals-b": lambda: (universe(3 * TILE // 2 + 5, 3), universe(3 * TILE // 2 + 5, 3)),
    "disjoint-a-below-b": lambda: (universe(TILE + 11, 4), universe(TILE + 7, 4) + (U64(1) << U64(60))),
    "disjoint-interleaved": lambda: (np.arange(0, 2 * (TILE + 9), 2, dtype=U64), np.arange(1, 2 * (TILE + 9), 2, dtype=U64)),
    "tile-minus-1": lambda: sized(TILE - 1),
    "tile": lambda: sized(TILE),
    "tile-plus-1": lambda: sized(TILE + 1),
    "three-tiles-overlap-0": lambda: thirds(2 * TILE + TILE // 2 + 3, 0),
    "three-tiles-overlap-third": lambda: thirds(2 * TILE + TILE // 2 + 3, 1 / 3),
    "three-tiles-overlap-1": lambda: thirds(2 * TILE + TILE // 2 + 3, 1),
    "two-level-259-tiles": lambda: thirds((4 * PART_COARSE + 2) * TILE + TILE // 3, 1 / 3, seed=0x3259),
    "na-much-larger": lambda: (universe(4 * TILE + 100, 5), universe(4 * TILE + 100, 5)[::997].copy()),
    "nb-much-larger": lambda: (universe(4 * TILE + 100, 6)[5::1013].copy(), universe(4 * TILE + 100, 6)),
    "straddle-every-boundary": lambda: straddle_sets(False),
    "straddle-none": lambda: straddle_sets(True),
}
THREE, BIG = "three-tiles-overlap-third", "two-level-259-tiles"


@functools.lru_cache(maxsize=None)
def shape(name):
    A, B = SHAPES[name]()
    A, B = np.ascontiguousarray(A, U64), np.ascontiguousarray(B, U64)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's three results of a shape, computed once"""
    from oracle import oracle as O
    A, B = shape(name)
    want = {OP_UNION: O.union([A, B]), OP_INTER: O.inter([A, B]), OP_DIFF: O.diff([A, B])}
    if len(B) == 0:
        # oracle.inter is the n-file command, whose fold stops at an empty later file and keeps the running result
        # (inter.go:211-217); the 2-way call is the plain intersection, as test_gpu_parity.py asserts for setop2
        assert np.array_equal(want[OP_INTER], A)
        want[OP_INTER] = np.empty(0, dtype=U64)
    return want


def test_the_two_level_shape_has_at_least_256_tiles():
    A, B = shape(BIG)
    assert (len(A) + len(B) + TILE - 1) // TILE == 4 * PART_COARSE + 3 >= 256


def test_shapes_are_what_their_names_say():
    for name in ("tile-minus-1", "tile", "tile-plus-1"):
        A, B = shape(name)
        assert len(A) + len(B) == TILE + {"tile-minus-1": -1, "tile": 0, "tile-plus-1": 1}[name]
    for name, ov in (("three-tiles-overlap-0", 0), ("three-tiles-overlap-third", None), ("three-tiles-overlap-1", 1)):
        A, B = shape(name)
        assert (len(A) + len(B) + TILE - 1) // TILE == 3 and (len(A) + len(B)) % TILE != 0
        m = len(np.intersect1d(A, B))
        assert (m == 0) if ov == 0 else (m == len(A) == len(B)) if ov == 1 else (0.3 < m / len(A) < 0.37)
    A, B = shape("na-much-larger")
    assert len(B) * 100 < len(A) and len(B) > 10
    A, B = shape("nb-much-larger")
    assert len(A) * 100 < len(B) and len(A) > 10
    for name in SHAPES:
        A, B = shape(name)
        assert np.all(A[1:] > A[:-1]) and np.all(B[1:] > B[:-1]), name


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    import torch
    from unikmer_amd import lib
    ctx = lib.Context(0)
    yield ctx, lib, torch
    ctx.close()


def dev(torch, a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]).copy()).cuda()
    torch.cuda.synchronize()
    return t


def host(t, dtype=U64):
    return t.cpu().numpy().view(dtype)


def stats(ctx, keys=("setop_multi_fused", "setop_multi_split")):
    return tuple(ctx.stat(k) for k in keys)


@contextlib.contextmanager
def options(ctx, opts):
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        yield
    finally:
        for k in opts:
            ctx.set_option(k, None)


_separate = {}


def separate(env, name):
    """the three separate setop2 calls on a shape, once"""
    ctx, lib, torch = env
    if name not in _separate:
        A, B = shape(name)
        dA, dB = dev(torch, A), dev(torch, B)
        _separate[name] = {op: host(ctx.setop2(op, dA, dB)).copy() for op in UID}
    return _separate[name]


def run_fused(env, name, ops, want_route=(1, 0)):
    ctx, lib, torch = env
    A, B = shape(name)
    dA, dB = dev(torch, A), dev(torch, B)
    s0, c0 = stats(ctx), stats(ctx, CACHE_STATS)
    got = ctx.setop2_multi(dA, dB, ops=ops)
    s1, c1 = stats(ctx), stats(ctx, CACHE_STATS)
    assert (s1[0] - s0[0], s1[1] - s0[1]) == want_route, "(fused, split) moved by %r" % ((s1[0] - s0[0], s1[1] - s0[1]),)
    if want_route == (1, 0):
        assert c1 == c0, "a fused call moved the partition cache's counters"
    assert sorted(got) == sorted(ops)
    want, sep = expected(name), separate(env, name)
    for op in ops:
        g = host(got[op])
        assert len(g) == len(want[op]), "op %d: %d records, the oracle has %d" % (op, len(g), len(want[op]))
        assert np.array_equal(g, want[op]), "op %d differs from the oracle (first at %d)" % (op, int(np.flatnonzero(g != want[op])[0]))
        assert np.array_equal(g, sep[op]), "op %d differs from ctx.setop2" % op
    assert np.array_equal(host(dA), A) and np.array_equal(host(dB), B), "an input was modified"


@pytest.mark.gpu
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_combination_is_bit_exact(env, name, combo):
    # (both inputs empty: nothing to fuse -- the split route answers, with three empty results)
    run_fused(env, name, COMBOS[combo], (0, 1) if name == "both-empty" else (1, 0))


@pytest.mark.gpu
def test_ticketed_tile_ids(env):
    ctx = env[0]
    with options(ctx, {"force_ticket": 1}):
        for name in (THREE, BIG, "straddle-every-boundary"):
            run_fused(env, name, UID)


# ---- routes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_duplicate_codes_take_the_split_route(env):
    ctx, lib, torch = env
    from oracle import oracle as O
    A, B = (x.copy() for x in shape(THREE))
    A[TILE + 5] = A[TILE + 4]                       # one duplicated code inside A (legal for inter and diff)
    A[100] = A[99]
    dA, dB = dev(torch, A), dev(torch, B)
    s0 = stats(ctx)
    got = ctx.setop2_multi(dA, dB, ops=(OP_INTER, OP_DIFF))
    assert stats(ctx) == (s0[0], s0[1] + 1)
    for op, fn in ((OP_INTER, O.inter), (OP_DIFF, O.diff)):
        assert np.array_equal(host(got[op]), fn([A, B]))
        assert np.array_equal(host(got[op]), host(ctx.setop2(op, dA, dB)))


@pytest.fixture(scope="module")
def taxenv():
    import torch
    from oracle import oracle as O
    from unikmer_amd import lib
    ctx = lib.Context(0)
    child, parent = synth_tree(depth=3, arity=8)
    ctx.taxonomy_load(child, parent)
    yield ctx, lib, torch, O, O.Taxonomy(child, parent), len(child)
    ctx.close()


def tax_case(taxenv, ops, ta, tb, flags=0, okw=None):
    """taxids of any form: the split route, equal to the separate calls; to the oracle where `okw` says how it is asked"""
    ctx, lib, torch, O, tax, _ = taxenv
    A, B = shape(THREE)
    dA, dB = dev(torch, A), dev(torch, B)
    up = lambda t: t if isinstance(t, int) or t is None else dev(torch, t)
    dta, dtb = up(ta), up(tb)
    s0 = stats(ctx)
    got = ctx.setop2_multi(dA, dB, ops=ops, a_taxids=dta, b_taxids=dtb, flags=flags)
    assert stats(ctx) == (s0[0], s0[1] + 1)
    full = lambda t, n: np.full(n, t, U32) if isinstance(t, int) else t
    for op in ops:
        gk, gt = got[op]
        sk, st = ctx.setop2(op, dA, dB, dta, dtb, flags=flags)
        assert np.array_equal(host(gk), host(sk)) and np.array_equal(host(gt, U32), host(st, U32)), op
        if okw is not None and op in okw:
            wk, wt = {OP_UNION: O.union, OP_INTER: O.inter, OP_DIFF: O.diff}[op]([A, B], [full(ta, len(A)), full(tb, len(B))], tax, **okw[op])
            assert np.array_equal(host(gk), wk) and np.array_equal(host(gt, U32), wt), op


def rand_taxids(n, ntax, seed):
    return (1 + splitmix64(np.arange(n, dtype=U64) ^ U64(seed)) % U64(ntax)).astype(U32)


@pytest.mark.gpu
def test_per_record_taxids_take_the_split_route(taxenv):
    A, B = shape(THREE)
    ta, tb = rand_taxids(len(A), taxenv[5], 11), rand_taxids(len(B), taxenv[5], 12)
    tax_case(taxenv, UID, ta, tb, okw={OP_UNION: {}, OP_INTER: {}, OP_DIFF: {}})


@pytest.mark.gpu
def test_file_taxids_take_the_split_route(taxenv):
    tax_case(taxenv, UID, 77, 300, okw={OP_UNION: {}, OP_INTER: {}, OP_DIFF: {}})


@pytest.mark.gpu
def test_mix_taxid_takes_the_split_route(taxenv):
    A, B = shape(THREE)
    ta, tb = rand_taxids(len(A), taxenv[5], 13), rand_taxids(len(B), taxenv[5], 14)
    ta[::5] = 0
    tax_case(taxenv, (OP_UNION, OP_INTER), ta, tb, flags=2, okw={OP_INTER: {"mix_taxid": True}})


@pytest.mark.gpu
def test_cmp_taxid_takes_the_split_route(taxenv):
    A, B = shape(THREE)
    ta, tb = rand_taxids(len(A), taxenv[5], 15), rand_taxids(len(B), taxenv[5], 16)
    tax_case(taxenv, (OP_INTER, OP_DIFF), ta, tb, flags=4, okw={OP_DIFF: {"compare_taxid": True}})


@pytest.mark.gpu
@pytest.mark.parametrize("op", UID)
def test_a_single_operation_takes_the_split_route(env, op):
    run_fused(env, THREE, (op,), (0, 1))


@pytest.mark.gpu
def test_the_partition_cache_does_not_see_a_fused_call():
    """setop2 union, inter, diff on one pair: the hit pattern of the partition and offset caches, with and without fused
    calls in between"""
    import torch
    from unikmer_amd import lib
    A, B = shape(BIG)
    want = expected(BIG)
    trace = {}
    for fused_between in (False, True):
        ctx = lib.Context(0)
        try:
            dA, dB = dev(torch, A), dev(torch, B)
            seen = []
            for op in UID:
                assert np.array_equal(host(ctx.setop2(op, dA, dB)), want[op])
                seen.append(stats(ctx, CACHE_STATS))
                if fused_between:
                    before = stats(ctx, CACHE_STATS)
                    got = ctx.setop2_multi(dA, dB, ops=UID)
                    assert all(np.array_equal(host(got[x]), want[x]) for x in UID)
                    assert stats(ctx, CACHE_STATS) == before and stats(ctx) == (len(seen), 0)
            trace[fused_between] = seen
        finally:
            ctx.close()
    assert trace[True] == trace[False], trace
    assert trace[False][-1][0] == 2, "the plain sequence itself no longer hits the cache: %r" % (trace[False],)


# ---- errors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ("A", "B"))
def test_unsorted_input(env, which):
    ctx, lib, torch = env
    A, B = (x.copy() for x in shape(THREE))
    x = A if which == "A" else B
    x[TILE + 3], x[TILE + 4] = x[TILE + 4], x[TILE + 3]
    with pytest.raises(lib.UnsortedError) as err:
        ctx.setop2_multi(dev(torch, A), dev(torch, B), ops=UID)
    assert err.value.code == lib.ERR_UNSORTED


@pytest.mark.gpu
@pytest.mark.parametrize("ops", ((), (3,)))
def test_invalid_ops(env, ops):
    ctx, lib, torch = env
    A, B = shape("tile")
    with pytest.raises(lib.UkmError) as err:
        ctx.setop2_multi(dev(torch, A), dev(torch, B), ops=ops)
    assert err.value.code == lib.ERR_INVALID


@pytest.mark.gpu
def test_taxids_without_a_taxonomy(env):
    ctx, lib, torch = env
    A, B = shape("tile")
    ta, tb = rand_taxids(len(A), 100, 1), rand_taxids(len(B), 100, 2)
    for call in (lambda: ctx.setop2_multi(dev(torch, A), dev(torch, B), ops=(OP_UNION, OP_INTER), a_taxids=dev(torch, ta), b_taxids=dev(torch, tb)),
                 lambda: ctx.setop2(OP_UNION, dev(torch, A), dev(torch, B), dev(torch, ta), dev(torch, tb))):
        with pytest.raises(lib.UkmError) as err:
            call()
        assert err.value.code == lib.ERR_NO_TAXONOMY


# ---- capacity ------------------------------------------------------------------------------------------------------------------------
def guarded(torch, cap):
    buf = torch.full((cap + GUARD,), G64 - (1 << 64), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return buf


@pytest.mark.gpu
@pytest.mark.parametrize("query", (False, True), ids=("one-short", "null-query"))
@pytest.mark.parametrize("short", UID)
def test_capacity(env, short, query):
    ctx, lib, torch = env
    A, B = shape(THREE)
    want = expected(THREE)
    need = {op: len(want[op]) for op in UID}
    dA, dB = dev(torch, A), dev(torch, B)
    caps = {op: (0 if query else need[op] - 1) if op == short else need[op] for op in UID}
    bufs = {op: guarded(torch, caps[op]) for op in UID}
    s0 = stats(ctx)
    with pytest.raises(lib.CapacityError) as err:
        ctx.setop2_multi(dA, dB, ops=UID, out={op: bufs[op][:caps[op]] for op in UID})      # (an empty tensor goes in as NULL)
    assert err.value.code == lib.ERR_CAPACITY and err.value.needed == need
    assert stats(ctx) == (s0[0] + 1, s0[1])
    for op in UID:
        assert (host(bufs[op][caps[op]:]) == U64(G64)).all(), "guard words behind out_cap = %d of op %d were overwritten" % (caps[op], op)
    assert np.array_equal(host(dA), A) and np.array_equal(host(dB), B), "an input was modified"
    # ... and the call that fits, into the same buffers
    bufs[short] = guarded(torch, need[short])
    got = ctx.setop2_multi(dA, dB, ops=UID, out={op: bufs[op][:need[op]] for op in UID})
    for op in UID:
        assert np.array_equal(host(got[op]), want[op])
        assert (host(bufs[op][need[op]:]) == U64(G64)).all()


# ---- alignment ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", (THREE, "straddle-every-boundary"))
def test_odd_slots_inside_one_slab(env, name):
    """inputs and outputs start on odd 8-byte slots of one 16-byte aligned device slab, back to back behind hostile guard
    words: in front of a stream its first code, behind it its last code + 1"""
    ctx, lib, torch = env
    A, B = shape(name)
    want = expected(name)
    pos, at = {}, 129                                                # (odd)
    img = []
    for key, n in (("A", len(A)), ("B", len(B))) + tuple((op, len(want[op])) for op in UID):
        at += (at + 1) % 2                                           # the next odd slot
        pos[key] = (at, n)
        at += n + 3
    total = at + 128
    img = np.full(total, G64, dtype=U64)
    for key, x in (("A", A), ("B", B)):
        s, n = pos[key]
        img[s - 3:s] = x[0]
        img[s:s + n] = x
        img[s + n:s + n + 3] = x[-1] + U64(1)
    slab = dev(torch, img)
    assert slab.data_ptr() % 16 == 0
    view = lambda key: slab[pos[key][0]:pos[key][0] + pos[key][1]]
    assert all(view(k).data_ptr() % 16 == 8 for k in pos)
    s0 = stats(ctx)
    got = ctx.setop2_multi(view("A"), view("B"), ops=UID, out={op: view(op) for op in UID})
    assert stats(ctx) == (s0[0] + 1, s0[1])
    after = host(slab)
    for op in UID:
        s, n = pos[op]
        assert got[op].data_ptr() == view(op).data_ptr() and len(got[op]) == n
        assert np.array_equal(after[s:s + n], want[op]), op
        img[s:s + n] = want[op]
    assert np.array_equal(after, img), "a word outside the outputs changed"


# ---- workspace ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", (THREE, BIG))
def test_workspace_contents_do_not_matter(name):
    """option ws_poison fills the arena with one byte before every call: four patterns; then the stale twin -- the same
    call on other values of identical lengths first, poisoning off, so that the case finds that call's words"""
    import torch
    from unikmer_amd import lib
    ctx = lib.Context(0)
    e3 = (ctx, lib, torch)
    try:
        for byte in (0x00, 0x55, 0xAA, 0xFF):
            with options(ctx, {"ws_poison": byte}):
                run_fused(e3, name, UID)
                assert ctx.stat("ws_poisoned_bytes") >= ctx.stat("workspace_bytes") > 0
        assert ctx.get_option("ws_poison") is None
        A, B = shape(name)
        oa, ob = thirds(len(A) + len(B) + 40000, 1 / 3, seed=0x0777)
        oa, ob = oa[:len(A)], ob[:len(B)]
        assert len(oa) == len(A) and len(ob) == len(B) and not np.array_equal(oa, A)
        from oracle import oracle as O
        other = ctx.setop2_multi(dev(torch, oa), dev(torch, ob), ops=UID)
        assert np.array_equal(host(other[OP_UNION]), O.union([oa, ob]))
        blocks = ctx.stat("workspace_blocks"), ctx.stat("workspace_bytes")
        run_fused(e3, name, UID)
        assert (ctx.stat("workspace_blocks"), ctx.stat("workspace_bytes")) == blocks, "the arena grew: not the same addresses"
    finally:
        ctx.close()


# ---- host arrays ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_numpy_inputs_and_outputs(env):
    ctx, lib, torch = env
    A, B = shape(THREE)
    want = expected(THREE)
    outs = {op: np.full(len(want[op]) + GUARD, G64, dtype=U64) for op in UID}
    s0 = stats(ctx)
    got = ctx.setop2_multi(np.array(A), np.array(B), ops=UID, out={op: outs[op][:len(want[op])] for op in UID})
    assert stats(ctx) == (s0[0] + 1, s0[1])
    for op in UID:
        assert isinstance(got[op], np.ndarray) and np.array_equal(got[op], want[op])
        assert (outs[op][len(want[op]):] == U64(G64)).all()
    # default outputs, and a size query on one of them
    got = ctx.setop2_multi(np.array(A), np.array(B), ops=(OP_INTER, OP_DIFF))
    assert np.array_equal(got[OP_INTER], want[OP_INTER]) and np.array_equal(got[OP_DIFF], want[OP_DIFF])
    with pytest.raises(lib.CapacityError) as err:
        ctx.setop2_multi(np.array(A), np.array(B), ops=(OP_INTER, OP_DIFF), out={OP_DIFF: np.empty(0, dtype=U64)})
    assert err.value.needed == {OP_INTER: len(want[OP_INTER]), OP_DIFF: len(want[OP_DIFF])}
