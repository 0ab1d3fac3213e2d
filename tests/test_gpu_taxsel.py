"""ukm_rank_pass / ukm_rfilter / ukm_tsplit and the `rfilter` / `tsplit` commands on the GPU.

Expected values come from the models: isPassed restated over dicts (tests/test_taxsel_cpu.py: is_passed, used here with
a taxonomy of two trees, merged ids and ranks by depth) and np.argsort(taxids, kind="stable") -- never from the library.
Every comparison is bit-exact.  The conditions the issue puts on the inputs (every filter keeps and drops something, the
walk of -n meets each of its exits, the <= of the walk against the < of the node itself) are asserted on the model's
answers before the library is called.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import splitmix64, synth_tree
from test_taxsel_cpu import FILTERS, NORANKS, RANK_FILE, RANK_IDS, RANKS, is_passed, to_rank_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")
TILE = 2048  # records per tile of the selection kernel and of the split kernel
SIZES = [0, 1, 7, 8, 9, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
GUARD64, GUARD32 = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5

pytestmark = pytest.mark.gpu


# ---- the taxonomy of the tests -------------------------------------------------------------------------------------------
def build_taxonomy():
    """tree 1: the complete 3-ary tree of depth 6 (1093 nodes, root 1), ranks RANKS[depth].  Tree 2: a binary tree of depth 7
    (255 nodes, root 2000), ranks RANKS[4 + depth].  A splitmix64-chosen tenth of the nodes is `no rank` / `clade`; the forced
    cases are listed below.  Returns (parent, rank, merged) as dicts."""
    child, par = synth_tree(depth=6, arity=3)
    assert len(child) == 1093
    parent = {int(c): int(p) for c, p in zip(child, par)}
    depth = {1: 0}
    for c in range(2, 1094):
        depth[c] = depth[parent[c]] + 1
    rank = {c: RANKS[depth[c]] for c in parent}
    for i in range(255):
        t = 2000 + i
        parent[t] = t if i == 0 else 2000 + (i - 1) // 2
        depth[t] = 0 if i == 0 else depth[parent[t]] + 1
        rank[t] = RANKS[4 + depth[t]]
    ids = np.array(sorted(parent), dtype=np.uint64)
    h = splitmix64(ids + np.uint64(12345))
    for t, x in zip(ids.tolist(), h.tolist()):
        if x % 10 == 0:
            rank[t] = NORANKS[(x >> 8) & 1]
    # the forced cases
    rank.update({1: "domain", 3: "kingdom", 5: "phylum", 7: "phylum"})
    rank.update({14: "no rank", 41: "clade", 122: "no rank"})   # a chain of three below 5 (phylum): 122 -> 41 -> 14 -> 5
    rank[2] = "no rank"                                          # a no-rank child of node 1
    rank[8] = "no rank"                                          # its parent 3 is a kingdom
    rank.update({2000: "no rank", 2001: "clade"})                # the second tree: its root, and a child of the root
    del rank[40], rank[2010]                                     # nodes without a known rank (rank id 0)
    merged = {3000: 7, 3001: 122, 3002: 2500, 3003: 1, 3004: 2001}    # 2500 is absent
    return parent, rank, merged


TAX = build_taxonomy()
SIZE = 3005                                                      # the largest id of the dumps + 1
UNIVERSE = np.array(list(range(0, SIZE + 6)) + sorted(TAX[2]) + [1, 7, 2000, 0xFFFFFFFF, 1 << 31], dtype=np.uint32)


def load_tax(ctx, with_ranks=True):
    parent, rank, merged = TAX
    child = np.array(sorted(parent), dtype=np.uint32)
    ctx.taxonomy_load(child, np.array([parent[int(c)] for c in child], dtype=np.uint32),
                      np.array(sorted(merged), dtype=np.uint32), np.array([merged[m] for m in sorted(merged)], dtype=np.uint32))
    if with_ranks:
        named = np.array(sorted(rank), dtype=np.uint32)
        ctx.taxonomy_set_ranks(named, np.array([RANK_IDS[rank[int(t)]] for t in named], dtype=np.uint8))


@pytest.fixture(scope="module")
def env():
    from unikmer_amd import lib
    ctx = lib.Context(0)
    load_tax(ctx)
    yield lib, ctx
    ctx.close()


_model_cache = {}


def model_pass(name):
    """{taxid: kept} over UNIVERSE, computed once per filter"""
    if name not in _model_cache:
        _model_cache[name] = {int(t): is_passed(TAX, FILTERS[name], int(t)) for t in UNIVERSE}
    return _model_cache[name]


def _dev(x, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype).view({np.uint64: np.int64, np.uint32: np.int32, np.uint8: np.uint8}[dtype])).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype) if hasattr(t, "cpu") else np.asarray(t)


# ---- the model's answers have the shape the issue asks for -------------------------------------------------------------------
def test_model_conditions():
    parent, rank, merged = TAX
    assert len(parent) == 1093 + 255 and len(set(rank.values())) == len(RANKS) + len(NORANKS)
    unordered = [t for t in parent if rank.get(t) in NORANKS]
    assert 100 < len(unordered) < 200
    for name in FILTERS:
        m = model_pass(name)
        kept = sum(m[t] for t in parent)
        print("%-12s keeps %4d of %d nodes" % (name, kept, len(parent)))
        assert 0 < kept < len(parent), name
    # unordered ranks that are not discarded: kept under -L, dropped under -H and under -E alone
    assert all(model_pass("L")[t] for t in unordered)
    assert not any(model_pass("H")[t] for t in unordered) and not any(model_pass("E")[t] for t in unordered)
    # -N -n -L phylum: every exit of the walk
    flt = FILTERS["N-n-L"]

    def why(t):
        tr = []
        return is_passed(TAX, flt, t, tr), tr[0]
    assert why(122) == (True, "walk:order")                     # 122 -> 41 -> 14 (all without order) -> 5: phylum == lower: <= keeps it
    assert why(5) == (False, "self") and rank[5] == "phylum"    # ... while the node whose OWN order is lower is dropped: <
    assert why(8) == (False, "walk:order")                      # its parent 3 is a kingdom: above lower
    assert why(2) == (False, "walk:parent1")
    assert why(2001) == (False, "walk:root") and why(2000) == (False, "walk:root")
    assert why(3001) == (True, "walk:order") and why(3004) == (False, "walk:root")      # merged ids walk from their targets
    assert why(3002) == (False, "absent") and why(40) == (False, "self")
    walked = [t for t in parent if why(t)[1].startswith("walk")]
    assert sum(why(t)[0] for t in walked) > 10 and sum(not why(t)[0] for t in walked) > 5
    # -R compares the record's taxid as given: the merged id of the discarded root passes
    assert not model_pass("R-other")[7] and model_pass("R-other")[3000] and model_pass("none")[3003] and not model_pass("R")[1]


# ---- ukm_rank_pass -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FILTERS))
def test_rank_pass(env, name):
    lib, ctx = env
    m = model_pass(name)
    want = np.array([m[int(t)] for t in UNIVERSE], dtype=np.uint8)
    f = to_rank_filter(lib, FILTERS[name])
    got = ctx.rank_pass(f, UNIVERSE)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(int(UNIVERSE[i]), int(want[i])) for i in bad[:10]]
    assert np.array_equal(_host(ctx.rank_pass(f, _dev(UNIVERSE, np.uint32)), np.uint8), want)


# ---- ukm_rfilter ---------------------------------------------------------------------------------------------------------------
POOL = np.array(sorted(TAX[0]) + sorted(TAX[2]) + [0, 1500, 2600, 2999, SIZE, SIZE + 5, 1 << 31, 0xFFFFFFFF], dtype=np.uint32)


def records(n, seed):
    i = np.arange(n, dtype=np.uint64)
    codes = splitmix64(i + np.uint64(seed << 32)) >> np.uint64(2)
    tax = POOL[(splitmix64(i + np.uint64((seed + 1) << 32)) % np.uint64(len(POOL))).astype(np.int64)]
    return codes, tax


def model_mask(name, tax):
    m = model_pass(name)
    return np.fromiter((m[t] for t in tax.tolist()), dtype=bool, count=len(tax))


@pytest.mark.parametrize("n", SIZES)
def test_rfilter_sizes(env, n):
    lib, ctx = env
    codes, tax = records(n, 3)
    for name in sorted(FILTERS):
        keep = model_mask(name, tax)
        gk, gt = ctx.rfilter(codes, to_rank_filter(lib, FILTERS[name]), taxids=tax)
        assert np.array_equal(gk, codes[keep]) and np.array_equal(gt, tax[keep]), name


@pytest.mark.parametrize("force_ticket", [0, 1])
def test_rfilter_many_tiles(env, force_ticket):
    lib, ctx = env
    n = 40 * TILE - 3
    codes, tax = records(n, 5)
    ctx.set_option("force_ticket", force_ticket)
    try:
        for name in ("N-n-L", "E+H", "none"):
            keep = model_mask(name, tax)
            assert 0 < int(keep.sum()) < n
            dk, dt = ctx.rfilter(_dev(codes, np.uint64), to_rank_filter(lib, FILTERS[name]), taxids=_dev(tax, np.uint32))
            assert np.array_equal(_host(dk, np.uint64), codes[keep]) and np.array_equal(_host(dt, np.uint32), tax[keep])
    finally:
        ctx.set_option("force_ticket", None)


def test_rfilter_file_taxid(env):
    """taxids=None: every record carries file_taxid -- a copy or an empty result"""
    lib, ctx = env
    codes, _ = records(TILE + 9, 7)
    m = model_pass("N-n-L")
    f = to_rank_filter(lib, FILTERS["N-n-L"])
    for t in (122, 3001, 365, 5, 2, 2001, 0, 3002, SIZE + 100, 0xFFFFFFFF, 64, 63):
        want = is_passed(TAX, FILTERS["N-n-L"], t)
        assert want == m.get(t, want)
        got = ctx.rfilter(codes, f, taxids=int(t))
        assert np.array_equal(got, codes if want else codes[:0]), t
    assert is_passed(TAX, FILTERS["N-n-L"], 122) and not is_passed(TAX, FILTERS["N-n-L"], 2)


def test_rfilter_capacity(env):
    """the size query with NULL outputs; out_cap = needed - 1: UKM_ERR_CAPACITY, *n_out = needed, nothing behind out_cap touched"""
    import torch
    lib, ctx = env
    n = 3 * TILE + 5
    codes, tax = records(n, 9)
    keep = model_mask("L", tax)
    need = int(keep.sum())
    assert TILE < need < n
    f = to_rank_filter(lib, FILTERS["L"])
    m = C.c_uint64()
    rc = ctx.L.ukm_rfilter(ctx.h, codes.ctypes.data, tax.ctypes.data, 0, n, C.addressof(f), None, None, 0, C.byref(m))
    assert rc == lib.ERR_CAPACITY and m.value == need
    dk, dt = _dev(codes, np.uint64), _dev(tax, np.uint32)
    ok = torch.full((need + 64,), GUARD64 - (1 << 64), dtype=torch.int64, device="cuda")
    ot = torch.full((need + 64,), GUARD32 - (1 << 32), dtype=torch.int32, device="cuda")
    rc = ctx.L.ukm_rfilter(ctx.h, dk.data_ptr(), dt.data_ptr(), 0, n, C.addressof(f), ok.data_ptr(), ot.data_ptr(), need - 1, C.byref(m))
    assert rc == lib.ERR_CAPACITY and m.value == need
    assert (_host(ok, np.uint64)[need - 1:] == GUARD64).all() and (_host(ot, np.uint32)[need - 1:] == GUARD32).all()
    rc = ctx.L.ukm_rfilter(ctx.h, dk.data_ptr(), dt.data_ptr(), 0, n, C.addressof(f), ok.data_ptr(), ot.data_ptr(), need, C.byref(m))
    assert rc == lib.OK and m.value == need
    assert np.array_equal(_host(ok, np.uint64)[:need], codes[keep]) and np.array_equal(_host(ot, np.uint32)[:need], tax[keep])
    assert (_host(ok, np.uint64)[need:] == GUARD64).all() and (_host(ot, np.uint32)[need:] == GUARD32).all()
    # host arrays
    hk, ht = np.full(need + 8, GUARD64, dtype=np.uint64), np.full(need + 8, GUARD32, dtype=np.uint32)
    rc = ctx.L.ukm_rfilter(ctx.h, codes.ctypes.data, tax.ctypes.data, 0, n, C.addressof(f), hk.ctypes.data, ht.ctypes.data, need - 1, C.byref(m))
    assert rc == lib.ERR_CAPACITY and m.value == need and (hk[need - 1:] == GUARD64).all() and (ht[need - 1:] == GUARD32).all()


def test_rfilter_workspace_poison(env):
    lib, ctx = env
    codes, tax = records(5 * TILE + 1, 11)
    f = to_rank_filter(lib, FILTERS["N-n-L"])
    keep = model_mask("N-n-L", tax)
    try:
        for poison in (0, 255):
            ctx.set_option("ws_poison", poison)
            gk, gt = ctx.rfilter(codes, f, taxids=tax)
            assert np.array_equal(gk, codes[keep]) and np.array_equal(gt, tax[keep]), poison
            assert np.array_equal(ctx.rank_pass(f, tax), keep.astype(np.uint8)), poison
    finally:
        ctx.set_option("ws_poison", None)


def test_ranks_come_and_go_with_the_taxonomy():
    from unikmer_amd import lib
    ctx = lib.Context(0)
    try:
        codes, tax = records(100, 13)
        f = to_rank_filter(lib, FILTERS["L"])

        def refused():
            for call in (lambda: ctx.rfilter(codes, f, taxids=tax), lambda: ctx.rank_pass(f, tax)):
                with pytest.raises(lib.UkmError) as e:
                    call()
                assert e.value.code == lib.ERR_NO_TAXONOMY
        refused()                                                # no taxonomy at all
        with pytest.raises(lib.UkmError) as e:
            ctx.taxonomy_set_ranks(np.array([1], dtype=np.uint32), np.array([1], dtype=np.uint8))
        assert e.value.code == lib.ERR_NO_TAXONOMY
        load_tax(ctx, with_ranks=False)
        refused()                                                # a taxonomy without ranks
        load_tax(ctx)
        keep = model_mask("L", tax)
        assert np.array_equal(ctx.rfilter(codes, f, taxids=tax)[0], codes[keep])
        for bad in (1500, 3000, SIZE + 7):                       # absent, a merged id, beyond the table: not nodes
            with pytest.raises(lib.UkmError) as e:
                ctx.taxonomy_set_ranks(np.array([1, bad], dtype=np.uint32), np.array([3, 3], dtype=np.uint8))
            assert e.value.code == lib.ERR_INVALID
        assert np.array_equal(ctx.rfilter(codes, f, taxids=tax)[0], codes[keep])       # nothing changed
        load_tax(ctx, with_ranks=False)                          # a second load drops the ranks
        refused()
    finally:
        ctx.close()


# ---- ukm_tsplit ----------------------------------------------------------------------------------------------------------------
def split_case(n, pattern):
    i = np.arange(n, dtype=np.uint64)
    codes = splitmix64(i + np.uint64(77 << 32)) % np.uint64(1000)            # unsorted, with repeats: stability shows
    r = splitmix64(i + np.uint64(78 << 32))
    if pattern == "one":
        tax = np.full(n, 5, dtype=np.uint32)
    elif pattern == "distinct":
        tax = ((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)     # an odd multiplier: a bijection
    elif pattern == "37":
        tax = (splitmix64(r % np.uint64(37)) >> np.uint64(35)).astype(np.uint32)
    elif pattern == "extremes":
        tax = np.array([0, 0xFFFFFFFF, 5, 1 << 31, 1], dtype=np.uint32)[(r % np.uint64(5)).astype(np.int64)]
    else:  # "boundaries": sorted, the groups are 2047 records, 1 record, the rest -- heads at sorted positions 0, 2047, 2048
        tax = np.where(np.arange(n) < 2047, 10, np.where(np.arange(n) < 2048, 20, 30)).astype(np.uint32)
        tax = tax[np.argsort(r, kind="stable")]
    return codes, tax


def model_split(codes, tax):
    order = np.argsort(tax, kind="stable")
    st = tax[order]
    heads = np.flatnonzero(np.r_[True, st[1:] != st[:-1]]) if len(tax) else np.empty(0, dtype=np.int64)
    return codes[order], st[heads], np.r_[heads, len(tax)].astype(np.uint64) if len(tax) else np.empty(0, dtype=np.uint64)


PATTERNS = ["one", "distinct", "37", "extremes", "boundaries"]


@pytest.mark.parametrize("n", SIZES)
def test_tsplit_sizes(env, n):
    lib, ctx = env
    for pattern in PATTERNS:
        codes, tax = split_case(n, pattern)
        wk, wt, wo = model_split(codes, tax)
        if pattern == "distinct":
            assert len(wt) == n
        if pattern == "boundaries" and n > TILE:
            assert wo.tolist() == [0, TILE - 1, TILE, n]
        gk, gt, go = ctx.tsplit(codes, tax)
        assert np.array_equal(gk, wk) and np.array_equal(gt, wt) and np.array_equal(go, wo), (n, pattern)


@pytest.mark.parametrize("force_ticket", [0, 1])
def test_tsplit_many_tiles_device(env, force_ticket):
    lib, ctx = env
    n = 40 * TILE - 3
    ctx.set_option("force_ticket", force_ticket)
    try:
        for pattern in ("37", "distinct", "extremes"):
            codes, tax = split_case(n, pattern)
            wk, wt, wo = model_split(codes, tax)
            gk, gt, go = ctx.tsplit(_dev(codes, np.uint64), _dev(tax, np.uint32))
            assert np.array_equal(_host(gk, np.uint64), wk) and np.array_equal(_host(gt, np.uint32), wt), pattern
            assert np.array_equal(_host(go, np.uint64), wo), pattern
    finally:
        ctx.set_option("force_ticket", None)


def test_tsplit_capacity(env):
    import torch
    lib, ctx = env
    n = 3 * TILE + 5
    codes, tax = split_case(n, "37")
    wk, wt, wo = model_split(codes, tax)
    groups = len(wt)
    assert groups == 37
    g = C.c_uint64()
    rc = ctx.L.ukm_tsplit(ctx.h, codes.ctypes.data, tax.ctypes.data, n, None, 0, None, None, 0, C.byref(g))      # the size query
    assert rc == lib.ERR_CAPACITY and g.value == groups
    dk, dt = _dev(codes, np.uint64), _dev(tax, np.uint32)

    def guarded():
        return (torch.full((n + 64,), GUARD64 - (1 << 64), dtype=torch.int64, device="cuda"),
                torch.full((groups + 64,), GUARD32 - (1 << 32), dtype=torch.int32, device="cuda"),
                torch.full((groups + 65,), GUARD64 - (1 << 64), dtype=torch.int64, device="cuda"))
    # too few groups: group_taxids[group_cap], group_off[group_cap + 1]
    ok, gt, go = guarded()
    rc = ctx.L.ukm_tsplit(ctx.h, dk.data_ptr(), dt.data_ptr(), n, ok.data_ptr(), n, gt.data_ptr(), go.data_ptr(), groups - 1, C.byref(g))
    assert rc == lib.ERR_CAPACITY and g.value == groups
    assert (_host(ok, np.uint64)[n:] == GUARD64).all() and (_host(gt, np.uint32)[groups - 1:] == GUARD32).all()
    assert (_host(go, np.uint64)[groups:] == GUARD64).all()
    # too few records
    ok, gt, go = guarded()
    rc = ctx.L.ukm_tsplit(ctx.h, dk.data_ptr(), dt.data_ptr(), n, ok.data_ptr(), n - 1, gt.data_ptr(), go.data_ptr(), groups, C.byref(g))
    assert rc == lib.ERR_CAPACITY and g.value == groups
    assert (_host(ok, np.uint64)[n - 1:] == GUARD64).all() and (_host(gt, np.uint32)[groups:] == GUARD32).all()
    assert (_host(go, np.uint64)[groups + 1:] == GUARD64).all()
    # exactly enough
    ok, gt, go = guarded()
    rc = ctx.L.ukm_tsplit(ctx.h, dk.data_ptr(), dt.data_ptr(), n, ok.data_ptr(), n, gt.data_ptr(), go.data_ptr(), groups, C.byref(g))
    assert rc == lib.OK and g.value == groups
    assert np.array_equal(_host(ok, np.uint64)[:n], wk) and (_host(ok, np.uint64)[n:] == GUARD64).all()
    assert np.array_equal(_host(gt, np.uint32)[:groups], wt) and (_host(gt, np.uint32)[groups:] == GUARD32).all()
    assert np.array_equal(_host(go, np.uint64)[:groups + 1], wo) and (_host(go, np.uint64)[groups + 1:] == GUARD64).all()
    # host arrays, one group short and one record short
    hk, ht, ho = np.full(n + 8, GUARD64, dtype=np.uint64), np.full(groups + 8, GUARD32, dtype=np.uint32), np.full(groups + 9, GUARD64, dtype=np.uint64)
    for out_cap, group_cap in ((n, groups - 1), (n - 1, groups)):
        rc = ctx.L.ukm_tsplit(ctx.h, codes.ctypes.data, tax.ctypes.data, n, hk.ctypes.data, out_cap, ht.ctypes.data, ho.ctypes.data, group_cap, C.byref(g))
        assert rc == lib.ERR_CAPACITY and g.value == groups
        assert (hk[out_cap:] == GUARD64).all() and (ht[group_cap:] == GUARD32).all() and (ho[group_cap + 1:] == GUARD64).all()
    # n == 0: UKM_OK, no groups, group_off untouched
    rc = ctx.L.ukm_tsplit(ctx.h, None, None, 0, hk.ctypes.data, len(hk), ht.ctypes.data, ho.ctypes.data, len(ht), C.byref(g))
    assert rc == lib.OK and g.value == 0 and (ho == GUARD64).all()


def test_tsplit_poison_and_arguments(env):
    lib, ctx = env
    codes, tax = split_case(5 * TILE + 1, "37")
    wk, wt, wo = model_split(codes, tax)
    try:
        for poison in (0, 255):
            ctx.set_option("ws_poison", poison)
            gk, gt, go = ctx.tsplit(codes, tax)
            assert np.array_equal(gk, wk) and np.array_equal(gt, wt) and np.array_equal(go, wo), poison
    finally:
        ctx.set_option("ws_poison", None)
    with pytest.raises(lib.UkmError) as e:
        ctx.tsplit(codes, None)
    assert e.value.code == lib.ERR_INVALID


# ---- through the binary ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    from unikmer_amd import build
    build.build()

    def run(*args, stdin=None):
        p = subprocess.run([BIN] + [str(a) for a in args], input=stdin, capture_output=True)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout.decode()
    return run


def canonical_code(kmer):
    code = lambda s: int("".join(str("ACGT".index(b)) for b in s), 4)
    return min(code(kmer), code(kmer[::-1].translate(str.maketrans("ACGT", "TGCA"))))


@pytest.fixture(scope="module")
def cli_data(cli, tmp_path_factory):
    """nodes.dmp with a rank column, merged.dmp, a rank file, and .unik files with per-record taxids written by `dump -K`"""
    d = tmp_path_factory.mktemp("taxsel")
    parent, rank, merged = TAX
    (d / "nodes.dmp").write_text("".join("%d\t|\t%d\t|\t%s\t|\t\t|\n" % (t, parent[t], rank.get(t, "").upper() if t % 2 else rank.get(t, ""))
                                         for t in sorted(parent)))
    (d / "merged.dmp").write_text("".join("%d\t|\t%d\t|\n" % (a, merged[a]) for a in sorted(merged)))
    (d / "ranks.txt").write_text(RANK_FILE)
    n = 700
    r = splitmix64(np.arange(n, dtype=np.uint64) + np.uint64(4242))
    kmers = sorted({"".join("ACGT"[(int(x) >> (2 * j)) & 3] for j in range(13)) for x in r}, key=canonical_code)
    kmers = [k for i, k in enumerate(kmers) if i == 0 or canonical_code(k) != canonical_code(kmers[i - 1])]
    pool = [t for t in POOL.tolist() if t < (1 << 31)]
    tax = [pool[int(x) % len(pool)] for x in splitmix64(np.arange(len(kmers), dtype=np.uint64) + np.uint64(777))]
    text = "".join("%s\t%d\n" % kt for kt in zip(kmers, tax)).encode()
    cli("dump", "-K", "-s", "-o", d / "sorted", stdin=text)                     # ascending canonical codes
    half = len(kmers) // 2
    order = np.argsort(splitmix64(np.arange(len(kmers), dtype=np.uint64))).tolist()
    rows = [(kmers[i], tax[i]) for i in order]
    cli("dump", "-K", "-o", d / "a", stdin="".join("%s\t%d\n" % kt for kt in rows[:half]).encode())
    cli("dump", "-K", "-o", d / "b", stdin="".join("%s\t%d\n" % kt for kt in rows[half:]).encode())
    return d


def view_t(cli, f):
    return [(k, int(t)) for k, t in (line.split("\t") for line in cli("view", "-t", f).splitlines())]


def test_cli_rfilter(cli, cli_data):
    d = cli_data
    a, b = view_t(cli, str(d / "a.unik")), view_t(cli, str(d / "b.unik"))
    assert len(a) > 300 and len(b) > 300
    flt = FILTERS["N-n-L"]
    cli("rfilter", "-n", "-L", "Phylum", "-r", d / "ranks.txt", "--data-dir", d, d / "a.unik", "-o", d / "fa")
    want = [kt for kt in a if is_passed(TAX, flt, kt[1])]
    assert 0 < len(want) < len(a) and view_t(cli, str(d / "fa.unik")) == want
    cli("rfilter", "-n", "-L", "phylum", "--data-dir", d, d / "a.unik", d / "b.unik", "-o", d / "fab")       # <data-dir>/ranks.txt
    assert view_t(cli, str(d / "fab.unik")) == [kt for kt in a + b if is_passed(TAX, flt, kt[1])]
    cli("rfilter", "-E", "class", "-E", "genus", "-r", d / "ranks.txt", "--data-dir", d, d / "a.unik", d / "b.unik", "-o", d / "fe")
    assert view_t(cli, str(d / "fe.unik")) == [kt for kt in a + b if is_passed(TAX, FILTERS["E"], kt[1])]
    cli("rfilter", "-B", "family,clade", "-r", d / "ranks.txt", "--data-dir", d, d / "b.unik", "-o", d / "fb")
    assert view_t(cli, str(d / "fb.unik")) == [kt for kt in b if is_passed(TAX, FILTERS["B"], kt[1])]
    cli("rfilter", "-R", "--root-taxid", 7, "-r", d / "ranks.txt", "--data-dir", d, d / "b.unik", "-o", d / "fr")
    assert view_t(cli, str(d / "fr.unik")) == [kt for kt in b if is_passed(TAX, FILTERS["R-other"], kt[1])]
    ranks = cli("rfilter", "--list-ranks", "-r", d / "ranks.txt", "--data-dir", d).splitlines()
    assert ranks[:len(RANKS)] == RANKS and set(ranks[len(RANKS):]) == set(NORANKS)


def test_cli_tsplit(cli, cli_data):
    d = cli_data
    rows = view_t(cli, str(d / "sorted.unik"))
    out = d / "split"
    cli("tsplit", "-O", out, "-o", "pre", d / "sorted.unik")
    groups = {}
    for k, t in rows:
        groups.setdefault(t, []).append(k)
    assert len(groups) > 50
    assert set(os.listdir(out)) == {"pre.taxid-%d.k13.unik" % t for t in groups}
    seen = 0
    for t, kmers in groups.items():
        f = str(out / ("pre.taxid-%d.k13.unik" % t))
        cols = cli("info", "-a", "--symbol-true", "yes", "--symbol-false", "no", f).splitlines()[1].split("\t")
        # file k canonical hashed scaled include-taxid global-taxid sorted compact gzipped version number description
        assert cols[1:8] == ["13", "yes", "no", "no", "no", str(t) if t else "", "yes"] and cols[11] == str(len(kmers)), cols
        assert cli("view", f).splitlines() == kmers                              # the group's k-mers in input order
        seen += len(kmers)
    assert seen == len(rows)
    # a directory that is not empty: a warning without --force, emptied with it
    (out / "stale.txt").write_text("x")
    cli("tsplit", "-O", out, "-o", "pre", "--force", d / "sorted.unik")
    assert set(os.listdir(out)) == {"pre.taxid-%d.k13.unik" % t for t in groups}
