"""ukm_screen on the GPU: per-record windows, hits and taxid LCA, compared for exact equality with tests/screen_model.py (windows
from the CPU oracle, membership a dict, the LCA the left fold of the oracle's pairwise LCA).  Shapes sit on, beside and away from
the edges of the reduction kernel's tile T (unikmer_amd/csrc/ukm_screen.h), on both routes (option "map_sorted" 0 / 1)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import screen_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "unikmer_amd", "csrc", "ukm_screen.h")).read()
T = int(re.search(r"constexpr int SCREEN_NT = (\d+);", _SRC).group(1)) * int(re.search(r"constexpr int SCREEN_VT = (\d+);", _SRC).group(1))

pytestmark = pytest.mark.gpu
ROUTES = [0, 1]
U64MAX = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def env():
    """(lib, ctx with a random forest loaded, oracle, oracle taxonomy of the same forest, the taxid pool)"""
    from unikmer_amd import lib
    from oracle import oracle
    ctx = lib.Context(0)
    child, parent, m_old, m_new, pool = M.random_forest(np.random.default_rng(77))
    ctx.taxonomy_load(child, parent, m_old, m_new)
    yield lib, ctx, oracle, oracle.Taxonomy(child, parent, m_old, m_new), pool
    ctx.close()


def _records(rng, lens, alphabet=b"ACGT"):
    lens = np.asarray(lens, dtype=np.int64)
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    bases = np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), int(off[-1]))].copy()
    return bases, off


def _set_of(rng, codes, pool, extra=50):
    """sorted set of the given codes plus `extra` random ones, a taxid from the pool for each"""
    keys = np.unique(np.concatenate([np.asarray(codes, dtype=np.uint64), rng.integers(0, 1 << 62, extra, dtype=np.uint64)]))
    tx = np.array([pool[int(i)] for i in rng.integers(0, len(pool), len(keys))], dtype=np.uint32)
    return keys, tx


def _half(rng, wins):
    """about half of the distinct window values"""
    allc = np.unique(np.array([c for w in wins for c in w], dtype=np.uint64))
    pick = rng.random(len(allc)) < 0.5
    pick[:1] = True      # (k = 1 has two values: never none of them)
    return allc[pick]


def _dev(x, dtype):
    import torch
    view = {np.uint64: np.int64, np.uint32: np.int32, np.uint8: np.uint8}[dtype]
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype).view(view).copy()).cuda()


def _host(t, dtype=np.uint32):
    return t.cpu().numpy().view(dtype) if hasattr(t, "cpu") else np.asarray(t)


def _check(env, route, bases, off, k, keys, tx, canonical=True, circular=False, hashed=False, wins=None):
    """one call with and one without taxids against the model; returns the model's (win, hit, lca)"""
    lib, ctx, O, tax, pool = env
    if wins is None:
        wins = M.windows(O, bases, off, k, canonical, circular, hashed)
    want = M.screen(wins, M.first_taxids(keys, tx), tax)
    ctx.set_option("map_sorted", route)
    try:
        win, hit, lca = ctx.screen(bases, off, k, keys, tx, canonical=canonical, circular=circular, hashed=hashed)
        win2, hit2, none = ctx.screen(bases, off, k, keys, canonical=canonical, circular=circular, hashed=hashed)
    finally:
        ctx.set_option("map_sorted", None)
    assert none is None
    for name, got, exp in (("win", win, want[0]), ("hit", hit, want[1]), ("lca", lca, want[2]), ("win no taxids", win2, want[0]),
                           ("hit no taxids", hit2, want[1])):
        got = np.asarray(got)
        bad = np.nonzero(got != exp)[0]
        assert len(got) == len(exp) and len(bad) == 0, (name, route, k, bad[:5].tolist(), got[bad[:5]].tolist(), exp[bad[:5]].tolist())
    return want


def _w(n, k):
    """bases of a record with n windows"""
    return n + k - 1 if n else 0


# ---- record edges on tile edges -------------------------------------------------------------------------------------------
EDGE_SHAPES = {
    "T-1,T,T+1,2T": lambda k: [_w(T - 1, k), _w(T, k), _w(T + 1, k), _w(2 * T, k)],
    "3T+5 between short": lambda k: [_w(3, k), _w(1, k), _w(3 * T + 5, k), _w(2, k), _w(1, k)],
    "boundary at every edge": lambda k: [_w(T, k)] * 4,
    "no boundary at an edge": lambda k: [_w(T + 7, k), _w(T - 3, k), _w(T + 11, k), _w(500, k)],
    "one record": lambda k: [_w(2 * T + 17, k)],
    "one short record": lambda k: [_w(5, k)],
}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", sorted(EDGE_SHAPES))
def test_record_edges_on_tile_edges(env, route, shape):
    k = 21
    rng = np.random.default_rng(sorted(EDGE_SHAPES).index(shape) + 5)
    bases, off = _records(rng, EDGE_SHAPES[shape](k))
    wins = M.windows(env[2], bases, off, k)
    keys, tx = _set_of(rng, _half(rng, wins), env[4])
    want = _check(env, route, bases, off, k, keys, tx, wins=wins)
    assert want[0].sum() > 0 and want[1].sum() > 0


# ---- short and empty records ------------------------------------------------------------------------------------------------
def _short_shapes(k):
    mix = [0, k - 1, k, k + 1]
    return {
        "mixed front and end": mix + [300, 0, k - 1] + mix[::-1] + [_w(T + 3, k)] + mix,
        "empty run at a tile edge": [_w(T, k)] + [0] * (T + 50) + [_w(100, k)] + [k - 1] * (T + 50) + [_w(7, k)],
        "empty run inside a tile": [_w(100, k)] + [0] * (T + 50) + [_w(100, k), 0, 0, _w(1, k)] + [0] * 300,
        "runs of one-window records": [k] * (T + 300) + [_w(40, k)] + [k, 0, k - 1] * 200,
        "all shorter than k": [0, k - 1, 1, k - 1, 0] * 3,
        "one empty record": [0],
    }


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", sorted(_short_shapes(21)))
def test_short_and_empty_records(env, route, shape):
    k = 21
    rng = np.random.default_rng(sorted(_short_shapes(k)).index(shape) + 50)
    bases, off = _records(rng, _short_shapes(k)[shape])
    wins = M.windows(env[2], bases, off, k)
    keys, tx = _set_of(rng, _half(rng, wins), env[4])
    _check(env, route, bases, off, k, keys, tx, wins=wins)


@pytest.mark.parametrize("route", ROUTES)
def test_many_short_records(env, route):
    """5,000 reads of 40-120 bases at k = 31: dozens of records per tile, some shorter than k"""
    k = 31
    rng = np.random.default_rng(9)
    lens = rng.integers(40, 121, 5000)
    lens[rng.integers(0, 5000, 60)] = rng.integers(0, k, 60)
    bases, off = _records(rng, lens)
    wins = M.windows(env[2], bases, off, k)
    keys, tx = _set_of(rng, _half(rng, wins), env[4])
    want = _check(env, route, bases, off, k, keys, tx, wins=wins)
    assert (want[1] > 0).sum() > 4000 and (want[0] == 0).sum() >= 30


# ---- hit patterns -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("pattern", ["none", "all", "first", "last", "tile edges"])
def test_hit_patterns(env, route, pattern):
    k = 31
    rng = np.random.default_rng(21)
    bases, off = _records(rng, [_w(n, k) for n in (1, 2, 700, T - 703, 5, T + 1, 1, 2 * T - 6, 90)])
    wins = M.windows(env[2], bases, off, k)
    flat = [c for w in wins for c in w]
    if pattern == "none":
        codes = []
    elif pattern == "all":
        codes = flat
    elif pattern == "first":
        codes = [w[0] for w in wins if w]
    elif pattern == "last":
        codes = [w[-1] for w in wins if w]
    else:   # the windows either side of every tile edge
        codes = [flat[i] for e in range(T, len(flat), T) for i in (e - 1, e)]
    keys, tx = _set_of(rng, codes, env[4], extra=0 if pattern == "all" else 50)
    want = _check(env, route, bases, off, k, keys, tx, wins=wins)
    if pattern == "none":
        assert want[1].sum() == 0
    if pattern == "all":
        assert np.array_equal(want[0], want[1])


# ---- the set's edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_set_edges(env, route):
    lib, ctx, O, tax, pool = env
    k = 32
    rng = np.random.default_rng(31)
    bases, off = _records(rng, [100, 64, 64, _w(T + 9, k), 40])
    bases[100:164] = ord("A")          # poly-A: code 0
    bases[164:228] = ord("T")          # poly-T: code 2^64 - 1 when not canonical, 0 when canonical
    nodes = [t for t in pool if t][:6]
    for canonical in (True, False):
        wins = M.windows(O, bases, off, k, canonical)
        flat = [c for w in wins for c in w]
        assert 0 in flat and (canonical or U64MAX in flat)
        # no set, one code, the extreme codes, duplicated codes with different taxids (the first copy decides)
        _check(env, route, bases, off, k, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32), canonical, wins=wins)
        _check(env, route, bases, off, k, np.array([wins[3][5]], dtype=np.uint64), np.array([nodes[0]], dtype=np.uint32), canonical, wins=wins)
        _check(env, route, bases, off, k, np.array([0], dtype=np.uint64), np.array([nodes[1]], dtype=np.uint32), canonical, wins=wins)
        keys = np.array([0, 0, wins[3][0], wins[3][0], wins[3][0], wins[3][T], U64MAX, U64MAX], dtype=np.uint64)
        keys.sort()
        tx = np.array([nodes[i % len(nodes)] for i in range(len(keys))], dtype=np.uint32)
        want = _check(env, route, bases, off, k, keys, tx, canonical, wins=wins)
        assert want[1][1] == 33 and want[2][1] == tx[0]


# ---- window variants ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("k,hashed,canonical,circular", [(1, 0, 1, 0), (21, 0, 0, 0), (31, 0, 1, 1), (32, 0, 1, 0), (32, 0, 0, 1), (23, 1, 1, 0),
                                                         (51, 1, 0, 0), (51, 1, 1, 1), (21, 0, 1, 0)])
def test_window_variants(env, route, k, hashed, canonical, circular):
    rng = np.random.default_rng(100 + k + hashed)
    iupac = (k, hashed) == (21, 0) and canonical
    bases, off = _records(rng, [k - 1, T + 100, 0, k, 777, k + 1, 2 * T + 3], b"ACGTRYSWKMBDHVNacgtn" if iupac else b"ACGT")
    wins = M.windows(env[2], bases, off, k, bool(canonical), bool(circular), bool(hashed))
    keys, tx = _set_of(rng, _half(rng, wins), env[4])
    want = _check(env, route, bases, off, k, keys, tx, bool(canonical), bool(circular), bool(hashed), wins=wins)
    assert want[1].sum() > 0


# ---- taxonomy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_taxonomy_cases(env, route):
    """records whose hits carry chosen taxids: spanning two trees, one merged id (unmapped), a merged id and its target, an
    unknown id alone and among others, zero"""
    lib, ctx, O, tax, pool = env
    child, parent, m_old, m_new, _ = M.random_forest(np.random.default_rng(77))
    forest = M.Forest(child, parent, m_old, m_new)
    roots = [int(c) for c, p in zip(child, parent) if c == p]
    tree_of = lambda t: forest.path(t)[0]
    a = next(int(t) for t in child if tree_of(int(t)) == roots[0] and int(t) != roots[0])
    b = next(int(t) for t in child if tree_of(int(t)) == roots[1] and int(t) != roots[1])
    a2 = next(int(t) for t in child if tree_of(int(t)) == roots[0] and int(t) not in (roots[0], a))
    merged, target = int(m_old[0]), int(m_new[0])
    dead = int(m_old[-1])       # merged onto an id the taxonomy does not have
    unknown = 100000
    plans = [[a, b], [merged, merged, merged], [merged, target], [target, merged, a2], [unknown, unknown], [unknown, a], [a, 0, a], [0, 0],
             [a, a2, a], [dead, dead], [dead, a], [a]]
    k = 21
    rng = np.random.default_rng(41)
    # record i: len(plans[i]) hit windows spread over a record that crosses a tile edge when i is even
    lens = [_w(T + 30 if i % 2 == 0 else 60, k) for i in range(len(plans))]
    bases, off = _records(rng, lens)
    wins = M.windows(O, bases, off, k)
    codes, tx = [], []
    for w, plan in zip(wins, plans):
        at = np.linspace(0, len(w) - 1, len(plan)).astype(int)
        codes += [w[i] for i in at]
        tx += plan
    order = np.argsort(np.array(codes, dtype=np.uint64), kind="stable")
    keys, tx = np.array(codes, dtype=np.uint64)[order], np.array(tx, dtype=np.uint32)[order]
    assert len(np.unique(keys)) == len(keys)
    want = _check(env, route, bases, off, k, keys, tx, wins=wins)
    assert want[1].tolist() == [len(p) for p in plans]
    assert want[2].tolist() == [M.closed_lca(forest, p) for p in plans]
    assert want[2][0] == 0 and want[2][1] == merged and want[2][2] == target and want[2][4] == unknown and want[2][5] == 0


def test_taxids_without_taxonomy(env):
    lib, ctx, O, tax, pool = env
    fresh = lib.Context(0)
    try:
        bases, off = _records(np.random.default_rng(1), [100])
        keys, tx = np.array([5], dtype=np.uint64), np.array([1], dtype=np.uint32)
        with pytest.raises(lib.UkmError) as e:
            fresh.screen(bases, off, 21, keys, tx)
        assert e.value.code == lib.ERR_NO_TAXONOMY
        win, hit, lca = fresh.screen(bases, off, 21, keys, tx, lca=False)      # out_lca NULL while taxids are given: no taxonomy needed
        assert lca is None and win.tolist() == [80] and hit.tolist() == [0]
    finally:
        fresh.close()


# ---- pointer kinds, NULL outputs, workspace, repeat ------------------------------------------------------------------------------------
def _case(env, seed=61, k=21):
    rng = np.random.default_rng(seed)
    bases, off = _records(rng, [_w(T - 5, k), 3, _w(T + 40, k), 0, _w(33, k)])
    wins = M.windows(env[2], bases, off, k)
    keys, tx = _set_of(rng, _half(rng, wins), env[4])
    return bases, off, k, keys, tx, M.screen(wins, M.first_taxids(keys, tx), env[3])


@pytest.mark.parametrize("route", ROUTES)
def test_pointer_kinds_and_null_outputs(env, route):
    lib, ctx, O, tax, pool = env
    bases, off, k, keys, tx, want = _case(env)
    n = len(off) - 1
    host = dict(bases=bases, off=off, keys=keys, tx=tx)
    dev = dict(bases=_dev(bases, np.uint8), off=_dev(off, np.uint64), keys=_dev(keys, np.uint64), tx=_dev(tx, np.uint32))
    ctx.set_option("map_sorted", route)
    try:
        for mask in range(16):      # every mix of host and device inputs
            a = {name: (dev if (mask >> i) & 1 else host)[name] for i, name in enumerate(("bases", "off", "keys", "tx"))}
            for dev_out in (False, True):
                outs = tuple(_dev(np.full(n, 0xEE, dtype=np.uint32), np.uint32) if dev_out else np.full(n, 0xEE, dtype=np.uint32) for _ in range(3))
                got = ctx.screen(a["bases"], a["off"], k, a["keys"], a["tx"], outs=outs)
                for g, w in zip(got, want):
                    assert np.array_equal(_host(g), w), (mask, dev_out)
        for skip in range(3):       # each output NULL in turn
            outs = [np.full(n, 0xEE, dtype=np.uint32) for _ in range(3)]
            outs[skip] = None
            got = ctx.screen(bases, off, k, keys, tx, outs=tuple(outs))
            for i, (g, w) in enumerate(zip(got, want)):
                assert (g is None) if i == skip else np.array_equal(g, w), (skip, i)
        got = ctx.screen(bases, off, k, keys, tx, outs=(None, None, np.zeros(n, dtype=np.uint32)))
        assert np.array_equal(got[2], want[2])
    finally:
        ctx.set_option("map_sorted", None)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("byte", [0xAA, 0x00])
def test_workspace_contents_do_not_matter(env, route, byte):
    lib, ctx, O, tax, pool = env
    bases, off, k, keys, tx, want = _case(env, seed=62)
    ctx.set_option("map_sorted", route)
    ctx.set_option("ws_poison", byte)
    try:
        for _ in range(2):
            got = ctx.screen(bases, off, k, keys, tx)
            for g, w in zip(got, want):
                assert np.array_equal(g, w)
    finally:
        ctx.set_option("ws_poison", None)
        ctx.set_option("map_sorted", None)


@pytest.mark.parametrize("route", ROUTES)
def test_two_calls_of_different_lengths(env, route):
    lib, ctx, O, tax, pool = env
    ctx.set_option("map_sorted", route)
    try:
        for seed, k in ((63, 21), (64, 31), (63, 21)):
            bases, off, k, keys, tx, want = _case(env, seed=seed, k=k)
            for g, w in zip(ctx.screen(bases, off, k, keys, tx), want):
                assert np.array_equal(g, w)
    finally:
        ctx.set_option("map_sorted", None)


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors(env):
    lib, ctx, O, tax, pool = env
    bases, off, k, keys, tx, want = _case(env)
    n = len(off) - 1
    with pytest.raises(lib.UnsortedError):
        ctx.screen(bases, off, k, keys[::-1].copy(), tx)
    for bad_k, hashed in ((0, False), (33, False), (65, True)):
        with pytest.raises(lib.UkmError) as e:
            ctx.screen(bases, off, bad_k, keys, tx, hashed=hashed)
        assert e.value.code == lib.ERR_K
    bad = bases.copy()
    bad[int(off[2]) + 50] = ord("*")
    with pytest.raises(lib.IllegalBaseError):
        ctx.screen(bad, off, k, keys, tx)
    with pytest.raises(lib.IllegalBaseError):
        ctx.screen(bad, off, k, keys[:0], None)                  # also without a set
    out = np.zeros(n, dtype=np.uint32)
    L = ctx.L
    args = (bases.ctypes.data, off.ctypes.data, n, k, 1, 0, 0, keys.ctypes.data)
    assert L.ukm_screen(ctx.h, *args, None, len(keys), None, None, out.ctypes.data) == lib.ERR_INVALID      # out_lca without set_taxids
    assert L.ukm_screen(None, *args, None, len(keys), out.ctypes.data, None, None) == lib.ERR_INVALID
    assert L.ukm_screen(ctx.h, bases.ctypes.data, off.ctypes.data, 1 << 32, k, 1, 0, 0, keys.ctypes.data, None, len(keys), out.ctypes.data,
                        None, None) == lib.ERR_INVALID and b"split the records" in L.ukm_last_error()
    assert L.ukm_screen(ctx.h, None, None, 0, k, 1, 0, 0, None, None, 0, None, None, None) == lib.OK        # no records: nothing to do
    # the context still works
    for g, w in zip(ctx.screen(bases, off, k, keys, tx), want):
        assert np.array_equal(g, w)
