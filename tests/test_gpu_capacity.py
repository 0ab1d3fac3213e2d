"""The out_cap contract of include/unikmer_hip.h, for every entry point that produces output and every internal route:

  - a buffer that is too small returns UKM_ERR_CAPACITY and *n_out holds the size that is needed (the two-call idiom of
    INTEGRATION.md and lib.Context._coords: call, read the size, allocate, call again),
  - an exactly fitting buffer and the documented upper bound both succeed with the oracle's result, bit for bit,
  - nothing outside [0, out_cap) is written, whatever the call returns,
  - a failed call leaves the context (workspace, look-back control words, ticket state) fit for the next one.

Every output array of a call is the middle of one allocation [front guard | out_cap | back guard] filled with a sentinel.
The back guard is at least bound - out_cap + 64 elements long, so a kernel that ignored out_cap altogether would still
write inside memory this test owns.  out_cap == 0 passes NULL pointers (lib._ptr): the size query.

The case table below is evaluated by the CPU oracle alone in test_case_table_oracle_only (no GPU): 2 <= need < bound for
every case, so that need - 1, need and bound are three distinct capacities.  The entry points whose documented bound IS
the size (every record / window kept: ukm_unique in UKM_PLAIN mode, ukm_encode_kmers, ukm_nthash without a filter, the
one-stream forms of union / inter / diff) are marked `exact` and have need == bound.
"""
import functools

import numpy as np
import pytest

from conftest import splitmix64, synth_tree

SEED = 0x756E696B6D6572
FRONT = 64                      # elements of the front guard (256 / 512 bytes: the slice stays 16-byte aligned)
SENT = {np.dtype(np.uint64): 0xA5A5A5A55A5A5A5A, np.dtype(np.uint32): 0xA5A55A5A, np.dtype(np.uint8): 0xA5}
SIGNED = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}
U64, U32 = np.uint64, np.uint32

# records per tile, from the kernels' sources
TILE_SETOP = 512 * 19       # ukm_setop_kernels.h: SETOP_NT x SETOP_VT (plain keys; one taxid per file on both sides)
TILE_SETOP_TAX = 512 * 7    #                      SETOP_NT x SETOP_VT_TAX (per-record taxids)
TILE_SETOP_RANK = 512 * 12  #                      SETOP_NT x VT_RANK (the multiset re-run)
TILE_UNIQ = 512 * 16        # ukm_scan.hip: UNIQ_NT x UNIQ_VT (half of it for the chunk protocol)
TILE_UNIQ_TAX = 512 * 12    #               UNIQ_NT x UNIQ_VT_TAX
TILE_SELECT = 256 * 8       # ukm_select.hip: NT x VT
TILE_WIN = 2048             # ukm_win_common.h: ENC_WT windows per tile; MIN_MT of the minimizer kernel is the same

ROUTE_NONE, ROUTE_TREE, ROUTE_KWAY, ROUTE_PUNION, ROUTE_SRMERGE, ROUTE_SRCOMMON, ROUTE_PCOMMON, ROUTE_PLACE = range(8)
PLAIN, UNIQUE, REPEATED, REPEATED_CHUNK, SINGLETON = 0, 1, 2, 3, 4
OP_UNION, OP_INTER, OP_DIFF = 0, 1, 2
F_MIX_TAXID, F_CMP_TAXID = 2, 4


# ---- the oracle and the inputs, each made once ------------------------------------------------------------------------------
@functools.lru_cache(None)
def _oracle():
    from oracle import oracle as O
    child, parent = synth_tree(5, 8)
    return O, O.Taxonomy(child, parent), len(child)


def _universe(n, gap_bits=24, seed=SEED):
    j = np.arange(n, dtype=U64)
    gaps = U64(1) + (splitmix64(U64(seed) ^ j) & U64((1 << gap_bits) - 1))
    return np.cumsum(gaps, dtype=U64)


def _member(n, f, p, seed):
    h = splitmix64(U64(seed + 1000 * (f + 1)) ^ np.arange(n, dtype=U64))
    return (h >> U64(11)).astype(np.float64) / float(1 << 53) < p


def _taxids(codes, salt):
    T = _oracle()[2]
    return (U64(1) + splitmix64(U64(SEED + 2 + salt) ^ codes) % U64(T)).astype(U32)


def _expand(files, taxs):
    """the oracle's view of a stream with ONE taxid: every record carries it"""
    if taxs is None:
        return None
    return [np.full(len(f), t, U32) if isinstance(t, int) else t for f, t in zip(files, taxs)]


@functools.lru_cache(None)
def _sets():
    """two sorted sets over one universe: a quarter only in A, a quarter only in B, half in both.  30 000 codes each: the
    union (40 000), the intersection (20 000) and the difference (10 000) all span more than one tile of 9728"""
    U = _universe(40_000, 22)
    m = splitmix64(U64(SEED + 1) ^ np.arange(len(U), dtype=U64)) & U64(3)
    return U[(m == 0) | (m >= 2)], U[(m == 1) | (m >= 2)]


def _dup(x):
    """every seventh code twice, every 21st three times"""
    return np.sort(np.concatenate([x, x[::7], x[::21]]))


@functools.lru_cache(None)
def _files(n_univ, nfiles, p, seed=7):
    U = _universe(n_univ)
    files = [U[_member(len(U), f, p, seed)] for f in range(nfiles)]
    return tuple(f for f in files if len(f))


@functools.lru_cache(None)
def _many_short(nfiles=200, per=3000, p=0.02):
    """the smallest shape the single-pass merge is tested with (test_gpu_srmerge.py)"""
    return _files(int(per / p), nfiles, p)


@functools.lru_cache(None)
def _chain(nfiles=6):
    """files that keep a common core (a third of the universe) so that inter / common of all of them is not empty"""
    U = _universe(6_000, 20)
    core = _member(len(U), 0, 0.3, 77)
    return tuple(U[core | _member(len(U), f + 1, 0.6, 78)] for f in range(nfiles))


@functools.lru_cache(None)
def _counted(nfiles=300):
    """test_gpu_srmerge.py::test_common_below_the_number_of_files_counts_inside_the_tiles"""
    U = _universe(20000)
    core = U[::7]
    files = []
    for f in range(nfiles):
        x = U[_member(len(U), f, 0.3, 11)]
        if f % 3:
            x = np.union1d(x, core)
        files.append(x)
    return tuple(files)


@functools.lru_cache(None)
def _big_merge():
    """2^20 records in 12 streams: at fan-in 8 the top level has two children and runs through the 2-way tile kernel"""
    rng = np.random.default_rng(41)
    return tuple(np.sort(rng.integers(0, 1 << 22, 87_000 + 977 * i).astype(U64)) for i in range(12))


def _tax_form(files, form):
    """None, one taxid per record, one per file, or the two mixed"""
    if form == "plain":
        return None
    T = _oracle()[2]
    per_file = [1 + (i * 7919 + 5) % T for i in range(len(files))]
    per_rec = [_taxids(f + U64(i), i) for i, f in enumerate(files)]
    if form == "rec":
        return per_rec
    if form == "file":
        return per_file
    return [per_file[i] if i % 3 else per_rec[i] for i in range(len(files))]


@functools.lru_cache(None)
def _reads():
    """30 000 bases in ragged records (short, empty, long; degenerate bases).  The last third repeats an earlier stretch, so that
    the distinct, the repeated (-d) and the singleton (-u) windows of ukm_count each fill more than one tile of the scan"""
    rng = np.random.default_rng(66)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 30_000)].copy()
    seq[1000:1040] = ord("N")
    seq[20_000:29_900] = seq[1_500:11_400]
    off = np.array([0, 10, 10, 5000, 5020, 12_000, 29_990, 30_000], dtype=U64)
    return seq, off


def _nwin(off, k):
    return int(np.maximum(np.diff(off.astype(np.int64)) - (k - 1), 0).sum())


@functools.lru_cache(None)
def _records():
    """14 000 unsorted records over 3000 distinct 31-mers, a taxid each"""
    rng = np.random.default_rng(14)
    base = splitmix64(np.arange(3000, dtype=U64) + U64(9 << 32)) >> U64(2)
    keys = base[rng.integers(0, len(base), 14_000)]
    tx = (U64(1) + splitmix64(np.arange(len(keys), dtype=U64) ^ U64(SEED)) % U64(64)).astype(U32)
    return base, keys, tx


# ---- the case table -----------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, data, call, expect, bound, dtypes, opts=None, route=None, tile=None, exact=False, verify=None):
        self.name, self._data, self._call, self._expect, self._bound = name, data, call, expect, bound
        self.dtypes, self.opts, self.route, self.tile, self.exact, self.verify = dtypes, opts or {}, route, tile, exact, verify

    @functools.lru_cache(None)
    def data(self):
        return self._data()

    @functools.lru_cache(None)
    def expected(self):
        """the oracle's output arrays, one per output array of the call; computed once per case, never per capacity"""
        O, tax, T = _oracle()
        e = self._expect(O, tax, *self.data())
        e = list(e) if isinstance(e, (tuple, list)) else [e]
        return [np.ascontiguousarray(a, dtype=dt) for a, dt in zip(e, self.dtypes)]

    @property
    def bound(self):
        return int(self._bound(*self.data()))

    def call(self, ctx, L, outs, data=None):
        """data: the case's inputs held elsewhere (test_gpu_alignment.py: device views of them), in the order of data()"""
        return self._call(ctx, L, outs, *(self.data() if data is None else data))


CASES = {}


def _add(name, **kw):
    assert name not in CASES, name
    CASES[name] = Case(name, **kw)


def _kt(tax):
    return [U64, U32] if tax else [U64]


def _o2(outs):
    """(out, out_taxids) keyword arguments of the binding"""
    return dict(out=outs[0], out_taxids=outs[1] if len(outs) > 1 else None)


# ukm_setop2 / ukm_setop2_ft
def _setop2(op, form, flags=0, dup="", opts=None, suffix=""):
    opname = ("union", "inter", "diff")[op]

    def data():
        A, B = _sets()
        A = _dup(A) if "a" in dup else A
        B = _dup(B) if "b" in dup else B
        ra = _taxids(A ^ np.arange(len(A), dtype=U64), 1)     # (the copies of a duplicated code carry different taxids)
        rb = _taxids(B ^ np.arange(len(B), dtype=U64), 2)
        ta, tb = {"plain": (None, None), "rec": (ra, rb), "fta": (17, rb), "ftb": (ra, 4242), "ftab": (17, 4242)}[form]
        return A, B, ta, tb

    def expect(O, tax, A, B, ta, tb):
        tl = None if form == "plain" else _expand([A, B], [ta, tb])
        if op == OP_UNION:
            return O.union([A, B], tl, tax)
        if op == OP_INTER:
            return O.inter([A, B], tl, tax, mix_taxid=bool(flags & F_MIX_TAXID))
        return O.diff([A, B], tl, tax, compare_taxid=bool(flags & F_CMP_TAXID))

    def call(ctx, L, outs, A, B, ta, tb):
        return ctx.setop2(op, A, B, ta, tb, flags=flags, **_o2(outs))

    tile = TILE_SETOP_RANK if dup else (TILE_SETOP if form in ("plain", "ftab") else TILE_SETOP_TAX)
    _add("setop2-%s-%s%s%s" % (opname, form, "-dup" + dup if dup else "", suffix), data=data, call=call, expect=expect,
         bound=lambda A, B, ta, tb: len(A) + len(B) if op == OP_UNION else len(A), dtypes=_kt(form != "plain"), opts=opts, tile=tile)


for _op in (OP_UNION, OP_INTER, OP_DIFF):
    _setop2(_op, "plain")
    for _src in (0, 1, 2):
        for _defer in (0, 1):       # (each combination has its own guarded taxid stores)
            _setop2(_op, "rec", opts={"setop_src": _src, "setop_defer": _defer}, suffix="-src%d-defer%d" % (_src, _defer))
    for _form in ("fta", "ftb", "ftab"):
        _setop2(_op, _form)
    for _d in ("a", "b", "ab"):     # (the fold-then-merge path of union, the rank path, the collapse path of diff)
        _setop2(_op, "plain", dup=_d)
    _setop2(_op, "rec", dup="ab")
_setop2(OP_INTER, "rec", flags=F_MIX_TAXID, suffix="-mix")
_setop2(OP_DIFF, "rec", flags=F_CMP_TAXID, suffix="-cmp")
_setop2(OP_DIFF, "rec", flags=F_CMP_TAXID, dup="ab", suffix="-cmp")


# ukm_unique
def _unique(mode, with_tax):
    def data():
        # 30 000 codes once, 30 000 twice, 10 000 three times: the distinct, the repeated and the singleton codes each fill
        # more than three tiles of 8192
        code = splitmix64(np.arange(70_000, dtype=U64) + U64(5 << 32)) >> U64(2)
        keys = np.sort(np.concatenate([code, code[30_000:], code[60_000:]]))
        n = len(keys)
        return keys, (_taxids(np.arange(n, dtype=U64), 3) if with_tax else None)

    tile = TILE_UNIQ_TAX if with_tax else TILE_UNIQ
    _add("unique-mode%d-%s" % (mode, "tax" if with_tax else "plain"), data=data,
         call=lambda ctx, L, outs, keys, tx: ctx.unique(keys, tx, mode=mode, **_o2(outs)),
         expect=lambda O, tax, keys, tx: O.unique(keys, tx, mode=mode, tax=tax),
         bound=lambda keys, tx: 2 * len(keys) if mode == REPEATED_CHUNK else len(keys), dtypes=_kt(with_tax),
         tile=tile // 2 if mode == REPEATED_CHUNK else tile, exact=mode == PLAIN)


for _mode in (PLAIN, UNIQUE, REPEATED, REPEATED_CHUNK, SINGLETON):
    _unique(_mode, False)
    _unique(_mode, True)


# windows: ukm_encode_kmers / ukm_nthash / ukm_minimizer / ukm_count
def _window_route(want):
    """the kernel that wrote the windows (stat "window_route"); a strip kernel reads the bases four bytes at a time: on a base
    array that does not start on a 4-byte boundary (tests/test_gpu_alignment.py) it is not launched and window_kernel answers"""
    def verify(ctx, data):
        bases = data[0]
        aligned = not hasattr(bases, "data_ptr") or bases.data_ptr() % 4 == 0   # (a host array is copied to an aligned one)
        assert ctx.stat("window_route") == (want if aligned else 1)
    return verify


def _windows():
    K = 31
    bound = lambda seq, off: _nwin(off, K)
    for strip in (0, 1):
        _add("encode-strip%d" % strip, data=_reads, call=lambda ctx, L, outs, seq, off: ctx.encode_kmers(seq, off, K, out=outs[0]),
             expect=lambda O, tax, seq, off: O.count_windows(seq, off, K), bound=bound, dtypes=[U64], opts={"win_strip": strip}, exact=True,
             verify=_window_route(1 + strip))
        _add("nthash-strip%d" % strip, data=_reads, call=lambda ctx, L, outs, seq, off: ctx.nthash(seq, off, K, out=outs[0]),
             expect=lambda O, tax, seq, off: O.count_windows(seq, off, K, hashed=True), bound=bound, dtypes=[U64], opts={"win_strip": strip},
             exact=True, verify=_window_route(1 + strip))
        # the Scaled filter keeps a quarter of the windows: the general kernel, once on its own and once behind a strip launch
        # that gave up (7000 candidates in a tile, the list holds 1024; tests/test_gpu_window_limits.py has the strip kernel's
        # own results): window_kernel answers both
        _add("nthash-scaled-strip%d" % strip, data=_reads,
             call=lambda ctx, L, outs, seq, off: ctx.nthash(seq, off, K, max_hash=ctx.max_hash(4), out=outs[0]),
             expect=lambda O, tax, seq, off: O.count_windows(seq, off, K, hashed=True, max_hash=O.max_hash(4)), bound=bound, dtypes=[U64],
             opts={"nthash_strip": strip}, tile=TILE_WIN, verify=_window_route(1))

    def minimizers(O, tax, seq, off, with_pos, k=23, w=5):
        hs, ps = [], []
        for r in range(len(off) - 1):
            rec = seq[int(off[r]):int(off[r + 1])]
            try:
                h, p = O.minimizer(rec, k, w)
            except ValueError:     # ErrShortSeq: the record is skipped
                continue
            hs.append(h)
            ps.append(p)
        return (np.concatenate(hs), np.concatenate(ps)) if with_pos else np.concatenate(hs)

    _add("minimizer", data=_reads, call=lambda ctx, L, outs, seq, off: ctx.minimizer(seq, off, 23, 5, out=outs[0]),
         expect=lambda O, tax, seq, off: minimizers(O, tax, seq, off, False), bound=lambda seq, off: _nwin(off, 23), dtypes=[U64], tile=TILE_WIN)
    _add("minimizer-pos", data=_reads, call=lambda ctx, L, outs, seq, off: ctx.minimizer(seq, off, 23, 5, out=outs[0], out_pos=outs[1]),
         expect=lambda O, tax, seq, off: minimizers(O, tax, seq, off, True), bound=lambda seq, off: _nwin(off, 23), dtypes=[U64, U64],
         tile=TILE_WIN)
    for mode in (UNIQUE, REPEATED, SINGLETON):
        _add("count-mode%d" % mode, data=_reads, call=lambda ctx, L, outs, seq, off, mode=mode: ctx.count(seq, off, K, mode=mode, out=outs[0]),
             expect=lambda O, tax, seq, off, mode=mode: O.unique(O.sort_u64(O.count_windows(seq, off, K)), mode=mode), bound=bound,
             dtypes=[U64], tile=TILE_UNIQ)


_windows()


# selection and mapping
def _grep_route(want):
    def verify(ctx, data):
        assert ctx.stat("grep_route") == want
    return verify


def _selection():
    def by_codes(O, tax, base, keys, tx):
        m = np.isin(keys, base[:1500])
        return keys[m], tx[m]

    for route, opts in ((1, {"grep_lds": 1}), (2, {"grep_lds": 0})):
        _add("grep-route%d" % route, data=_records, call=lambda ctx, L, outs, base, keys, tx: ctx.grep(keys, queries=base[:1500], taxids=tx, **_o2(outs)),
             expect=by_codes, bound=lambda base, keys, tx: len(keys), dtypes=[U64, U32], opts=opts, tile=TILE_SELECT, verify=_grep_route(route))
    qt = np.arange(1, 33, dtype=U32)

    def by_taxids(O, tax, base, keys, tx):
        m = np.isin(tx, qt)
        return keys[m], tx[m]

    _add("grep-route3", data=_records, call=lambda ctx, L, outs, base, keys, tx: ctx.grep(keys, query_taxids=qt, taxids=tx, **_o2(outs)),
         expect=by_taxids, bound=lambda base, keys, tx: len(keys), dtypes=[U64, U32], tile=TILE_SELECT, verify=_grep_route(3))

    def filtered(O, tax, base, keys, tx):
        from test_gpu_select import model_filter   # filterCode's loops as they are (filter.go:181-221)
        hit = model_filter(keys, 31)
        return keys[~hit], tx[~hit]

    _add("filter", data=_records, call=lambda ctx, L, outs, base, keys, tx: ctx.filter(keys, 31, taxids=tx, **_o2(outs)), expect=filtered,
         bound=lambda base, keys, tx: len(keys), dtypes=[U64, U32], tile=TILE_SELECT)
    _add("sample", data=_records, call=lambda ctx, L, outs, base, keys, tx: ctx.sample(keys, start=3, window=2, taxids=tx, **_o2(outs)),
         expect=lambda O, tax, base, keys, tx: (keys[2::2], tx[2::2]), bound=lambda base, keys, tx: len(keys), dtypes=[U64, U32], tile=TILE_SELECT)

    @functools.lru_cache(None)
    def genome():
        from test_gpu_map import windows   # the windows per record from the oracle's iterator
        O = _oracle()[0]
        k = 23
        rng = np.random.default_rng(5)
        recs = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy() for n in (3000, k - 1, 1500, 700)]
        piece = recs[0][10:10 + 3 * k].copy()      # a piece of record 0 again in record 0 and in the later records
        recs[0][200:200 + len(piece)] = piece
        recs[2][50:50 + len(piece)] = piece
        recs[3][50:50 + len(piece)] = piece
        bases = np.concatenate(recs)
        off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(U64)
        wins = windows(O, bases, off, k)
        allw = np.array([c for w in wins if w is not None for c in w], dtype=U64)
        rng = np.random.default_rng(k)
        q = np.concatenate([allw[rng.integers(0, len(allw), 300)], rng.integers(0, 1 << 62, 50, dtype=U64) | U64(1 << 46)])
        rng.shuffle(q)
        codes = np.unique(allw[rng.random(len(allw)) < 0.7])
        return bases, off, k, wins, q, codes

    def located(O, tax, bases, off, k, wins, q, codes):
        from test_gpu_map import model_locate
        rows = model_locate(wins, q.tolist())
        return [np.array([r[i] for r in rows]) for i in range(3)]

    def mapped(O, tax, bases, off, k, wins, q, codes):
        from test_gpu_map import model_map
        rows = model_map(wins, list(range(len(off) - 1)), codes.tolist(), k, True, k)
        return [np.array([r[i] for r in rows]) for i in range(3)]

    for srt in (0, 1):
        _add("locate-sorted%d" % srt, data=genome, call=lambda ctx, L, outs, bases, off, k, wins, q, codes: ctx.locate(bases, off, k, q, outs=outs),
             expect=located, bound=lambda bases, off, k, *_: _nwin(off, k), dtypes=[U64, U32, U64], opts={"map_sorted": srt})
        _add("map-sorted%d" % srt, data=genome,
             call=lambda ctx, L, outs, bases, off, k, wins, q, codes: ctx.map(bases, off, None, k, codes, allow_multi=True, min_len=k, outs=outs),
             expect=mapped, bound=lambda bases, off, k, *_: _nwin(off, k), dtypes=[U32, U64, U64], opts={"map_sorted": srt})


_selection()


# n-way entry points.  data() of all of them: (files, taxids list or None, the oracle's expanded taxids)
def _streams(shape, form, edit=None):
    def data():
        files = list(shape())
        taxs = _tax_form(files, form)
        if edit is not None:
            files, taxs = edit(files, taxs)
        return files, taxs, _expand(files, taxs)
    return data


def _total(files, taxs, ex):
    return sum(len(f) for f in files)


def _first(files, taxs, ex):
    return len(files[0])


def _reverse_second(files, taxs):
    """one unsorted stream: the union normalises it and tries again"""
    files[1] = files[1][::-1].copy()
    if taxs is not None and not isinstance(taxs[1], int):
        taxs[1] = taxs[1][::-1].copy()
    return files, taxs


def _stable(files, ex):
    cat = np.concatenate(files)
    o = np.argsort(cat, kind="stable")
    return (cat[o], np.concatenate(ex)[o]) if ex is not None else cat[o]


def _nway():
    three = lambda: _files(4000, 3, 0.5)
    five = lambda: _files(8000, 5, 0.5)
    thirty = lambda: _files(3000, 30, 0.5, 77)
    union_shapes = [
        ("tree", three, {}, ROUTE_TREE, None), ("kway", five, {"kway": 1, "srmerge": 0, "punion": 0}, ROUTE_KWAY, None),
        ("srmerge", _many_short, {"srmerge": 1}, ROUTE_SRMERGE, None), ("punion", thirty, {"punion": 1}, ROUTE_PUNION, None),
        ("unsorted", three, {}, ROUTE_TREE, _reverse_second),
        ("two", lambda: _files(4000, 2, 0.5), {}, ROUTE_NONE, None), ("one", lambda: _files(4000, 1, 0.5), {}, ROUTE_NONE, None),
    ]
    for name, shape, opts, route, edit in union_shapes:
        for form in ("plain", "rec", "file", "mixed"):
            if name == "one" and form == "mixed":
                continue
            # (files with one taxid each beside files with one per record: the probe union may leave them to the merges, so
            #  the case neither names nor asserts a route: whichever answers keeps the contract)
            loose = name == "punion" and form == "mixed"
            pinned = None if loose else route
            _add("union-%s-%s" % ("thirty-files" if loose else name, form), data=_streams(shape, form, edit), call=lambda ctx, L, outs, files, taxs, ex: ctx.union(files, taxs, **_o2(outs)),
                 expect=lambda O, tax, files, taxs, ex: O.union(files, ex, tax), bound=_total, dtypes=_kt(form != "plain"), opts=opts, route=pinned,
                 exact=name == "one")

    def merge(name, shape, form, mode, final, opts, route):
        def expect(O, tax, files, taxs, ex):
            if mode == PLAIN:
                return _stable(files, ex)
            return O.merge_k(files, ex, mode=mode, final_round=final, tax=tax)
        _add("merge-%s-%s" % (name, form), data=_streams(shape, form),
             call=lambda ctx, L, outs, files, taxs, ex: ctx.merge_k(files, taxs, mode=mode, final_round=final, **_o2(outs)), expect=expect,
             bound=lambda files, taxs, ex: 2 * _total(files, taxs, ex), dtypes=_kt(form != "plain"), opts=opts, route=route)

    for form in ("plain", "rec"):
        merge("plain", three, form, PLAIN, True, {}, None)    # (cap >= total: straight into the caller's buffer; below: workspace, then the scan)
        merge("unique", three, form, UNIQUE, True, {}, None)
        merge("repeated", three, form, REPEATED, True, {}, None)
        merge("chunk", three, form, REPEATED, False, {}, None)
        merge("place", lambda: _files(3000, 40, 0.7), form, PLAIN, True, {"place": 1, "punion": 1}, ROUTE_PLACE)
        merge("srmerge", _many_short, form, PLAIN, True, {"srmerge": 1}, ROUTE_SRMERGE)
        merge("kway", five, form, PLAIN, True, {"kway": 1, "srmerge": 0, "place": 0}, ROUTE_KWAY)
        merge("pcommon", lambda: _files(3000, 30, 0.8, 79), form, REPEATED, True, {"punion": 1}, ROUTE_PCOMMON)

    def same_ct():
        files = list(three())
        taxs = [77] * len(files)      # (the chunk files of `sort -m` over a `count -t` file: the plain merge and a fill)
        return files, taxs, _expand(files, taxs)
    _add("merge-same-file-taxid", data=same_ct, call=lambda ctx, L, outs, files, taxs, ex: ctx.merge_k(files, taxs, mode=PLAIN, **_o2(outs)),
         expect=lambda O, tax, files, taxs, ex: _stable(files, ex), bound=lambda files, taxs, ex: 2 * _total(files, taxs, ex), dtypes=[U64, U32])
    merge("2e20", _big_merge, "rec", PLAIN, True, {}, ROUTE_KWAY)

    # inter / diff over six streams: the probe fold, the range fold, the chained fold, the synchronous fold
    def dup_first(files, taxs):
        n = len(files[0])
        files[0] = _dup(files[0])
        if taxs is not None:
            taxs[0] = _taxids(files[0] ^ np.arange(len(files[0]), dtype=U64), 50)
        assert len(files[0]) > n
        return files, taxs

    def unsorted_later(files, taxs):
        rng = np.random.default_rng(8)
        for i in (2, 4):
            perm = rng.permutation(len(files[i]))
            files[i] = files[i][perm]
            if taxs is not None and not isinstance(taxs[i], int):
                taxs[i] = taxs[i][perm]
        return files, taxs

    thinned = lambda: _chain()[:1] + tuple(f[::6] for f in _chain()[1:])    # (later files that leave some of the first)
    folds = [("pfold", {}, None), ("rfold", {"no_pfold": 1}, None), ("chain", {"no_pfold": 1, "no_fold": 1}, None), ("sync", {}, dup_first)]
    for name, opts, edit in folds:
        for form in ("plain", "rec"):
            _add("inter-%s-%s" % (name, form), data=_streams(_chain, form, edit), call=lambda ctx, L, outs, files, taxs, ex: ctx.inter(files, taxs, **_o2(outs)),
                 expect=lambda O, tax, files, taxs, ex: O.inter(files, ex, tax), bound=_first, dtypes=_kt(form != "plain"), opts=opts)
            _add("diff-%s-%s" % (name, form), data=_streams(thinned, form, edit),
                 call=lambda ctx, L, outs, files, taxs, ex: ctx.diff(files, taxs, **_o2(outs)),
                 expect=lambda O, tax, files, taxs, ex: O.diff(files, ex, tax), bound=_first, dtypes=_kt(form != "plain"), opts=opts)
    _add("inter-mix-taxid", data=_streams(_chain, "rec"), call=lambda ctx, L, outs, files, taxs, ex: ctx.inter(files, taxs, mix_taxid=True, **_o2(outs)),
         expect=lambda O, tax, files, taxs, ex: O.inter(files, ex, tax, mix_taxid=True), bound=_first, dtypes=[U64, U32])
    sf = [1, 1, 0, 1, 0, 1]
    _add("diff-t-unsorted-later", data=_streams(thinned, "rec", unsorted_later),
         call=lambda ctx, L, outs, files, taxs, ex: ctx.diff(files, taxs, compare_taxid=True, sorted_flags=sf, **_o2(outs)),
         expect=lambda O, tax, files, taxs, ex: O.diff(files, ex, tax, compare_taxid=True, sorted_flags=sf), bound=_first, dtypes=[U64, U32])
    for name, ishape, dshape, form in (("file-taxids", _chain, thinned, "file"), ("two", lambda: _chain()[:2], lambda: thinned()[:2], "rec")):
        _add("inter-%s" % name, data=_streams(ishape, form), call=lambda ctx, L, outs, files, taxs, ex: ctx.inter(files, taxs, **_o2(outs)),
             expect=lambda O, tax, files, taxs, ex: O.inter(files, ex, tax), bound=_first, dtypes=[U64, U32])
        _add("diff-%s" % name, data=_streams(dshape, form), call=lambda ctx, L, outs, files, taxs, ex: ctx.diff(files, taxs, **_o2(outs)),
             expect=lambda O, tax, files, taxs, ex: O.diff(files, ex, tax), bound=_first, dtypes=[U64, U32])
    for which in ("inter", "diff"):
        _add("%s-one" % which, data=_streams(lambda: _chain()[:1], "rec"),
             call=lambda ctx, L, outs, files, taxs, ex, which=which: getattr(ctx, which)(files, taxs, **_o2(outs)),
             expect=lambda O, tax, files, taxs, ex, which=which: getattr(O, which)(files, ex, tax), bound=_first, dtypes=[U64, U32], exact=True)

    # common: the threshold equal to the number of files (probe fold), and below it three ways
    def common(name, shape, thr, form, opts, route):
        _add("common-%s-%s" % (name, form), data=_streams(shape, form),
             call=lambda ctx, L, outs, files, taxs, ex: ctx.common(files, thr(files), taxs, **_o2(outs)),
             expect=lambda O, tax, files, taxs, ex: O.common(files, thr(files), ex, tax), bound=_total, dtypes=_kt(form != "plain"), opts=opts, route=route)

    for form in ("plain", "rec"):
        common("all", _chain, len, form, {}, None)
        common("pcommon", lambda: _files(3000, 30, 0.8, 79), lambda f: len(f) // 2, form, {"punion": 1, "common_probe": 0}, ROUTE_PCOMMON)
        common("srcommon", _counted, lambda f: 120, form, {"srmerge": 1, "common_probe": 0, "punion": 0}, ROUTE_SRCOMMON)
        common("scan", _chain, lambda f: 3, form, {"punion": 0, "srmerge": 0}, None)


_nway()

NAMES = sorted(CASES)
TILED = [n for n in NAMES if CASES[n].tile]


def capacities(need, bound, tile):
    """0, 1, need - 1, need, bound; for the tiled kernels also one value inside the first tile, tile - 1, tile, tile + 1 and one
    value inside the last tile.  Ascending, the NULL-pointer size query (0) last: a kernel that ignored out_cap is caught by
    the guards of the smaller capacities before it is handed a NULL pointer."""
    caps = {0, 1, need - 1, need, bound}
    if tile:
        caps |= {tile // 2, tile - 1, tile, tile + 1, max(need - tile // 3, 0)}
    caps = sorted(c for c in caps if 0 <= c <= bound)
    return caps[1:] + caps[:1]


def test_case_table_oracle_only():
    """no GPU: every case's expected output from the oracle alone; 2 <= need < bound (need == bound where the documented
    bound is the size itself), all output arrays of a case equally long"""
    for name in NAMES:
        c = CASES[name]
        exp = c.expected()
        need = len(exp[0])
        assert len(exp) == len(c.dtypes) and all(len(e) == need for e in exp), name
        assert need >= 2, (name, need)
        if c.exact:
            assert need == c.bound, (name, need, c.bound)
        else:
            assert need < c.bound, (name, need, c.bound)
        caps = capacities(need, c.bound, c.tile)
        if c.tile:     # (the brackets round one tile are failing capacities: a full tile, a guarded one and one behind out_cap)
            assert need > c.tile + 1, (name, need, c.tile)
        assert {0, 1, need - 1, need, c.bound} <= set(caps) and caps[-1] == 0, name


# ---- the helper every GPU case goes through ---------------------------------------------------------------------------------
class Guarded:
    """one output array: [front guard | cap | back guard], all sentinel; the call gets the middle.  shift: the front guard
    is FRONT + shift elements, so the middle starts `shift` elements behind a 16-byte boundary"""

    def __init__(self, dtype, cap, bound, place, shift=0):
        self.dt, self.cap, self.front = np.dtype(dtype), cap, FRONT + shift
        back = max(bound - cap, 0) + 64
        host = np.full(self.front + cap + back, SENT[self.dt], dtype=self.dt)
        if place == "device":
            import torch
            self.buf = torch.from_numpy(host.view(SIGNED[self.dt])).cuda()
            ptr = self.buf.data_ptr()
        else:
            self.buf = host
            ptr = host.ctypes.data
        assert ptr % 16 == 0
        self.mid = self.buf[self.front:self.front + cap]

    def host(self):
        return self.buf.cpu().numpy().view(self.dt) if hasattr(self.buf, "cpu") else self.buf

    def check(self, what):
        h = self.host()
        bad = np.flatnonzero(h != self.dt.type(SENT[self.dt]))
        bad = bad[(bad < self.front) | (bad >= self.front + self.cap)] - self.front
        assert len(bad) == 0, "%s: %d guard words written, at offsets %s from the start of the buffer of %d" % (what, len(bad), bad[:8].tolist(), self.cap)

    def head(self, n):
        return self.host()[self.front:self.front + n]


def attempt(ctx, L, case, cap, place, shifts=None, data=None):
    """shifts: one Guarded shift per output array; data: see Case.call"""
    exp = case.expected()
    need = len(exp[0])
    what = "%s, out_cap = %d (need %d, bound %d), %s outputs" % (case.name, cap, need, case.bound, place)
    bufs = [Guarded(dt, cap, case.bound, place, shift=s) for dt, s in zip(case.dtypes, shifts or [0] * len(case.dtypes))]
    err = res = None
    try:
        res = case.call(ctx, L, [b.mid for b in bufs], data)
    except L.CapacityError as e:
        err = e
    for i, b in enumerate(bufs):
        b.check("%s, output array %d" % (what, i))
    if cap >= need:
        assert err is None, "%s: %s" % (what, err)
        first = res[0] if isinstance(res, tuple) else res
        assert len(first) == need, "%s: n_out = %d" % (what, len(first))
        for i, (b, e) in enumerate(zip(bufs, exp)):
            assert np.array_equal(b.head(need), e), "%s: output array %d differs from the oracle" % (what, i)
        if case.route is not None:
            assert ctx.last_route() == case.route, "%s: route %d answered, not %d" % (what, ctx.last_route(), case.route)
        if case.verify is not None:
            case.verify(ctx, data if data is not None else case.data())
    else:
        assert err is not None, "%s: the call succeeded" % what
        assert err.needed == need, "%s: UKM_ERR_CAPACITY with n_out = %s" % (what, err.needed)


def exercise(ctx, L, case, place, ticket=False):
    opts = dict(case.opts, force_ticket=1) if ticket else case.opts
    need = len(case.expected()[0])
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        for cap in capacities(need, case.bound, case.tile):
            attempt(ctx, L, case, cap, place)
            if cap < need:
                attempt(ctx, L, case, case.bound, place)     # the same context, straight after the failed call
    finally:
        for k in opts:
            ctx.set_option(k, None)


@pytest.fixture(scope="module")
def env():
    from unikmer_amd import lib as L
    ctx = L.Context(0)
    ctx.taxonomy_load(*synth_tree(5, 8))
    yield ctx, L
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("place", ["host", "device"])
@pytest.mark.parametrize("name", NAMES)
def test_capacity(env, name, place):
    ctx, L = env
    exercise(ctx, L, CASES[name], place)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TILED)
def test_capacity_ticketed(env, name):
    """the ticketed instantiations of the tiled kernels are kernels of their own"""
    ctx, L = env
    exercise(ctx, L, CASES[name], "device", ticket=True)


@pytest.mark.gpu
def test_size_query_of_an_empty_result_and_null_out_taxids(env):
    """include/unikmer_hip.h: a size query (out_cap == 0, NULL outputs) on an empty result with taxids is UKM_OK with
    *n_out == 0; a NULL out_taxids with out_cap > 0 and records that carry taxids stays UKM_ERR_INVALID"""
    ctx, L = env
    A, B = _sets()
    a, b = A[::2], A[1::2]                                     # disjoint: inter is empty; all distinct: -d is empty
    ta, tb = _taxids(a, 1), _taxids(b, 2)
    none64, none32 = np.empty(0, U64), np.empty(0, U32)        # (lib._ptr: NULL)
    empty = [lambda o, t: ctx.setop2(OP_INTER, a, b, ta, tb, out=o, out_taxids=t),
             lambda o, t: ctx.inter([a, b], [ta, tb], out=o, out_taxids=t),
             lambda o, t: ctx.inter([a, b, a, b, a], [ta, tb, ta, tb, ta], out=o, out_taxids=t),
             lambda o, t: ctx.unique(a, ta, mode=REPEATED, out=o, out_taxids=t)]
    for i, call in enumerate(empty):
        gk, gt = call(none64, none32)
        assert len(gk) == 0 and len(gt) == 0, i
    full = [lambda o, t: ctx.setop2(OP_UNION, a, b, ta, tb, out=o, out_taxids=t),
            lambda o, t: ctx.union([a, b, A], [ta, tb, _taxids(A, 3)], out=o, out_taxids=t),
            lambda o, t: ctx.unique(a, ta, mode=UNIQUE, out=o, out_taxids=t),
            lambda o, t: ctx.grep(a, queries=a[:10], taxids=ta, out=o, out_taxids=t)]
    for i, call in enumerate(full):
        with pytest.raises(L.UkmError) as e:
            call(np.empty(2 * len(A), U64), none32)
        assert e.value.code == L.ERR_INVALID, (i, e.value)
    # and the context answers the next call
    gk, gt = ctx.setop2(OP_INTER, a, a, ta, ta)
    assert np.array_equal(gk, a) and np.array_equal(gt, ta)
