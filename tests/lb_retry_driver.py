"""Driver of tests/test_gpu_lb_retry.py: every look-back kernel with a watchdog, run once in THIS process against the
library UKM_LIB_PATH names.  Not collected by pytest; started as `python tests/lb_retry_driver.py OUT.jsonl`.

The seam library (unikmer_amd/build.py: libunikmer_hip_lbtest.so, compiled with UKM_LB_TEST_TIMEOUT) makes every tile >= 1
whose id came from blockIdx give up its look-back at once, so the first launch of each look-back kernel writes every
tile at base 0, raises its watchdog flag, and the host repeats the launch with ticketed tile ids (ukm_lb_launch; the
chained fold falls back to the synchronous one).  Every case runs on a fresh Context -- the switch to tickets is permanent
-- and leaves one JSON line: {"name", "error" (a traceback, or null), "wd" ([lb_watchdogs, ticket_latched] at every mark
of the case), "seconds"}.  Expected values come from the CPU oracle (and, where it has no such operation, from the
numpy / Python models the other test modules use).  A HIP error ends the process at once: nothing more is started.

Tile sizes (records per workgroup), from the sources:
  ukm_setops.hip   (ukm_setop_kernels.h) 512 x 19 = 9728 plain, 512 x 7 = 3584 with per-record taxids (SETOP_VT_TAX), 512 x 12 = 6144 with
                   ranks and for diff without -t; the fused partition and its cache start at 4 * PART_COARSE = 256 tiles
  ukm_scan.hip     unique: 512 x 16 = 8192, 512 x 12 = 6144 with taxids, half of either in the chunk protocol
  ukm_encode.hip   (ukm_win_kernels.h, ukm_win_minimizer.h) window kernel 2048 positions, minimizer 2048 windows, ntHash strip
                   filter 256 lanes x L = 256 positions
  ukm_select.hip, ukm_tsplit.hip, ukm_map.hip   256 x 8 = 2048
Every shape below has at least 3 tiles and a partial last one.
"""
import json
import os
import sys
import time
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

U64, U32, U8 = np.uint64, np.uint32, np.uint8
G64, G32 = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5
GUARD = 64                      # guard words directly behind out_cap records of every output
OP_UNION, OP_INTER, OP_DIFF = 0, 1, 2
SMALL = 16_000                  # |A| = |B|: 32,000 merged records = 3.3 plain tiles, 8.9 taxid tiles, 5.2 rank tiles
FUSED = 1_300_000               # 2.6e6 merged records = 268 plain tiles >= 256
FIRED, QUIET = (1, 1), (0, 0)   # [lb_watchdogs, ticket_latched] behind a call whose first launch timed out / any other call

CASES = []                      # (name, function, the marks expected under the seam library)


def case(name, *marks):
    """marks: what h.mark() must read, in order, under the seam library; under the product library every mark is QUIET"""
    def deco(fn):
        CASES.append((name, fn, [list(m) for m in marks]))
        return fn
    return deco


def expected(name, seam):
    for n, _, marks in CASES:
        if n == name:
            return marks if seam else [list(QUIET)] * len(marks)
    raise KeyError(name)


STANDARD = (QUIET, FIRED, FIRED)      # a fresh context, the call, the same call again
CONTROL = (QUIET, QUIET, QUIET)       # a call without a look-back (or one that starts ticketed)


# ---- the harness ---------------------------------------------------------------------------------------------------------
class H:
    def __init__(self):
        import torch
        from oracle import oracle
        from unikmer_amd import lib
        self.torch, self.L, self.O = torch, lib, oracle
        self.ctx = None
        self.wd = []
        self._in, self._out = [], []

    def begin(self):
        self.ctx = self.L.Context(0)
        self.wd, self._in, self._out = [], [], []
        self.mark()

    def end(self):
        if self.ctx is not None:
            self.ctx.close()
            self.ctx = None

    def mark(self):
        self.wd.append([self.ctx.stat("lb_watchdogs"), self.ctx.stat("ticket_latched")])

    def up(self, x, dtype):
        """a device copy of x; the case ends with check_inputs()"""
        a = np.ascontiguousarray(x, dtype=dtype)
        t = self.torch.from_numpy(a.view({U64: np.int64, U32: np.int32, U8: np.uint8}[dtype]).copy()).cuda()
        self.torch.cuda.synchronize()
        self._in.append((t, a.copy(), dtype))
        return t

    def write(self, dst, x, dtype):
        """new contents in place (the same pointer and size)"""
        a = np.ascontiguousarray(x, dtype=dtype)
        assert len(a) == dst.numel()
        dst.copy_(self.torch.from_numpy(a.view({U64: np.int64, U32: np.int32}[dtype]).copy()).cuda())
        self.torch.cuda.synchronize()
        self._in = [(t, a.copy(), d) if t is dst else (t, h, d) for t, h, d in self._in]

    def out(self, dtype, cap):
        """an output of `cap` records with GUARD guard words directly behind them"""
        tt, g = {U64: (self.torch.int64, G64 - (1 << 64)), U32: (self.torch.int32, G32 - (1 << 32))}[dtype]
        buf = self.torch.full((cap + GUARD,), g, dtype=tt, device="cuda")
        self.torch.cuda.synchronize()
        self._out.append((buf, cap, dtype))
        return buf[:cap]

    def host(self, t, dtype):
        return t.cpu().numpy().view(dtype)

    def check_guards(self):
        for buf, cap, dtype in self._out:
            tail = self.host(buf[cap:], dtype)
            assert (tail == (G64 if dtype == U64 else G32)).all(), "guard words behind out_cap = %d were overwritten" % cap
        self._out = []

    def check_inputs(self):
        for t, a, dtype in self._in:
            assert np.array_equal(self.host(t, dtype), a), "an input was modified"

    def same(self, got, want, what=""):
        got = got if isinstance(got, tuple) else (got,)
        want = want if isinstance(want, tuple) else (want,)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            g = self.host(g, w.dtype.type)
            assert len(g) == len(w), "%s output %d: %d records, the oracle has %d" % (what, i, len(g), len(w))
            assert np.array_equal(g, w), "%s output %d differs from the oracle (first at %d)" % (what, i, int(np.flatnonzero(g != w)[0]))

    def standard(self, call, want):
        """call(caps) -> the outputs, allocated with out() at the capacities it is given (None: exactly the oracle's sizes).
        The call; the same call again on the same context; guards and inputs."""
        for what in ("first call", "repeated call"):
            self.same(call(None), want, what)
            self.mark()
            self.check_guards()
        self.check_inputs()

    def short(self, call, want, need):
        """out_cap one below the result: the capacity error carries the oracle's count, twice; then the call that fits"""
        for what in ("first call", "repeated call"):
            try:
                call(need - 1)
                raise AssertionError("%s: no capacity error" % what)
            except self.L.CapacityError as e:
                assert e.needed == need, "%s: the capacity error says %r, the oracle %d" % (what, e.needed, need)
            self.mark()
            self.check_guards()
        self.same(call(None), want, "fitting call")
        self.check_guards()
        self.check_inputs()


# ---- data ----------------------------------------------------------------------------------------------------------------
def splitmix64(x):
    x = np.asarray(x, dtype=U64)
    with np.errstate(over="ignore"):
        z = x + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


_cache = {}


def memo(fn):
    def g(*a):
        k = (fn.__name__,) + a
        if k not in _cache:
            _cache[k] = fn(*a)
        return _cache[k]
    return g


@memo
def sets(n, seed=0x6C62):
    """two sorted sets of n codes: a third only in A, a third only in B, a third in both, in random order (tiles produce
    different counts for every operation)"""
    nu = int(n * 1.52) + 64
    j = np.arange(nu, dtype=U64)
    U = (U64(1) << U64(32)) + np.cumsum(U64(2) + (splitmix64(U64(seed) ^ j) & U64((1 << 24) - 1)), dtype=U64)
    m = splitmix64(U64(seed + 1) ^ j) % U64(3)
    A, B = U[m != 1][:n], U[m != 0][:n]
    assert len(A) == n and len(B) == n
    return A, B


@memo
def multisets(n):
    """the sets with runs of equal codes inside each file (pairs, and runs of three and four)"""
    A, B = (x.copy() for x in sets(n))
    A[7::7] = A[6::7][:len(A[7::7])]
    i = np.arange(21, n - 2, 21)
    B[i + 2] = B[i + 1] = B[i] = B[i - 1]
    assert np.all(A[1:] >= A[:-1]) and np.all(B[1:] >= B[:-1])
    return A, B


@memo
def spine_forest():
    """A forest whose clade cut follows a 40-level spine (pairs below different clade nodes share many levels), a large bush
    at its end, two more trees and two merged ids: the taxonomy of tests/test_gpu_parity.py's dense-LCA test.  The pool
    mixes relatives inside one clade (root paths: the DEFER tiles' fix list), unrelated pairs, zero and unknown ids."""
    child, parent = [1], [1]
    nxt, spine = 2, 1
    for _ in range(40):
        for _ in range(2):
            root = nxt; nxt += 1
            child.append(root); parent.append(spine)
            for _ in range(3):
                m = nxt; nxt += 1
                child.append(m); parent.append(root)
                for _ in range(3):
                    child.append(nxt); parent.append(m); nxt += 1
        s2 = nxt; nxt += 1
        child.append(s2); parent.append(spine)
        spine = s2
    for k in range(3000):
        child.append(nxt); parent.append(spine if k < 30 else nxt - 30); nxt += 1
    r2 = nxt; nxt += 1
    child.append(r2); parent.append(r2)
    for k in range(200):
        child.append(nxt); parent.append(r2 if k < 5 else nxt - 5); nxt += 1
    r3 = nxt + 10
    child.append(r3); parent.append(r3)
    child, parent = np.array(child, U32), np.array(parent, U32)
    mo, mn = np.array([r3 + 5, r3 + 6], U32), np.array([int(child[777]), 999_999], U32)
    pool = np.concatenate([child, child, child, [0] * 400, [r3 + 5, r3 + 6, r3 + 7, 2 ** 31] * 50]).astype(U32)
    return child, parent, mo, mn, pool


def load_forest(h):
    child, parent, mo, mn, _ = spine_forest()
    h.ctx.taxonomy_load(child, parent, mo, mn)
    if "forest" not in _cache:
        _cache["forest"] = h.O.Taxonomy(child, parent, mo, mn)
    return _cache["forest"]


@memo
def set_taxids(n):
    pool = spine_forest()[4]
    A, B = sets(n)
    ta = pool[(splitmix64(A ^ U64(0x7461)) % U64(len(pool))).astype(np.int64)]
    tb = pool[(splitmix64(B ^ U64(0x7462)) % U64(len(pool))).astype(np.int64)]
    return ta, tb


@memo
def reads(total, nrec, seed):
    """random ACGT records of different lengths, `total` bases in all"""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(100, total - 100), nrec - 1, replace=False))
    off = np.concatenate([[0], cuts, [total]]).astype(U64)
    return np.frombuffer(b"ACGT", dtype=U8)[rng.integers(0, 4, total)].copy(), off


def oracle_fn(O, op):
    return {OP_UNION: O.union, OP_INTER: O.inter, OP_DIFF: O.diff}[op]


# ---- ukm_setop2 ------------------------------------------------------------------------------------------------------------
def setop_call(h, op, dA, dB, bound, ta=None, tb=None, flags=0):
    tax = ta is not None
    def call(cap):
        ck = bound if cap is None else cap
        out = h.out(U64, ck)
        outt = h.out(U32, ck) if tax else None
        return h.ctx.setop2(op, dA, dB, ta, tb, flags=flags, out=out, out_taxids=outt)
    return call


def add_plain(n, tag):
    for op, opname in ((OP_UNION, "union"), (OP_INTER, "inter"), (OP_DIFF, "diff")):
        @case("setop2-%s-%s" % (opname, tag), *STANDARD)
        def _(h, op=op):
            A, B = sets(n)
            want = oracle_fn(h.O, op)([A, B])
            h.standard(setop_call(h, op, h.up(A, U64), h.up(B, U64), len(want)), want)


add_plain(SMALL, "small")
add_plain(FUSED, "fused")


def add_tax(tag, ops, opts, flags=0, okw=None):
    for op, opname in ops:
        @case("setop2-tax-%s-%s" % (tag, opname), *STANDARD)
        def _(h, op=op):
            tax = load_forest(h)
            for k, v in opts.items():
                h.ctx.set_option(k, v)
            A, B = sets(SMALL)
            ta, tb = set_taxids(SMALL)
            wk, wt = oracle_fn(h.O, op)([A, B], [ta, tb], tax, **(okw or {}))
            h.standard(setop_call(h, op, h.up(A, U64), h.up(B, U64), len(wk), h.up(ta, U32), h.up(tb, U32), flags), (wk, wt))


UI = ((OP_UNION, "union"), (OP_INTER, "inter"))
add_tax("defer", UI, {})                                                  # DEFER tiles + setop_taxid_fix_kernel
add_tax("defer0", UI, {"setop_defer": 0})                                 # the LCAs inside the merge step; source words for inter
add_tax("defer0-src0", UI, {"setop_defer": 0, "setop_src": 0})            # ... and the taxid instantiation for both
add_tax("src1", ((OP_INTER, "inter"),), {"setop_src": 1})                 # source words + setop_taxid_gather_kernel
add_tax("src2", ((OP_UNION, "union"),), {"setop_src": 2})
add_tax("carried", ((OP_DIFF, "diff"),), {})                              # diff without -t: taxids carried on the rank-sized tile
add_tax("cmp", ((OP_DIFF, "diff"),), {}, flags=4, okw={"compare_taxid": True})   # UKM_F_CMP_TAXID
add_tax("mix", ((OP_INTER, "inter"),), {}, flags=2, okw={"mix_taxid": True})     # UKM_F_MIX_TAXID


def add_ct(opname, op, fa, fb, flags=0, okw=None):
    @case("setop2_ft-%s-%d-%d%s" % (opname, fa, fb, "-mix" if flags else ""), *STANDARD)
    def _(h):
        tax = load_forest(h)
        A, B = sets(SMALL)
        wk, wt = oracle_fn(h.O, op)([A, B], [np.full(len(A), fa, U32), np.full(len(B), fb, U32)], tax, **(okw or {}))
        dA, dB = h.up(A, U64), h.up(B, U64)
        def call(cap):
            ck = len(wk) if cap is None else cap
            return h.ctx.setop2(op, dA, dB, int(fa), int(fb), flags=flags, out=h.out(U64, ck), out_taxids=h.out(U32, ck))
        h.standard(call, (wk, wt))


for _opname, _op in (("union", OP_UNION), ("inter", OP_INTER), ("diff", OP_DIFF)):
    add_ct(_opname, _op, 700, 3000)                                       # two nodes of the forest: the CT epilogue
add_ct("inter", OP_INTER, 0, 3000, flags=2, okw={"mix_taxid": True})
add_ct("inter", OP_INTER, 700, 3000, flags=2, okw={"mix_taxid": True})


for _opname, _op in (("inter", OP_INTER), ("diff", OP_DIFF)):
    @case("setop2-dup-%s" % _opname, *STANDARD)
    def _(h, op=_op):
        # the retried plain pass finds FLAG_DUP; the re-run on (code, rank) pairs follows, ticketed
        A, B = multisets(SMALL)
        want = oracle_fn(h.O, op)([A, B])
        h.standard(setop_call(h, op, h.up(A, U64), h.up(B, U64), len(want)), want)


@case("setop2-union-small-short", *STANDARD)
def _(h):
    A, B = sets(SMALL)
    want = h.O.union([A, B])
    h.short(setop_call(h, OP_UNION, h.up(A, U64), h.up(B, U64), len(want)), want, len(want))


@case("setop2-tax-defer-union-short", *STANDARD)
def _(h):
    tax = load_forest(h)
    A, B = sets(SMALL)
    ta, tb = set_taxids(SMALL)
    wk, wt = h.O.union([A, B], [ta, tb], tax)
    h.short(setop_call(h, OP_UNION, h.up(A, U64), h.up(B, U64), len(wk), h.up(ta, U32), h.up(tb, U32)), (wk, wt), len(wk))


# ---- the set-op caches x timeout, fused shape ------------------------------------------------------------------------------
def cache_stats(h):
    return tuple(h.ctx.stat(k) for k in ("setop_part_hits", "setop_part_stale", "setop_offs_hits", "setop_offs_stale"))


def cache_case(h, rewrite):
    A, B = sets(FUSED)
    dA, dB = h.up(A, U64), h.up(B, U64)
    run = lambda op, a: h.same(setop_call(h, op, dA, dB, len(a) + len(B) if op == OP_UNION else len(a))(None), oracle_fn(h.O, op)([a, B]), "op %d" % op)
    # warm the partition cache with ticketed tiles, recording no match counts
    h.ctx.set_option("force_ticket", 1)
    h.ctx.set_option("setop_offs_reuse", 0)
    run(OP_INTER, A)
    h.mark()
    assert cache_stats(h) == (0, 0, 0, 0)
    h.ctx.set_option("force_ticket", None)
    h.ctx.set_option("setop_offs_reuse", None)
    if rewrite:
        # the buffers rewritten in place under the key: FLAG_STALE -> SEARCH -> timeout -> retry
        A = sets(FUSED, 0x7777)[0]
        h.write(dA, A, U64)
    # the union keeps the look-back on a cached table (SETOP_OFFS_OPS = inter and diff): VERIFY_LOOKBACK, timeout, retry
    run(OP_UNION, A)
    h.mark()
    assert cache_stats(h) == ((0, 1, 0, 0) if rewrite else (1, 0, 0, 0)), cache_stats(h)
    # A third call hits the cache and takes its offsets from the match counts recorded behind the RETRIED pass: counts
    # committed from the damaged first pass would show as "setop_offs_stale" (or as a wrong result)
    run(OP_INTER, A)
    h.mark()
    assert cache_stats(h) == ((1, 1, 1, 0) if rewrite else (2, 0, 1, 0)), cache_stats(h)
    run(OP_DIFF, A)
    assert cache_stats(h) == ((2, 1, 2, 0) if rewrite else (3, 0, 2, 0)), cache_stats(h)
    h.check_guards()
    h.check_inputs()


@case("setop2-cache-hit-then-timeout", QUIET, QUIET, FIRED, FIRED)
def _(h):
    cache_case(h, False)


@case("setop2-cache-stale-then-timeout", QUIET, QUIET, FIRED, FIRED)
def _(h):
    cache_case(h, True)


# ---- ukm_unique ------------------------------------------------------------------------------------------------------------
@memo
def sorted_with_repeats(n):
    """n sorted codes: singletons, pairs and longer runs, a different mix in every tile"""
    j = np.arange(n, dtype=U64)
    step = (splitmix64(j ^ U64(0x756E)) % U64(4) > (j // U64(3000)) % U64(3)).astype(U64)
    k = U64(1000) + np.cumsum(step, dtype=U64) * U64(7)
    t = spine_forest()[4][(splitmix64(j ^ U64(0x756F)) % U64(len(spine_forest()[4]))).astype(np.int64)]
    return k, t


UNIQ_N = 3 * 8192 + 77
for _mode, _mname in ((1, "unique"), (2, "repeated"), (3, "repeated_chunk"), (4, "singleton")):
    for _tax in (False, True):
        @case("unique-%s%s" % (_mname, "-tax" if _tax else ""), *STANDARD)
        def _(h, mode=_mode, with_tax=_tax):
            k, t = sorted_with_repeats(UNIQ_N)
            tax = load_forest(h) if with_tax else None
            want = h.O.unique(k, t if with_tax else None, mode, tax)
            n = len(want[0]) if with_tax else len(want)
            assert 0 < n < len(k)
            dk, dt = h.up(k, U64), (h.up(t, U32) if with_tax else None)
            def call(cap):
                c = n if cap is None else cap
                return h.ctx.unique(dk, dt, mode, out=h.out(U64, c), out_taxids=h.out(U32, c) if with_tax else None)
            h.standard(call, want)


@case("unique-in-place", *CONTROL)
def _(h):
    # output = input: a damaged first pass would be read by the retry, so the call starts ticketed (no watchdog at all)
    k, _ = sorted_with_repeats(UNIQ_N)
    want = h.O.unique(k, None, 1, None)
    for _ in range(2):
        buf = h.out(U64, len(k))
        buf.copy_(h.torch.from_numpy(k.view(np.int64).copy()).cuda())
        h.torch.cuda.synchronize()
        h.same(h.ctx.unique(buf, None, 1, out=buf), want, "in place")
        h.mark()
        h.check_guards()


# ---- ukm_nthash, ukm_encode_kmers, ukm_minimizer, ukm_count -------------------------------------------------------------------
READS = (250_000, 40, 5)        # 250,000 bases: 4 strip tiles of 65,536 positions, 123 window tiles of 2048


def windows_case(name, marks, opts, fn):
    @case(name, *marks)
    def _(h):
        for k, v in opts.items():
            h.ctx.set_option(k, v)
        seq, off = reads(*READS)
        want, call = fn(h, seq, off, h.up(seq, U8), h.up(off, U64))
        assert len(want[0] if isinstance(want, tuple) else want) > 100
        h.standard(call, want)


def nthash_fn(scale, circular=False):
    def fn(h, seq, off, dseq, doff):
        mh = h.O.max_hash(scale) if scale else 0
        want = h.O.count_windows(seq, off, 51, hashed=True, circular=circular, max_hash=mh)
        return want, lambda cap: h.ctx.nthash(dseq, doff, 51, circular=circular, max_hash=mh, out=h.out(U64, len(want) if cap is None else cap))
    return fn


windows_case("nthash-strip-filter", STANDARD, {"nthash_strip": 1}, nthash_fn(1000))
windows_case("nthash-window-filter", STANDARD, {"nthash_strip": 0}, nthash_fn(50))
windows_case("nthash-window-filter-circular", STANDARD, {}, nthash_fn(50, circular=True))
windows_case("nthash-unfiltered", CONTROL, {}, nthash_fn(0))


def encode_fn(h, seq, off, dseq, doff):
    want = h.O.count_windows(seq, off, 31)
    return want, lambda cap: h.ctx.encode_kmers(dseq, doff, 31, out=h.out(U64, len(want) if cap is None else cap))


windows_case("encode_kmers", CONTROL, {}, encode_fn)


def minimizer_fn(h, seq, off, dseq, doff):
    hs, ps = [], []
    for r in range(len(off) - 1):
        rec = seq[int(off[r]):int(off[r + 1])]
        if len(rec) >= 23:
            a, b = h.O.minimizer(rec, 23, 5)
            hs.append(a); ps.append(b)
    want = (np.concatenate(hs), np.concatenate(ps))
    n = len(want[0])
    return want, lambda cap: h.ctx.minimizer(dseq, doff, 23, 5, out=h.out(U64, n if cap is None else cap), out_pos=h.out(U64, n if cap is None else cap))


windows_case("minimizer", STANDARD, {}, minimizer_fn)


def count_fn(h, seq, off, dseq, doff):
    # the retry in the middle of a pipeline: filtered windows (times out, retried) -> sort -> unique (ticketed by then)
    mh = h.O.max_hash(20)
    want = h.O.unique(h.O.sort_u64(h.O.count_windows(seq, off, 21, hashed=True, max_hash=mh)))
    return want, lambda cap: h.ctx.count(dseq, doff, 21, hashed=True, max_hash=mh, out=h.out(U64, len(want) if cap is None else cap))


windows_case("count-hashed-scaled", STANDARD, {}, count_fn)


@case("nthash-strip-filter-short", *STANDARD)
def _(h):
    h.ctx.set_option("nthash_strip", 1)
    seq, off = reads(*READS)
    want, call = nthash_fn(1000)(h, seq, off, h.up(seq, U8), h.up(off, U64))
    h.short(call, want, len(want))


# ---- ukm_grep, ukm_filter, ukm_sample, ukm_rfilter, ukm_tsplit ----------------------------------------------------------------
SEL_N = 3 * 2048 + 517


@memo
def records(n):
    i = np.arange(n, dtype=U64)
    codes = splitmix64(i + U64(31 << 32)) >> U64(2)
    # kept fractions that change from tile to tile
    tax = (splitmix64(i + U64(32 << 32)) % (U64(20) + (i // U64(2048)) * U64(40))).astype(U32)
    return codes, tax


def select_case(name, marks, fn, setup=None):
    @case(name, *marks)
    def _(h):
        if setup:
            setup(h)
        codes, tax = records(SEL_N)
        keep, call = fn(h, codes, tax, h.up(codes, U64), h.up(tax, U32))
        want = (codes[keep], tax[keep])
        assert 0 < len(want[0]) < len(codes)
        outs = lambda cap: dict(out=h.out(U64, len(want[0]) if cap is None else cap), out_taxids=h.out(U32, len(want[0]) if cap is None else cap))
        h.standard(lambda cap: call(**outs(cap)), want)


def grep_keys(invert):
    def fn(h, codes, tax, dk, dt):
        q = codes[splitmix64(codes) % U64(3) == 0][::-1].copy()
        keep = np.isin(codes, q)
        dq = h.up(q, U64)
        return (~keep if invert else keep), lambda **o: h.ctx.grep(dk, dq, taxids=dt, invert=invert, **o)
    return fn


def grep_taxids(h, codes, tax, dk, dt):
    qt = np.arange(0, 200, 3, dtype=U32)
    dq = h.up(qt, U32)
    return np.isin(tax, qt), lambda **o: h.ctx.grep(dk, query_taxids=dq, taxids=dt, **o)


select_case("grep-keys", STANDARD, grep_keys(False))
select_case("grep-keys-invert", STANDARD, grep_keys(True))
select_case("grep-keys-directory", STANDARD, grep_keys(False), setup=lambda h: h.ctx.set_option("grep_lds", 0))
select_case("grep-taxids", STANDARD, grep_taxids)


@case("filter", *STANDARD)
def _(h):
    from test_gpu_select import model_filter
    i = np.arange(SEL_N, dtype=U64)
    # 31-mers with low-complexity stretches in some of them: the low bases of every third code repeat one base
    codes = splitmix64(i + U64(33 << 32)) >> U64(2)
    low = (splitmix64(i + U64(34 << 32)) % U64(3) == 0)
    codes = np.where(low, codes & ~U64((1 << 40) - 1), codes).astype(U64)
    tax = records(SEL_N)[1]
    hit = model_filter(codes, 31)
    want = (codes[~hit], tax[~hit])
    assert 0 < len(want[0]) < len(codes)
    dk, dt = h.up(codes, U64), h.up(tax, U32)
    h.standard(lambda cap: h.ctx.filter(dk, 31, taxids=dt, out=h.out(U64, len(want[0])), out_taxids=h.out(U32, len(want[0]))), want)


@case("sample", *CONTROL)
def _(h):
    # ukm_sample computes every output position from the record index (sample_kernel): no compaction, no look-back
    codes, tax = records(SEL_N)
    sel = np.arange(6, SEL_N, 3)
    want = (codes[sel], tax[sel])
    dk, dt = h.up(codes, U64), h.up(tax, U32)
    h.standard(lambda cap: h.ctx.sample(dk, 7, 3, taxids=dt, out=h.out(U64, len(sel)), out_taxids=h.out(U32, len(sel))), want)


@case("rfilter", *STANDARD)
def _(h):
    import test_gpu_taxsel as T
    T.load_tax(h.ctx)
    codes, tax = T.records(SEL_N, 5)
    keep = T.model_mask("N-n-L", tax)
    want = (codes[keep], tax[keep])
    assert 0 < len(want[0]) < len(codes)
    f = T.to_rank_filter(h.L, T.FILTERS["N-n-L"])
    dk, dt = h.up(codes, U64), h.up(tax, U32)
    h.standard(lambda cap: h.ctx.rfilter(dk, f, taxids=dt, out=h.out(U64, len(want[0])), out_taxids=h.out(U32, len(want[0]))), want)


def tsplit_model(codes, tax):
    order = np.argsort(tax, kind="stable")
    st = tax[order]
    heads = np.flatnonzero(np.r_[True, st[1:] != st[:-1]])
    return codes[order], st[heads], np.r_[heads, len(tax)].astype(U64)


@case("tsplit", *STANDARD)
def _(h):
    codes, tax = records(SEL_N)
    want = tsplit_model(codes, tax)
    g = len(want[1])
    assert g > 100
    dk, dt = h.up(codes, U64), h.up(tax, U32)
    # (all three outputs given: no size query in front of the call)
    h.standard(lambda cap: h.ctx.tsplit(dk, dt, out=h.out(U64, len(codes)), group_taxids=h.out(U32, g), group_off=h.out(U64, g + 1)), want)


@case("tsplit-short", *STANDARD)
def _(h):
    codes, tax = records(SEL_N)
    want = tsplit_model(codes, tax)
    g = len(want[1])
    dk, dt = h.up(codes, U64), h.up(tax, U32)
    def call(cap):
        c = g if cap is None else cap
        return h.ctx.tsplit(dk, dt, out=h.out(U64, len(codes)), group_taxids=h.out(U32, c), group_off=h.out(U64, c + 1))
    h.short(call, want, g)


# ---- ukm_locate, ukm_map, ukm_map_gapped ------------------------------------------------------------------------------------
MAP_K = 31
MAP_LENS = [3000, 17, 4, 2048 + MAP_K - 1, 6000, MAP_K, MAP_K - 1, 9000]      # 20,000 windows: 10 tiles of 2048


@memo
def genome():
    rng = np.random.default_rng(131)
    acgt = np.frombuffer(b"ACGT", dtype=U8)
    recs = [acgt[rng.integers(0, 4, n)].copy() for n in MAP_LENS]
    piece = recs[0][10:10 + 3 * MAP_K].copy()
    recs[0][200:200 + len(piece)] = piece
    for r in recs[1:]:
        if len(r) > 100 + len(piece):
            r[50:50 + len(piece)] = piece
    off = np.zeros(len(recs) + 1, dtype=U64)
    off[1:] = np.cumsum(MAP_LENS)
    return np.concatenate(recs), off


def genome_model(h, circular):
    import map_model as M
    k = ("genome_model", circular)
    if k not in _cache:
        bases, off = genome()
        wins = M.windows(h.O, bases, off, MAP_K, False, circular)
        _cache[k] = wins
    return _cache[k]


def map_codes(h):
    if "map_codes" not in _cache:
        allw = np.unique(np.array([c for w in genome_model(h, True) if w is not None for c in w], dtype=U64))
        _cache["map_codes"] = allw[np.random.default_rng(31).random(len(allw)) < 0.8]
    return _cache["map_codes"]


def cols(rows, dtypes):
    return tuple(np.array([r[i] for r in rows], dtype=dt) for i, dt in enumerate(dtypes))


for _circ in (False, True):
    @case("locate%s" % ("-circular" if _circ else ""), *STANDARD)
    def _(h, circular=_circ):
        from test_gpu_map import model_locate
        bases, off = genome()
        wins = genome_model(h, circular)
        q = map_codes(h)[::7][::-1].copy()
        want = cols(model_locate(wins, q.tolist()), (U64, U32, U64))
        n = len(want[0])
        assert n > 100
        db, do, dq = h.up(bases, U8), h.up(off, U64), h.up(q, U64)
        h.standard(lambda cap: h.ctx.locate(db, do, MAP_K, dq, circular=circular, outs=[h.out(U64, n), h.out(U32, n), h.out(U64, n)]), want)


def map_case(name, circular, x, X, gapped, allow_multi=False):
    @case(name, *STANDARD)
    def _(h):
        import map_model as M
        bases, off = genome()
        wins = genome_model(h, circular)
        codes = map_codes(h)
        n_rec = len(MAP_LENS)
        goff = np.arange(n_rec + 1, dtype=U64)
        cls = M.classes(wins, list(range(n_rec)), set(codes.tolist()), allow_multi)
        want = cols(M.model_map_gapped(cls, MAP_LENS, MAP_K, circular, MAP_K, x, X), (U32, U64, U64))
        n = len(want[0])
        assert n > 20
        db, do, dg, ds = h.up(bases, U8), h.up(off, U64), h.up(goff, U64), h.up(codes, U64)
        def call(cap):
            outs = [h.out(U32, n), h.out(U64, n), h.out(U64, n)]
            if gapped:
                return h.ctx.map_gapped(db, do, dg, MAP_K, ds, circular=circular, allow_multi=allow_multi, min_len=MAP_K, max_gap_size=x,
                                        max_gap_num=X, outs=outs)
            return h.ctx.map(db, do, dg, MAP_K, ds, allow_multi=allow_multi, min_len=MAP_K, outs=outs)
        h.standard(call, want)


map_case("map", False, 0, 0, False)
map_case("map-allow-multi", False, 0, 0, False, allow_multi=True)
map_case("map_gapped-gaps", False, 2, 3, True)
map_case("map_gapped-circular", True, 0, 0, True)
map_case("map_gapped-circular-gaps", True, 3, 255, True)


# ---- the chained fold -------------------------------------------------------------------------------------------------------
@memo
def fold_files():
    """five files: the first spans 3.3 plain tiles (9.3 with taxids), the later ones keep or remove a different share each"""
    A, _ = sets(2 * SMALL)
    later = [A[splitmix64(A ^ U64(900 + i)) % U64(10) < U64(9 - i)] for i in range(4)]
    return [A] + later


for _which in ("inter", "diff"):
    for _tax in (False, True):
        @case("fold-chained-%s%s" % (_which, "-tax" if _tax else ""), *STANDARD)
        def _(h, which=_which, with_tax=_tax):
            # no range fold, no probe fold: one link per file (fold_chained).  Every link's first launch times out; the flags are
            # read at the end and the synchronous fold answers -- not UKM_ERR_UNSORTED for the partly written running result
            h.ctx.set_option("no_fold", 1)
            h.ctx.set_option("no_pfold", 1)
            tax = load_forest(h) if with_tax else None
            ss = fold_files()
            pool = spine_forest()[4]
            ts = [pool[(splitmix64(s ^ U64(77 + i)) % U64(len(pool))).astype(np.int64)] for i, s in enumerate(ss)] if with_tax else None
            want = getattr(h.O, which)(ss, ts, tax)
            n = len(want[0]) if with_tax else len(want)
            assert 0 < n < len(ss[0])
            ds = [h.up(s, U64) for s in ss]
            dt = [h.up(t, U32) for t in ts] if with_tax else None
            h.standard(lambda cap: getattr(h.ctx, which)(ds, dt, out=h.out(U64, n), out_taxids=h.out(U32, n) if with_tax else None), want)


NAMES = [c[0] for c in CASES]
assert len(set(NAMES)) == len(NAMES)


def main(out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    h = H()
    only = os.environ.get("LB_RETRY_ONLY")       # (a substring of the case names: a developer's narrow run)
    with open(out_path, "w") as fh:
        for name, fn, _ in CASES:
            if only and only not in name:
                continue
            rec = {"name": name, "error": None}
            t0 = time.time()
            fatal = False
            try:
                h.begin()
                fn(h)
            except Exception as e:
                rec["error"] = traceback.format_exc()
                # a HIP error may be a GPU fault: start nothing more on the device
                fatal = (isinstance(e, h.L.UkmError) and e.code == h.L.ERR_HIP) or "HIP error" in str(e) or "hipError" in str(e)
            rec["wd"] = h.wd
            rec["seconds"] = round(time.time() - t0, 3)
            fh.write(json.dumps(rec) + "\n")
            fh.flush()
            if fatal:
                sys.stderr.write("HIP error in case %s: stopping\n%s" % (name, rec["error"]))
                return 3
            try:
                h.end()
            except Exception:
                sys.stderr.write("closing the context of case %s failed: stopping\n%s" % (name, traceback.format_exc()))
                return 3
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
