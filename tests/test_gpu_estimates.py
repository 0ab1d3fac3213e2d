"""Inputs that defeat every SAMPLED size estimate of an internal buffer, so that the way out behind each estimate runs.

Three buffers are sized from an estimate plus 2^20 records of slack instead of an upper bound; with fewer than about
10^6 windows or later records the `min(estimate, bound)` picks the bound and the overflow branch is dead code:

  * ukm_count's window buffer under a Scaled filter: 1.5 x the expected share of the windows + 2^20.  A low-complexity
    record whose one canonical hash lies below max_hash keeps EVERY window: the window pass runs a second time into a
    buffer of the exact size (stat "count_window_retries"), and UKM_ERR_CAPACITY stays what the header says it is, a
    statement about the caller's out_cap.
  * the miss list of the hash-probe union, in the plain pass (pu2_probe_kernel), the pass with per-record taxids
    (pt_probe_kernel) and the pass over files with one taxid each (pr_probe_kernel): later x (2 x sampled miss rate +
    0.01) + 2^20.  The hit sample opens at most 16 later files -- of 32, the even ones.  Here the odd ones consist of
    codes no other file holds: the sample sees hits only, the list overflows behind guarded stores, the pass raises its
    overflow flag (stat "punion_flags"), the route declines and the general merge answers.

test_inputs_defeat_the_estimates (no GPU) recomputes both estimates from the oracle's numbers: whoever changes an
estimate is told there to rebuild these inputs, instead of the GPU tests going vacuous."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conftest import synth_tree  # noqa: E402

U64, U32 = np.uint64, np.uint32

# ---- the estimates these inputs are built to defeat (copies of the formulas: see the module docstring) -------------------
SLACK = 1 << 20


def count_window_estimate(bases, max_hash):
    """the estimate this input is built to defeat: ukm_count's window buffer (ukm_encode.hip: count_window_estimate)"""
    return 1.5 * (2.0 * max_hash / 2.0 ** 64) * bases + SLACK


def miss_list_estimate(later, n0):
    """the estimate this input is built to defeat: the probe union's miss list after a sample without a single miss
    (ukm_probe_union.hip / ukm_probe_ranked.hip), with its chunk slack: one chunk of 64 per wave of 16 per range of 2048"""
    return 0.01 * later + SLACK + later / 32 + 64 * 16 * -(-n0 // 2048)


PU_FLAG_OVERFLOW = 2    # include/unikmer_hip.h, stat "punion_flags"


# ---- A: low-complexity records under --scale ---------------------------------------------------------------------------
# (name, k, scale, random bases, the repeated base and how often): poly-A's canonical 51-mer hashes to 0.04257 x 2^64, below
# 2^64 / 23; poly-C's canonical 31-mer to 0.1288 x 2^64, below 2^64 / 7
COUNT_INPUTS = {"polyA-k51-s23": (51, 23, 2_000_000, b"A", 2_000_000),
                "polyC-k31-s7": (31, 7, 1_000_000, b"C", 3_000_000)}


@functools.lru_cache(maxsize=None)
def count_input(name):
    k, scale, nrand, base, nrep = COUNT_INPUTS[name]
    rng = np.random.default_rng(k)
    seq = np.concatenate([np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, nrand)],
                          np.full(nrep, base[0], dtype=np.uint8)])
    off = np.array([0, nrand, nrand + nrep], dtype=U64)
    return seq, off, k, scale


@functools.lru_cache(maxsize=None)
def count_windows_sorted(name, circular):
    """every window the Scaled filter keeps, sorted (the oracle, once per input and shape; shared, never changed)"""
    from oracle import oracle as O
    seq, off, k, scale = count_input(name)
    w = O.sort_u64(O.count_windows(seq, off, k, hashed=True, canonical=True, circular=circular, max_hash=O.max_hash(scale)))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def count_expected(name, circular, mode):
    from oracle import oracle as O
    e = O.unique(count_windows_sorted(name, circular), mode=mode)
    e.setflags(write=False)
    return e


# ---- B: 32 later files of which the hit sample opens the even ones -------------------------------------------------------
NLATER, SUBSET, PRIVATE, UNIVERSE = 32, 100_000, 150_000, 400_000
BASE_FILES = {"plain": 8, "record-taxids": 4, "file-taxids": 8}


@functools.lru_cache(maxsize=None)
def union_input(case):
    """(base files, later files): the universe are EVEN 40-bit codes, evenly spread; a base file draws each with p = 0.6
    (about 240,000 codes: strictly the largest files, so they become the base set); later file 2 i is a 100,000-record
    subset of the universe; later file 2 i + 1 holds 150,000 ODD codes of its own, every 16th of 2,400,000 spread over the
    same span (the range-load guard sees an even load)"""
    rng = np.random.default_rng(4000 + BASE_FILES[case] + len(case))
    uni = (np.arange(UNIVERSE, dtype=U64) * U64((1 << 39) // UNIVERSE)) * U64(2)
    base = [uni[rng.random(UNIVERSE) < 0.6] for _ in range(BASE_FILES[case])]
    nodd = NLATER // 2
    priv = (np.arange(nodd * PRIVATE, dtype=U64) * U64((1 << 39) // (nodd * PRIVATE))) * U64(2) + U64(1)
    later = []
    for i in range(nodd):
        later.append(np.sort(rng.choice(uni, SUBSET, replace=False)))
        later.append(np.ascontiguousarray(priv[i::nodd]))
    for f in base + later:
        f.setflags(write=False)
    return base, later


@functools.lru_cache(maxsize=None)
def union_taxids(case):
    """per-record taxids (arrays) or one taxid per file (ints) for base + later files; None for the plain case"""
    base, later = union_input(case)
    T = len(synth_tree(5, 8)[0])
    rng = np.random.default_rng(77)
    if case == "record-taxids":
        return [rng.integers(1, T + 1, len(f)).astype(U32) for f in base + later]
    if case == "file-taxids":
        return [int(t) for t in rng.integers(1, T + 1, len(base) + len(later))]
    return None


def _as_arrays(files, taxs):
    return None if taxs is None else [np.full(len(f), t, U32) if isinstance(t, int) else t for f, t in zip(files, taxs)]


@functools.lru_cache(maxsize=None)
def union_expected(case, even_only):
    from oracle import oracle as O
    base, later = union_input(case)
    taxs = union_taxids(case)
    files = later[0::2] if even_only else base + later
    if taxs is not None:
        taxs = taxs[len(base)::2] if even_only else taxs
        child, parent = synth_tree(5, 8)
        return O.union(files, _as_arrays(files, taxs), O.Taxonomy(child, parent))
    return O.union(files)


# ---- D: the inputs still do what they are for (oracle only, no GPU) ------------------------------------------------------
def test_inputs_defeat_the_estimates():
    """If this fails after a change to one of the two estimates, REBUILD THE INPUT so that it overflows the new estimate (and
    update the copy of the formula above): the GPU tests below would otherwise pass without running a single overflow branch."""
    from oracle import oracle as O
    for name in COUNT_INPUTS:
        seq, off, k, scale = count_input(name)
        for circular in (False, True):
            kept, est = len(count_windows_sorted(name, circular)), count_window_estimate(len(seq), O.max_hash(scale))
            assert kept > est, "%s circular=%d: %d windows pass the filter, the estimate this input is built to defeat allows %d" % (name, circular, kept, est)
            assert est < len(seq) + 1, "the estimate is not below the exact bound: min() would pick the bound"
            # (one code with two million copies and more: the caller's out needs a small fraction of the windows)
            assert 1 <= len(count_expected(name, circular, O.REPEATED)) < len(count_expected(name, circular, O.UNIQUE)) < kept / 2
    for case, k0 in BASE_FILES.items():
        base, later = union_input(case)
        assert len(later) == NLATER and min(len(f) for f in base) > max(len(f) for f in later), "the base files must be the largest"
        everything_else = np.unique(np.concatenate(base + later[0::2]))
        odd = np.concatenate(later[1::2])
        private = len(odd)
        assert len(np.unique(odd)) == private and not np.isin(odd, everything_else).any(), "odd files hold codes of their own"
        assert all(np.all(f[1:] > f[:-1]) for f in base + later), "sorted sets"
        n_later = sum(len(f) for f in later)
        n0 = len(np.unique(np.concatenate(base)))
        # (the pass over files with one taxid each probes the base files too and is sized from all records: the larger slack)
        for records in (n_later, n_later + sum(len(f) for f in base)):
            est = miss_list_estimate(records, n0)
            assert private > est, "%s: %d private codes, the estimate this input is built to defeat allows %d" % (case, private, est)
            assert est < n_later, "the estimate is not below the exact bound"
        # what the hit sample sees: the even files, nearly all of whose records are in the base set
        hits = np.mean([np.isin(f, np.unique(np.concatenate(base))).mean() for f in later[0::2]])
        assert hits > 0.95, (case, hits)
        assert n_later <= 6_500_000 and len(count_input("polyA-k51-s23")[0]) <= 4_000_000


# ---- GPU -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    from oracle import oracle as O
    from unikmer_amd import lib as L
    ctx = L.Context(0)
    child, parent = synth_tree(5, 8)
    ctx.taxonomy_load(child, parent)
    yield O, L, ctx
    ctx.close()


def _dev(x):
    import torch
    signed = {np.dtype(U64): np.int64, np.dtype(U32): np.int32, np.dtype(np.uint8): np.uint8}[x.dtype]
    return torch.from_numpy(np.array(x).view(signed)).cuda()


def _host(x, dtype=U64):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy().view(dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("resident", ["host", "device"])
@pytest.mark.parametrize("force_ticket", [0, 1])
@pytest.mark.parametrize("circular", [False, True])
@pytest.mark.parametrize("name", list(COUNT_INPUTS))
def test_count_outgrows_its_window_estimate(env, name, circular, force_ticket, resident):
    """ukm_count on a record that keeps every window under --scale: bit for bit the oracle's distinct / repeated / singleton
    set, one repeated window pass per call, UKM_ERR_CAPACITY only for the caller's out (with the size needed), and a context
    that answers ordinary calls afterwards.  Not circular: the strip filter's candidate list overflows first and the
    general kernel meets the small buffer; circular: the general kernel at once.

    Before the fix every call here failed with UKM_ERR_CAPACITY and needed == 0."""
    O, L, ctx = env
    seq, off, k, scale = count_input(name)
    mh = O.max_hash(scale)
    dseq, doff = (_dev(seq), _dev(off)) if resident == "device" else (seq, off)

    def out_of(n):
        return _dev(np.zeros(n, U64)) if resident == "device" else np.zeros(n, U64)

    ctx.set_option("force_ticket", force_ticket)
    try:
        retries = ctx.stat("count_window_retries")
        for mode in (L.UNIQUE, L.REPEATED, L.SINGLETON):
            exp = count_expected(name, circular, mode)
            got = ctx.count(dseq, doff, k, canonical=True, circular=circular, hashed=True, max_hash=mh, mode=mode)
            retries += 1
            assert ctx.stat("count_window_retries") == retries, "the window pass was not repeated: the input no longer defeats the estimate"
            assert np.array_equal(_host(got), exp), (name, circular, mode)
            # the caller's buffer: exactly large enough, one short, and the size query
            got = ctx.count(dseq, doff, k, circular=circular, hashed=True, max_hash=mh, mode=mode, out=out_of(len(exp)))
            assert np.array_equal(_host(got), exp), (name, circular, mode, "exact out_cap")
            caps = sorted({len(exp) - 1, 0})
            for cap in caps:
                with pytest.raises(L.CapacityError) as e:
                    ctx.count(dseq, doff, k, circular=circular, hashed=True, max_hash=mh, mode=mode, out=out_of(cap))
                assert e.value.needed == len(exp), (name, circular, mode, cap)
            retries += 1 + len(caps)
            assert ctx.stat("count_window_retries") == retries
        # the context afterwards: an ordinary count and a 2-way operation
        rng = np.random.default_rng(5)
        s2 = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 50_000)]
        o2 = np.array([0, 20_000, 50_000], dtype=U64)
        before = ctx.stat("count_window_retries")
        assert np.array_equal(ctx.count(s2, o2, 31), O.unique(O.sort_u64(O.count_windows(s2, o2, 31))))
        assert np.array_equal(ctx.count(s2, o2, 31, hashed=True, max_hash=mh), O.unique(O.sort_u64(O.count_windows(s2, o2, 31, hashed=True, max_hash=mh))))
        assert ctx.stat("count_window_retries") == before
        a, b = np.unique(rng.integers(0, 1 << 40, 30_000, dtype=U64)), np.unique(rng.integers(0, 1 << 40, 30_000, dtype=U64))
        b = np.union1d(b, a[::3])
        for op, ref in ((L.OP_UNION, O.union), (L.OP_INTER, O.inter), (L.OP_DIFF, O.diff)):
            assert np.array_equal(ctx.setop2(op, a, b), ref([a, b])), op
    finally:
        ctx.set_option("force_ticket", None)


def _union(ctx, files, taxs):
    if taxs is None:
        return ctx.union(files), None
    return ctx.union(files, taxs)


@pytest.mark.gpu
@pytest.mark.parametrize("case,punion,poison", [(c, m, None) for c in BASE_FILES for m in (1, 2)] + [("plain", 1, 0xAA)])
def test_probe_union_outgrows_its_miss_list(env, case, punion, poison):
    """The union of files whose hit sample promises a short miss list and whose odd files bring 2.4 M new codes: the probe
    pass (plain, with per-record taxids, over files with one taxid each) overflows the list behind guarded stores, says so
    in its flag word, the route declines and the general merge gives the oracle's union; the same context then takes the
    probe route for the even files alone.  (`merge -d` through the counting probes is not here: its list bound is exact.)

    What this cannot tell: WHICH probe kernel raised the flag -- all three read-backs store into the one stat, and a
    file-taxids case that left the ranked pass for the generic tables (option "punion_ranked" 0) would pass all the same;
    the case names say which pass the route picks for such input today.  miss_list_estimate's chunk slack is the plain
    pass's (ranges of 2,048 base entries); the passes with taxids size their ranges by the number of compute units, so
    for them the CPU-side guard holds the formula only approximately (the private codes exceed it by a million) and it is
    the flag assertion here that says the list did overflow."""
    O, L, ctx = env
    base, later = union_input(case)
    taxs = union_taxids(case)
    opts = {"punion": punion, "ws_poison": poison}
    for key, v in opts.items():
        if v is not None:
            ctx.set_option(key, v)
    try:
        # (an earlier call's flags cannot satisfy the assertion below: a small union through the probe route leaves 0 first)
        assert np.array_equal(ctx.union(later[0:4:2] + base[:2]), O.union(later[0:4:2] + base[:2]))
        assert ctx.stat("punion_attempts") >= 1 and ctx.stat("punion_flags") == 0
        gk, gt = _union(ctx, base + later, taxs)
        assert ctx.last_route() != L.ROUTE_PUNION, "the probe route answered: its miss list did not overflow"
        assert ctx.stat("punion_attempts") >= 1, "the probe route was never tried"
        assert ctx.stat("punion_flags") & PU_FLAG_OVERFLOW, "flags = %d" % ctx.stat("punion_flags")
        exp = union_expected(case, False)
        if taxs is None:
            assert np.array_equal(gk, exp)
        else:
            assert np.array_equal(gk, exp[0]) and np.array_equal(gt, exp[1])
        # the context is in no bad state: the even files alone go through the probe route
        even = later[0::2]
        gk, gt = _union(ctx, even, None if taxs is None else taxs[len(base)::2])
        assert ctx.last_route() == L.ROUTE_PUNION and ctx.stat("punion_flags") == 0
        exp = union_expected(case, True)
        if taxs is None:
            assert np.array_equal(gk, exp)
        else:
            assert np.array_equal(gk, exp[0]) and np.array_equal(gt, exp[1])
    finally:
        for key in opts:
            ctx.set_option(key, None)
