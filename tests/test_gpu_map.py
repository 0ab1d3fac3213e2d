"""ukm_locate / ukm_map and the `locate` / `map` commands on the GPU.

The expected values come from a small model in this file -- a dict of code -> positions and the plain loops of locate.go
and map.go (at -x 0 -X 0) -- over windows from the CPU oracle's kmer_iter / hash_iter; never from the library under test.
"""
import os
import subprocess

import numpy as np
import pytest

from conftest import AMUC, GOLDEN, IAI39, MG1655

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from unikmer_amd import lib
    from oracle import oracle
    ctx = lib.Context(0)
    yield lib, ctx, oracle
    ctx.close()


# ---- the model ---------------------------------------------------------------------------------------------------------
def windows(O, bases, off, k, hashed=False, circular=False):
    """per record: the list of canonical window values, or None for a record shorter than k (sketches.ErrShortSeq)"""
    it = O.hash_iter if hashed else O.kmer_iter
    out = []
    for r in range(len(off) - 1):
        seq = bases[int(off[r]):int(off[r + 1])]
        out.append(it(seq, k, True, circular).tolist() if len(seq) >= k else None)
    return out


def model_locate(wins, queries):
    """locate.go:143-288"""
    m = {}
    for r, w in enumerate(wins):
        if w is None:
            continue
        for i, code in enumerate(w):
            m.setdefault(code, []).append((r, i))
    out = []
    for j, code in enumerate(queries):
        locs = m.get(code)
        if locs is not None:
            out.extend((j, r, i) for r, i in locs)
            del m[code]
    return out


def model_map(wins, genome_of, codes, k, allow_multi, min_len, max_gap_size=0, max_gap_num=0):
    """map.go:116-491 without --circular; genome_of[r] = genome of record r (the first pass's numbering, also in the second)"""
    m = set(codes)
    m2 = {}
    if not allow_multi:
        for r, w in enumerate(wins):
            if w is None:
                continue
            g = m2.setdefault(genome_of[r], {})
            for code in w:
                if code not in g:
                    g[code] = False
                elif not g[code]:
                    g[code] = True
    out = []
    last_gap_num = lastmatch = 0
    flag = True
    for r, w in enumerate(wins):
        if w is None:
            continue
        c, start, gaps, gap_nums = 0, -1, 0, 0
        g = m2.get(genome_of[r], {})
        for i, code in enumerate(w):
            if code in m:
                gaps = 0
                if not allow_multi and g.get(code, False):
                    if last_gap_num <= max_gap_num and start >= 0 and lastmatch - start + k >= min_len:
                        out.append((r, start, lastmatch + k))
                    c, start, flag = 0, -1, True
                else:
                    c += 1
                    if c == 1 and flag:
                        start, gap_nums, gaps, last_gap_num = i, 0, 0, 0
                if c >= 1:
                    lastmatch, last_gap_num = i, gap_nums
            else:
                gaps += 1
                if gaps == 1:
                    gap_nums += 1
                if gaps <= max_gap_size and gap_nums <= max_gap_num:
                    c = 0
                    if start >= 0:
                        flag = False
                else:
                    if last_gap_num <= max_gap_num and start >= 0 and lastmatch - start + k >= min_len:
                        out.append((r, start, lastmatch + k))
                    c, start, flag = 0, -1, True
        if last_gap_num <= max_gap_num + 1 and start >= 0 and lastmatch - start + k >= min_len:
            out.append((r, start, lastmatch + k))
    return out


def _rows(*cols):
    return [tuple(int(v) for v in row) for row in zip(*cols)]


def _dev(x, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype).view({np.uint64: np.int64, np.uint32: np.int32, np.uint8: np.uint8}[dtype])).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype) if hasattr(t, "cpu") else t


def _genome(seed, lens, k):
    """random records with planted repeats: a piece of record 0 reappears inside the later records and twice in record 0"""
    rng = np.random.default_rng(seed)
    recs = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy() for n in lens]
    piece = recs[0][10:10 + 3 * k].copy()
    if len(recs[0]) > 400:
        recs[0][200:200 + len(piece)] = piece
    for r in recs[1:]:
        if len(r) > 100 + len(piece):
            r[50:50 + len(piece)] = piece
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    return np.concatenate(recs), off


# ---- ukm_locate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,hashed", [(4, False), (23, False), (31, False), (32, False), (23, True), (51, True)])
@pytest.mark.parametrize("circular", [False, True])
def test_locate_matches_model(env, k, hashed, circular):
    lib, ctx, O = env
    bases, off = _genome(k * 7 + hashed, [3000, k - 1, 1500, 700, k], k)      # one record shorter than k, one of exactly k
    wins = windows(O, bases, off, k, hashed, circular)
    allw = np.array([c for w in wins if w is not None for c in w], dtype=np.uint64)
    rng = np.random.default_rng(k)
    present = allw[rng.integers(0, len(allw), 400)]
    absent = rng.integers(0, 1 << 62, 100, dtype=np.uint64) | np.uint64(1 << 63 if hashed else 0)
    q = np.concatenate([present, absent, present[:50]])                         # duplicates: behind and between
    rng.shuffle(q)
    want = model_locate(wins, q.tolist())
    assert len(want) >= 400
    gq, gr, gp = ctx.locate(bases, off, k, q, circular=circular, hashed=hashed)
    assert _rows(gq, gr, gp) == want
    # device pointers in, device pointers out
    dq, dr, dp = ctx.locate(_dev(bases, np.uint8), _dev(off, np.uint64), k, _dev(q, np.uint64), circular=circular, hashed=hashed)
    assert dq.is_cuda and _rows(_host(dq, np.uint64), _host(dr, np.uint32), _host(dp, np.uint64)) == want
    # one entry short: the exact size comes back
    with pytest.raises(lib.CapacityError):
        ctx.locate(bases, off, k, q, circular=circular, hashed=hashed, out_cap=len(want) - 1)
    import ctypes as C
    n = C.c_uint64()
    cap = len(want) - 1
    oq, orc, op = np.empty(cap, np.uint64), np.empty(cap, np.uint32), np.empty(cap, np.uint64)
    rc = ctx.L.ukm_locate(ctx.h, bases.ctypes.data, off.ctypes.data, len(off) - 1, k, int(circular), int(hashed), q.ctypes.data, len(q),
                          oq.ctypes.data, orc.ctypes.data, op.ctypes.data, cap, C.byref(n))
    assert rc == lib.ERR_CAPACITY and n.value == len(want)
    g2 = ctx.locate(bases, off, k, q, circular=circular, hashed=hashed, out_cap=len(want))
    assert _rows(*g2) == want


def test_locate_edges(env):
    lib, ctx, O = env
    k = 23
    bases, off = _genome(5, [2000, 900], k)
    gq, gr, gp = ctx.locate(bases, off, k, np.empty(0, np.uint64))              # nq = 0
    assert len(gq) == len(gr) == len(gp) == 0
    q = np.array(windows(O, bases, off, k)[1][:5], dtype=np.uint64)
    short = np.zeros(3, dtype=np.uint64)
    short[1:] = [10, 15]                                                        # only records shorter than k
    assert len(ctx.locate(bases[:15], short, k, q)[0]) == 0
    bad = bases.copy()
    bad[100] = ord("*")
    with pytest.raises(lib.IllegalBaseError):
        ctx.locate(bad, off, k, q)
    with pytest.raises(lib.UkmError) as e:
        ctx.locate(bases, off, 33, q)
    assert e.value.code == lib.ERR_K


def test_locate_many_windows(env):
    """enough windows for several tiles of the join and the bucket route of the sort; every window is a hit"""
    lib, ctx, O = env
    k = 15
    rng = np.random.default_rng(3)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 300_000)]
    off = np.array([0, 120_000, 120_010, 300_000], dtype=np.uint64)
    wins = windows(O, bases, off, k)
    q = np.unique(np.array([c for w in wins if w for c in w], dtype=np.uint64))
    rng.shuffle(q)
    want = model_locate(wins, q.tolist())
    assert len(want) == sum(len(w) for w in wins if w)
    assert _rows(*ctx.locate(bases, off, k, q)) == want
    # both routes forced: lookups in genome order / all (code, window) pairs sorted first
    for route in (0, 1):
        ctx.set_option("map_sorted", route)
        try:
            assert _rows(*ctx.locate(bases, off, k, q)) == want, route
            assert _rows(*ctx.locate(bases, off, k, np.concatenate([q[:1000], q[:1000]]))) == model_locate(wins, q[:1000].tolist() * 2), route
        finally:
            ctx.set_option("map_sorted", None)


# ---- ukm_map -------------------------------------------------------------------------------------------------------------
def _set_of(wins, picks):
    """sorted distinct codes of the windows picks = [(record, first, last)] (inclusive)"""
    return np.unique(np.array([c for r, a, b in picks for c in wins[r][a:b + 1]], dtype=np.uint64))


def _map_both(ctx, bases, off, goff, k, codes, **kw):
    """host pointers and device pointers must agree"""
    h = _rows(*ctx.map(bases, off, goff, k, codes, **kw))
    d = ctx.map(_dev(bases, np.uint8), _dev(off, np.uint64), _dev(goff, np.uint64), k, _dev(codes, np.uint64), **kw)
    assert _rows(_host(d[0], np.uint32), _host(d[1], np.uint64), _host(d[2], np.uint64)) == h
    return h


@pytest.mark.parametrize("k,hashed", [(23, False), (31, True)])
def test_map_runs_and_boundaries(env, k, hashed):
    lib, ctx, O = env
    rng = np.random.default_rng(11)
    recs = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)] for n in (1000, 10, 800, 600)]
    bases = np.concatenate(recs)
    off = np.zeros(5, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    wins = windows(O, bases, off, k, hashed)
    n0, n2 = len(wins[0]), len(wins[2])
    min_len = 60
    L = min_len - k                       # last - first of a run of exactly min_len bases
    picks = [(0, 0, 99),                  # touches the start of a record
             (0, n0 - 120, n0 - 1),       # touches the end of record 0 ...
             (2, 0, 79),                  # ... and goes on at the start of record 2 (record 1 is shorter than k): must split
             (2, 200, 200 + L),           # exactly min_len
             (2, 400, 400 + L - 1),       # min_len - 1: dropped
             (3, len(wins[3]) - 50, len(wins[3]) - 1)]
    codes = _set_of(wins, picks)
    goff = np.arange(5, dtype=np.uint64)
    want = model_map(wins, [0, 1, 2, 3], codes.tolist(), k, True, min_len)
    assert (0, 0, 99 + k) in want and (0, n0 - 120, n0 - 1 + k) in want and (2, 0, 79 + k) in want
    assert (2, 200, 200 + L + k) in want and not any(s == 400 for r, s, e in want if r == 2)
    for allow in (True, False):
        got = _map_both(ctx, bases, off, goff, k, codes, hashed=hashed, allow_multi=allow, min_len=min_len)
        assert got == model_map(wins, [0, 1, 2, 3], codes.tolist(), k, allow, min_len), allow
    # min_len 1: every run, also single windows
    assert _map_both(ctx, bases, off, goff, k, codes, hashed=hashed, allow_multi=True, min_len=1) == \
        model_map(wins, [0, 1, 2, 3], codes.tolist(), k, True, 1)
    assert n2 > 500


def test_map_multiple_mapped_and_genome_grouping(env):
    lib, ctx, O = env
    k = 21
    rng = np.random.default_rng(23)
    recs = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy() for n in (1500, 1200, 900)]
    recs[0][700:700 + k] = recs[0][100:100 + k]      # window 100 of record 0 reappears as window 700 of the SAME record
    recs[1][300:300 + k] = recs[0][400:400 + k]      # window 400 of record 0 reappears in ANOTHER record
    bases = np.concatenate(recs)
    off = np.zeros(4, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in recs])
    wins = windows(O, bases, off, k)
    assert wins[0][100] == wins[0][700] and wins[0][400] == wins[1][300]
    codes = _set_of(wins, [(0, 50, 150), (0, 350, 450), (0, 650, 750), (1, 250, 350), (2, 10, 200)])
    per_rec, one = np.arange(4, dtype=np.uint64), np.array([0, 3], dtype=np.uint64)
    res = {}
    for name, goff, gof in (("per_rec", per_rec, [0, 1, 2]), ("one", one, [0, 0, 0])):
        for allow in (False, True):
            want = model_map(wins, gof, codes.tolist(), k, allow, 30)
            res[name, allow] = _map_both(ctx, bases, off, goff, k, codes, allow_multi=allow, min_len=30)
            assert res[name, allow] == want, (name, allow)
    # the repeat inside record 0 splits its runs without -M whatever the grouping; the repeat across records only when the
    # records are one genome
    def covers(regions, rec, w):
        return any(r == rec and s <= w and w + k <= e for r, s, e in regions)
    assert (0, 50, 150 + k) in res["per_rec", True] and not covers(res["per_rec", False], 0, 100) and not covers(res["one", False], 0, 700)
    assert covers(res["per_rec", False], 0, 99 - k) and covers(res["per_rec", False], 0, 101 + k)   # the run goes on around the repeat
    assert (0, 350, 450 + k) in res["per_rec", False] and not covers(res["one", False], 0, 400) and not covers(res["one", False], 1, 300)
    assert res["per_rec", False] != res["one", False] and res["per_rec", True] == res["one", True]
    # set with duplicates = the same set; empty set = nothing; unsorted set = error
    dup = np.sort(np.concatenate([codes, codes[::3]]))
    assert _rows(*ctx.map(bases, off, per_rec, k, dup, min_len=30)) == res["per_rec", False]
    assert len(ctx.map(bases, off, per_rec, k, np.empty(0, np.uint64), min_len=30)[0]) == 0
    with pytest.raises(lib.UnsortedError):
        ctx.map(bases, off, per_rec, k, codes[::-1].copy(), min_len=30)
    # both routes forced (lookups in genome order / every window sorted first) are the same function
    for route in (0, 1):
        ctx.set_option("map_sorted", route)
        try:
            for allow in (False, True):
                assert _rows(*ctx.map(bases, off, one, k, codes, allow_multi=allow, min_len=30)) == res["one", allow], route
                assert _rows(*ctx.map(bases, off, per_rec, k, codes, allow_multi=allow, min_len=30)) == res["per_rec", allow], route
        finally:
            ctx.set_option("map_sorted", None)
    # one region short
    with pytest.raises(lib.CapacityError):
        ctx.map(bases, off, per_rec, k, codes, min_len=30, out_cap=len(res["per_rec", False]) - 1)


def test_map_random_dense(env):
    """a set that covers most of a repetitive genome: many short runs, many multiple-mapped codes, several tiles"""
    lib, ctx, O = env
    k = 11
    rng = np.random.default_rng(5)
    unit = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 5000)]
    bases = np.concatenate([unit, unit[::-1], unit[1000:3000], np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 40000)]])
    off = np.array([0, 7000, 7005, 30000, len(bases)], dtype=np.uint64)
    wins = windows(O, bases, off, k)
    allw = np.unique(np.array([c for w in wins if w for c in w], dtype=np.uint64))
    codes = allw[rng.random(len(allw)) < 0.9]
    for goff, gof in ((np.arange(5, dtype=np.uint64), [0, 1, 2, 3]), (np.array([0, 2, 4], dtype=np.uint64), [0, 0, 1, 1])):
        for allow in (False, True):
            for min_len in (1, 15, 40):
                want = model_map(wins, gof, codes.tolist(), k, allow, min_len)
                for route in (0, 1):
                    ctx.set_option("map_sorted", route)
                    try:
                        got = _rows(*ctx.map(bases, off, goff, k, codes, allow_multi=allow, min_len=min_len))
                    finally:
                        ctx.set_option("map_sorted", None)
                    assert got == want, (gof, allow, min_len, route)


# ---- fixture genomes at full size ------------------------------------------------------------------------------------------
def test_map_ecoli_inter_on_iai39(env, genomes):
    """README quick start: the k = 23 intersection of the two E. coli genomes (2,576,170 codes) mapped on Ecoli-IAI39"""
    lib, ctx, O = env
    k = 23
    sets = []
    for name in (IAI39, MG1655):
        b, o = genomes(name)
        sets.append(np.unique(O.count_windows(b, o, k)))
    codes = np.intersect1d(sets[0], sets[1])
    assert len(codes) == 2_576_170
    bases, off = genomes(IAI39)
    assert len(off) == 2
    wins = windows(O, bases, off, k)
    goff = np.array([0, 1], dtype=np.uint64)
    cl = codes.tolist()
    expect = {(200, False): 2741, (200, True): 2926, (1000, False): 43, (1000, True): 58}
    for (min_len, allow), count in expect.items():
        want = model_map(wins, [0], cl, k, allow, min_len)
        got = _rows(*ctx.map(bases, off, goff, k, codes, allow_multi=allow, min_len=min_len))
        print("map IAI39 -m %d%s: %d regions (model %d)" % (min_len, " -M" if allow else "", len(got), len(want)))
        assert got == want
        assert len(got) == count
        if (min_len, allow) == (200, False):
            assert [(s, e) for _, s, e in got[:3]] == [(0, 308), (300, 556), (868, 1302)]


# ---- through the binary ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    from unikmer_amd import build
    build.build()

    def run(*args):
        p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout.decode()
    return run


def test_cli_locate_readme_lines(cli, tmp_path):
    """reference README.md:174,189-194"""
    g = os.path.join(GOLDEN, AMUC)
    cli("count", "-k", 23, "-W", 5, "-H", "-K", "-l", g, "-o", tmp_path / "m")
    lines = cli("locate", "-g", g, str(tmp_path / "m") + ".unik").splitlines()[:5]
    assert lines == ["NC_010655.1\t2\t25\tATCTTATAAAATAACCACATAAC\t0\t.",
                     "NC_010655.1\t5\t28\tTTATAAAATAACCACATAACTTA\t0\t.",
                     "NC_010655.1\t6\t29\tTATAAAATAACCACATAACTTAA\t0\t.",
                     "NC_010655.1\t9\t32\tAAAATAACCACATAACTTAAAAA\t0\t.",
                     "NC_010655.1\t13\t36\tTAACCACATAACTTAAAAAGAAT\t0\t."]


def test_cli_map_ecoli(cli, tmp_path, genomes):
    a, b, i = (str(tmp_path / n) for n in ("a", "b", "i"))
    g = os.path.join(GOLDEN, IAI39)
    cli("count", "-k", 23, "-K", "-s", g, "-o", a)
    cli("count", "-k", 23, "-K", "-s", os.path.join(GOLDEN, MG1655), "-o", b)
    cli("inter", a + ".unik", b + ".unik", "-o", i)
    bed = cli("map", "-g", g, i + ".unik").splitlines()
    assert len(bed) == 2741
    name = bed[0].split("\t")[0]
    assert bed[:3] == ["%s\t0\t308" % name, "%s\t300\t556" % name, "%s\t868\t1302" % name]
    assert cli("uniqs", "-g", g, "-W", i + ".unik").splitlines() == bed          # one record: -W changes nothing
    assert len(cli("map", "-g", g, "-M", "-m", 1000, i + ".unik").splitlines()) == 58
    fa = cli("map", "-g", g, "-m", 1000, "-a", i + ".unik").splitlines()
    heads = [ln for ln in fa if ln.startswith(">")]
    assert len(heads) == 43
    bases, off = genomes(IAI39)
    first = cli("map", "-g", g, "-m", 1000, i + ".unik").splitlines()[0].split("\t")
    s, e = int(first[1]), int(first[2])
    assert heads[0] == ">%s:%d-%d" % (name, s + 1, e)
    seq = "".join(fa[1:fa.index(heads[1])])
    assert seq == bases[s:e].tobytes().decode() and all(len(ln) <= 60 for ln in fa if not ln.startswith(">"))
