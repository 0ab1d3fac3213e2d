"""ukm_pair_counts on the GPU: all-pairs shared distinct-code counts against numpy (np.intersect1d sizes of np.unique'd
streams), exact in every case.  Shapes are the smallest at which the kernel can go wrong: the edges of the 64-stream tile
(63, 64, 65), a three-tile triangle with its mirror (130), column totals around a 32-bit word and around the K tile of
64 words, several column blocks through option "pair_block_cols"."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KT_COLS = 2048          # columns of a K tile: 64 words x 32 bits (unikmer_amd/csrc/ukm_pairs.h)
U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def L():
    from unikmer_amd import lib
    return lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def expected(streams, rows=None):
    """(counts, sizes) by numpy: intersect1d sizes of the unique'd streams"""
    u = [np.unique(np.asarray(s, dtype=np.uint64)) for s in streams]
    n = len(u)
    rows = n if rows is None else rows
    c = np.zeros((rows, n), dtype=np.uint64)
    for i in range(rows):
        for j in range(n):
            c[i, j] = len(u[i]) if i == j else c[j, i] if j < i else len(np.intersect1d(u[i], u[j], assume_unique=True))
    return c, np.array([len(x) for x in u], dtype=np.uint64)


def make_streams(n, seed, pool_size=400, most=300):
    """n streams of 0 .. `most` codes drawn WITH replacement (duplicates inside a stream, no order) from a pool of about
    pool_size codes that holds 0 and 2^64 - 1; every third stream sorted; stream 0 holds both extreme codes; with 5 or more
    streams: stream 1 empty, 2 == 3, 4 nested in 0"""
    rng = np.random.default_rng(seed)
    pool = np.unique(np.concatenate([rng.integers(0, 1 << 63, pool_size - 2, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                                     np.array([0, U64MAX], dtype=np.uint64)]))
    out = []
    for i in range(n):
        s = pool[rng.integers(0, len(pool), int(rng.integers(0, most + 1)))]
        out.append(np.sort(s) if i % 3 == 2 else s)
    out[0] = np.concatenate([out[0], np.array([U64MAX, 0, U64MAX], dtype=np.uint64)])
    if n >= 5:
        out[1] = np.empty(0, dtype=np.uint64)
        out[3] = out[2][::-1].copy()
        out[4] = out[0][: len(out[0]) // 2].copy()
    return out


@pytest.fixture(scope="module")
def s130():
    """130 streams and numpy's answer, computed once and left unchanged"""
    streams = make_streams(130, 130)
    c, s = expected(streams)
    c.setflags(write=False)
    s.setflags(write=False)
    return streams, c, s


def check(ctx, streams, rows=None, want=None):
    c, s = ctx.pair_counts(streams, rows=rows)
    wc, ws = want if want is not None else expected(streams, rows)
    assert c.dtype == np.uint64 and c.shape == wc.shape and s.shape == ws.shape
    assert np.array_equal(s, ws), np.flatnonzero(s != ws)[:8]
    assert np.array_equal(c, wc), np.argwhere(c != wc)[:8]
    return c, s


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 130])
def test_stream_counts(ctx, n, s130):
    if n == 130:
        streams, wc, ws = s130
        c, _ = check(ctx, streams, want=(wc, ws))
        assert np.array_equal(c, c.T)
        assert (c > 0).mean() > 0.5            # most pairs share something: the pool is small
    else:
        check(ctx, make_streams(n, n))
    assert ctx.stat("pair_blocks") == 1


def test_fixed_sets(ctx):
    a = np.array([5, 9, 1, 0, U64MAX, 9, 9, 7], dtype=np.uint64)       # unsorted, duplicates, both extreme codes
    streams = [a, np.empty(0, dtype=np.uint64), a[::-1].copy(),          # empty; identical to a as a set
               np.array([2, 4, 6, 8], dtype=np.uint64),                  # disjoint from a
               np.array([U64MAX, 0, 7], dtype=np.uint64),                # nested in a
               np.empty(0, dtype=np.uint64)]
    c, s = check(ctx, streams)
    assert s.tolist() == [6, 0, 6, 4, 3, 0]
    assert c[0].tolist() == [6, 0, 6, 0, 3, 0] and not c[1].any() and not c[:, 1].any() and c[3, 4] == 0 and c[5, 5] == 0
    assert ctx.stat("pair_columns") == 10
    # nothing but empty streams
    c, s = check(ctx, [np.empty(0, dtype=np.uint64)] * 3)
    assert not c.any() and not s.any() and ctx.stat("pair_columns") == 0 and ctx.stat("pair_blocks") == 0


@pytest.mark.parametrize("total", [31, 32, 33, KT_COLS - 32, KT_COLS - 1, KT_COLS, KT_COLS + 1, KT_COLS + 32])
def test_column_edges(ctx, total):
    rng = np.random.default_rng(total)
    pool = np.unique(rng.integers(0, 1 << 63, 2 * total, dtype=np.uint64))[:total]
    pool[0], pool[-1] = 0, U64MAX
    assert len(np.unique(pool)) == total
    streams = [rng.permutation(pool), pool[rng.random(total) < 0.5], pool[-40:], pool[:1], pool[total - 33:total - 31]]
    check(ctx, streams)
    assert ctx.stat("pair_columns") == total


def block_streams(n, seed, draws):
    """n streams over a pool of 5 K tiles' worth of distinct codes; stream 1 is the whole pool, backwards"""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, 1 << 64, 5 * KT_COLS, dtype=np.uint64))
    streams = [pool[rng.integers(0, len(pool), draws)] for _ in range(n)]
    streams[1] = pool[::-1].copy()                                     # a bit in every column of every block
    return pool, streams


@pytest.mark.parametrize("n", [6, 65])
def test_multi_block_accumulation(ctx, n):
    """columns walked in blocks of ONE K tile: the counts accumulate over the blocks.  The statistics prove that several
    blocks ran: a test that silently ran one block would hide the accumulation path."""
    pool, streams = block_streams(n, n, 300 if n > 6 else 4000)
    want = expected(streams)
    ctx.set_option("pair_block_cols", KT_COLS)
    try:
        c1, s1 = check(ctx, streams, want=want)
        assert ctx.stat("pair_blocks") >= 3
        assert ctx.stat("pair_blocks") == -(-len(pool) // KT_COLS)
        assert ctx.stat("pair_columns") == len(np.unique(np.concatenate(streams))) == len(pool)
        ctx.set_option("pair_block_cols", 2 * KT_COLS + 1)             # rounded up to 3 K tiles
        check(ctx, streams, want=want)
        assert ctx.stat("pair_blocks") == -(-len(pool) // (3 * KT_COLS))
    finally:
        ctx.set_option("pair_block_cols", None)
    c0, s0 = check(ctx, streams, want=want)
    assert ctx.stat("pair_blocks") == 1
    assert c0.tobytes() == c1.tobytes() and s0.tobytes() == s1.tobytes()


@pytest.mark.parametrize("rows", [1, 63, 65])
def test_rectangular(ctx, rows, s130):
    streams, wc, ws = s130
    c, s = check(ctx, streams, rows=rows, want=(wc[:rows], ws))
    assert c.shape == (rows, 130) and len(s) == 130


def _packed_unaligned(torch, streams):
    """the streams one behind another in ONE device allocation, the first at 8 mod 16 bytes"""
    total = sum(len(s) for s in streams)
    buf = torch.zeros(total + 3, dtype=torch.int64, device="cuda")
    base = 1 if buf.data_ptr() % 16 == 0 else 0
    out, off = [], base
    for s in streams:
        v = buf[off:off + len(s)]
        v.copy_(torch.from_numpy(s.view(np.int64).copy()))
        out.append(v)
        off += len(s)
    assert out[0].data_ptr() % 16 == 8 and len({v.data_ptr() % 16 for v in out if v.numel()}) == 2
    return buf, out


def test_buffer_placement(ctx, s130):
    import torch
    streams, wc, ws = s130
    streams, wc, ws = streams[:70], wc[:70, :70], ws[:70]
    dev = [torch.from_numpy(s.view(np.int64).copy()).cuda() for s in streams]
    mixed = [d if i % 2 else s for i, (s, d) in enumerate(zip(streams, dev))]
    torch.cuda.synchronize()
    for inputs in (streams, dev, mixed):
        check(ctx, inputs, want=(wc, ws))
    buf, packed = _packed_unaligned(torch, streams)
    torch.cuda.synchronize()
    check(ctx, packed, want=(wc, ws))
    # both outputs on the device, and rows < n with device outputs
    for rows in (70, 3):
        out = torch.full((rows * 70,), -1, dtype=torch.int64, device="cuda")
        sz = torch.full((70,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        c, s = ctx.pair_counts(dev, rows=rows, out=out, sizes=sz)
        assert c is out and s is sz
        assert np.array_equal(out.cpu().numpy().view(np.uint64).reshape(rows, 70), wc[:rows])
        assert np.array_equal(sz.cpu().numpy().view(np.uint64), ws)
    # sizes=False: no size array at all
    c, s = ctx.pair_counts(dev, sizes=False)
    assert s is None and np.array_equal(c, wc)


@pytest.mark.parametrize("rows", [65, 2])
def test_canaries(ctx, rows, s130):
    """guard words around both outputs stay intact, on the device and on the host"""
    import torch
    streams, wc, ws = s130
    streams, wc, ws = streams[:65], wc[:rows, :65], ws[:65]
    G, MARK = 8, 0x5A5A5A5A5A5A5A5A
    out = torch.full((rows * 65 + 2 * G,), MARK, dtype=torch.int64, device="cuda")
    sz = torch.full((65 + 2 * G,), MARK, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.pair_counts(streams, rows=rows, out=out[G:-G], sizes=sz[G:-G])
    o, z = out.cpu().numpy(), sz.cpu().numpy()
    assert (o[:G] == MARK).all() and (o[-G:] == MARK).all() and (z[:G] == MARK).all() and (z[-G:] == MARK).all()
    assert np.array_equal(o[G:-G].view(np.uint64).reshape(rows, 65), wc) and np.array_equal(z[G:-G].view(np.uint64), ws)
    ho = np.full(rows * 65 + 2 * G, MARK, dtype=np.uint64)
    hz = np.full(65 + 2 * G, MARK, dtype=np.uint64)
    ctx.pair_counts(streams, rows=rows, out=ho[G:-G], sizes=hz[G:-G])
    assert (ho[:G] == MARK).all() and (ho[-G:] == MARK).all() and (hz[:G] == MARK).all() and (hz[-G:] == MARK).all()
    assert np.array_equal(ho[G:-G].reshape(rows, 65), wc) and np.array_equal(hz[G:-G], ws)


def test_independence_of_earlier_calls_and_workspace(ctx, s130):
    streams, wc, ws = s130
    c0, s0 = check(ctx, streams, want=(wc, ws))
    c1, s1 = check(ctx, streams, want=(wc, ws))
    assert c0.tobytes() == c1.tobytes() and s0.tobytes() == s1.tobytes()
    try:
        for fill in (0xFF, 0x5A):
            ctx.set_option("ws_poison", fill)
            for rows in (None, 63):
                c, s = check(ctx, streams, rows=rows, want=(wc[:rows], ws))
                assert ctx.stat("ws_poisoned_bytes") > 0
                assert c.tobytes() == c0[:rows].tobytes() and s.tobytes() == s0.tobytes()
            ctx.set_option("pair_block_cols", KT_COLS)
            check(ctx, block_streams(4, 77, 2000)[1])
            assert ctx.stat("pair_blocks") >= 3
            ctx.set_option("pair_block_cols", None)
    finally:
        ctx.set_option("ws_poison", None)
        ctx.set_option("pair_block_cols", None)


def test_agrees_with_the_rest_of_the_library(ctx, s130):
    streams, wc, ws = s130
    c, s = ctx.pair_counts(streams)
    u = [np.unique(x) for x in streams]
    for i, j in ((0, 4), (2, 3), (7, 8), (64, 129), (63, 64), (100, 5)):
        if len(u[i]) and len(u[j]):
            assert c[i, j] == len(ctx.inter([u[i], u[j]])), (i, j)
    assert all(int(s[i]) == len(u[i]) for i in range(130))
    same = [streams[0]] * 66
    c, s = ctx.pair_counts(same)
    assert (c == len(u[0])).all() and (s == len(u[0])).all()
    assert ctx.last_kernel_ms() >= 0 and ctx.last_call_ms() >= ctx.last_kernel_ms()
    assert ctx.stat("pair_kernel_us") == pytest.approx(ctx.last_kernel_ms() * 1000, abs=2)


def test_errors(ctx, L):
    a = [np.arange(4, dtype=np.uint64), np.arange(2, 9, dtype=np.uint64)]
    for rows in (0, 3, -1):
        with pytest.raises(L.UkmError) as e:
            ctx.pair_counts(a, rows=rows)
        assert e.value.code == L.ERR_INVALID and "nrows" in str(e.value)
    lib = L.load()
    kp = (C.c_void_p * 2)(a[0].ctypes.data, a[1].ctypes.data)
    lens = (C.c_uint64 * 2)(4, 7)
    out = np.full(4, 99, dtype=np.uint64)
    args = (ctx.h, C.cast(kp, C.POINTER(C.c_void_p)), lens, 2, 2)
    assert lib.ukm_pair_counts(*args, 1, out.ctypes.data, None) == L.ERR_INVALID and b"flags" in lib.ukm_last_error()
    assert lib.ukm_pair_counts(ctx.h, None, None, 65537, 1, 0, None, None) == L.ERR_INVALID and b"nstreams" in lib.ukm_last_error()
    assert lib.ukm_pair_counts(ctx.h, None, None, 0, 0, 0, None, None) == L.ERR_INVALID
    assert lib.ukm_pair_counts(*args, 0, None, None) == L.ERR_INVALID
    assert (out == 99).all()
    assert lib.ukm_pair_counts(*args, 0, out.ctypes.data, None) == 0 and out.tolist() == [4, 2, 2, 7]   # NULL sizes is allowed


def test_command_line_module(ctx, tmp_path):
    from unikmer_amd import unikfile as U
    rng = np.random.default_rng(3)
    pool = np.unique(rng.integers(0, 1 << 42, 500, dtype=np.uint64))             # 21-mers
    sets = [np.sort(pool[rng.random(len(pool)) < p]) for p in (0.7, 0.4, 0.5)]
    hdr = {"k": 21, "flag": U.CANONICAL | U.SORTED}
    paths = []
    for name, keys in zip(("a.unik", "b.unik", "c.unik"), sets):
        paths.append(str(tmp_path / name))
        U.save(ctx, paths[-1], hdr, keys)
    other = str(tmp_path / "k23.unik")
    U.save(ctx, other, dict(hdr, k=23), sets[0])
    wc, ws = expected(sets)

    def run(*args):
        return subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-m", "unikmer_amd.similarity"] + list(args),
                              cwd=ROOT, capture_output=True, text=True)

    def parse(text):
        lines = [ln.split("\t") for ln in text.strip("\n").split("\n")]
        return lines[0][1:], [ln[0] for ln in lines[1:]], [ln[1:] for ln in lines[1:]]
    p = run(*paths)
    assert p.returncode == 0, p.stderr
    cols, rows, cells = parse(p.stdout)
    assert cols == rows == ["a.unik", "b.unik", "c.unik"]
    assert np.array_equal(np.array(cells, dtype=np.uint64), wc)
    p = run("--metric", "jaccard", "--rows", "2", *paths)
    assert p.returncode == 0, p.stderr
    cols, rows, cells = parse(p.stdout)
    assert cols == ["a.unik", "b.unik", "c.unik"] and rows == ["a.unik", "b.unik"]
    wj = wc[:2].astype(np.float64) / (ws[:2, None].astype(np.float64) + ws[None, :].astype(np.float64) - wc[:2].astype(np.float64))
    assert np.allclose(np.array(cells, dtype=np.float64), wj, rtol=1e-5, atol=0)   # printed with 6 significant digits
    p = run(paths[0], other)
    assert p.returncode != 0 and "k23.unik" in p.stderr and "a.unik" in p.stderr and p.stdout == ""
