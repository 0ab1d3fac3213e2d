"""ukm_view / ukm_dump against tests/text_model.py (pinned to the host loops of `view` and `dump` by tests/test_text_cpu.py):
view equals the model byte for byte, dump gives the model's records or the model's first bad line, from host arrays and from
device tensors."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "unikmer_amd", "csrc", "ukm_text.hip")).read()


def _const(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, _SRC).group(1))


FIXV_RECS = _const("FIXV_RECS")   # lines per tile of the fixed-width view
VIEW_RECS = _const("VIEW_RECS")   # records per tile of every other view
TILE = _const("DUMP_TILE")        # text bytes per tile of dump
LINE = _const("DUMP_LINE")        # the longest legal line of dump, its LF included
assert LINE == M.MAX_LINE
TOP, TOP32 = (1 << 64) - 1, (1 << 32) - 1
PAT = 0xA5


@pytest.fixture(scope="module")
def lib():
    from unikmer_amd import lib as L
    return L


@pytest.fixture(scope="module")
def ctx(lib):
    c = lib.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}[a.dtype]
    return torch.from_numpy(a.view(signed).copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype) if hasattr(t, "cpu") else np.asarray(t, dtype=dtype)


def u64(v):
    return np.array([int(x) for x in v], dtype=np.uint64)


def u32(v):
    return None if v is None else np.array([int(x) for x in v], dtype=np.uint32)


def check_view(ctx, codes, tax, ft, k, hashed, fmt, where=("host", "device")):
    want = M.render(codes, tax, ft, k, hashed, fmt)
    kk, tt = u64(codes), u32(tax)
    for w in where:
        a, b = (kk, tt) if w == "host" else (dev(kk), dev(tt))
        got = ctx.view(a, b, ft, k=k, hashed=hashed, fmt=fmt)
        assert host(got, np.uint8).tobytes() == want, (w, k, hashed, fmt, len(codes))
    return want


def records(n, k, seed):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 1 << 63, n, dtype=np.uint64) >> rng.integers(0, 63, n).astype(np.uint64)   # every number of digits
    tax = (rng.integers(0, 1 << 32, n, dtype=np.uint64) >> rng.integers(0, 32, n).astype(np.uint64)).astype(np.uint32)
    return codes, tax


# ---- view ---------------------------------------------------------------------------------------------------------------------
SIZES = lambda t: (0, 1, t - 1, t, t + 1, 2 * t + 1)   # noqa: E731


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("hashed", [False, True])
def test_view_sizes_around_the_tile(ctx, fmt, hashed):
    t = FIXV_RECS if fmt == M.KMER and not hashed else VIEW_RECS
    codes, tax = records(2 * t + 1, 31, 3)
    for n in SIZES(t):
        check_view(ctx, codes[:n], tax[:n], 0, 31, hashed, fmt, where=("device",) if n > 1 else ("host", "device"))


@pytest.mark.parametrize("fmt,hashed,k", [(M.KMER, False, 3), (M.KMER_TAXID, False, 3), (M.FASTA, False, 3),
                                          (M.FASTQ | M.WITH_TAXID, True, 64)])
def test_view_more_tiles_than_one_scan_round(ctx, fmt, hashed, k):
    """257 tiles + 3: the one-workgroup scan of the tile sizes loops (a small k: the model spells every letter in Python)"""
    t = FIXV_RECS if fmt == M.KMER and not hashed else VIEW_RECS
    codes, tax = records(257 * t + 3, k, 4)
    check_view(ctx, codes, tax, 0, k, hashed, fmt, where=("device",))


EDGE_CODES = [0] + [v for e in range(1, 20) for v in (10 ** e - 1, 10 ** e)] + [TOP]
EDGE_TAX = [0, 9, 10, TOP32]


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_view_every_number_of_digits(ctx, fmt):
    codes = EDGE_CODES * 4                                     # (the top codes have bits above 2k set for every k <= 31)
    tax = [EDGE_TAX[(i // len(EDGE_CODES) + i) % 4] for i in range(len(codes))]
    for k in (1, 31, 32):
        check_view(ctx, codes, tax, 0, k, False, fmt)
    for k in (1, 64):
        check_view(ctx, codes, tax, 0, k, True, fmt)
    for ft in EDGE_TAX:                                        # taxids == NULL: the file's one taxid
        check_view(ctx, codes, None, ft, 31, False, fmt, where=("device",))
        check_view(ctx, codes, None, ft, 64, True, fmt, where=("device",))


@pytest.mark.parametrize("fmt,hashed", [(M.KMER, False), (M.KMER_TAXID, False), (M.FASTQ | M.WITH_TAXID, True)])
def test_view_writes_its_bytes_and_no_other(ctx, lib, fmt, hashed):
    """the output at every offset 0..15 of a slab: what lies in front of and behind [0, n_out) survives; out_cap one short:
    UKM_ERR_CAPACITY with the exact size and nothing written; out_cap 0 with NULL: the size"""
    import torch
    t = FIXV_RECS if fmt == M.KMER and not hashed else VIEW_RECS
    codes, tax = records(t + 7, 23, 5)
    want = M.render(codes, tax, 0, 23, hashed, fmt)
    dk, dt = dev(codes), dev(tax)
    n = C.c_uint64()
    rc = ctx.L.ukm_view(ctx.h, dk.data_ptr(), dt.data_ptr(), 0, len(codes), 23, int(hashed), fmt, None, 0, C.byref(n))
    assert rc == lib.ERR_CAPACITY and n.value == len(want)
    for off in range(16):
        slab = torch.full((len(want) + 256,), PAT, dtype=torch.uint8, device="cuda")
        got = ctx.view(dk, dt, 0, k=23, hashed=hashed, fmt=fmt, out=slab[64 + off: 64 + off + len(want)])
        s = slab.cpu().numpy()
        assert got.cpu().numpy().tobytes() == want
        assert (s[: 64 + off] == PAT).all() and (s[64 + off + len(want):] == PAT).all(), off
    slab = torch.full((len(want) + 256,), PAT, dtype=torch.uint8, device="cuda")
    with pytest.raises(lib.CapacityError) as e:
        ctx.view(dk, dt, 0, k=23, hashed=hashed, fmt=fmt, out=slab[67: 67 + len(want) - 1])
    assert e.value.needed == len(want) and (slab.cpu().numpy() == PAT).all()
    # host pointers in and out, the output in the middle of a host slab
    hs = np.full(len(want) + 64, PAT, dtype=np.uint8)
    got = ctx.view(codes, tax, 0, k=23, hashed=hashed, fmt=fmt, out=hs[5: 5 + len(want)])
    assert got.tobytes() == want and (hs[:5] == PAT).all() and (hs[5 + len(want):] == PAT).all()


def test_calls_do_not_depend_on_what_the_workspace_held(ctx):
    codes, tax = records(3 * VIEW_RECS + 5, 31, 6)
    text = M.render(codes, tax, 0, 31, False, M.KMER_TAXID)
    tb = np.frombuffer(text, dtype=np.uint8)
    for byte in (0x00, 0xFF):
        ctx.set_option("ws_poison", byte)
        try:
            for fmt in (M.KMER, M.KMER_TAXID, M.FASTA | M.WITH_TAXID):
                assert ctx.view(codes, tax, 0, k=31, fmt=fmt).tobytes() == M.render(codes, tax, 0, 31, False, fmt)
            keys, tx = ctx.dump(tb, k=31, flags=M.D_TAXID)
            want = M.parse(text, 31, M.D_TAXID)
            assert keys.tolist() == want.codes and tx.tolist() == want.taxids
        finally:
            ctx.set_option("ws_poison", None)


# ---- dump ---------------------------------------------------------------------------------------------------------------------
def check_dump(ctx, lib, text, k, flags, where=("host", "device")):
    """the model's records, or the model's first bad line"""
    want = M.parse(text, k, flags)
    b = np.frombuffer(text, dtype=np.uint8)
    for w in where:
        arr = b if w == "host" else dev(b)
        if want.bad_off is not None:
            with pytest.raises(lib.FormatError) as e:
                ctx.dump(arr, k=k, flags=flags)
            assert e.value.bad_off == want.bad_off, (w, text[:80])
            continue
        keys, tax = ctx.dump(arr, k=k, flags=flags)
        assert host(keys, np.uint64).tolist() == want.codes, (w, text[:80])
        assert (tax is None) == (want.taxids is None)
        if tax is not None:
            assert host(tax, np.uint32).tolist() == want.taxids
    return want


def good_lines(n, k, flags, seed, eol=b"\n"):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if flags & M.D_DECIMAL:
            f1 = b"%d" % (int(rng.integers(0, 1 << 63)) >> int(rng.integers(0, 63)))
        else:
            f1 = bytes(rng.choice(np.frombuffer(b"ACGTacgtNnMVHRDWSBYKUu", dtype=np.uint8), k))
        f2 = b"\t%d" % (int(rng.integers(0, 1 << 32)) >> int(rng.integers(0, 32))) if flags & M.D_TAXID else b""
        out.append(f1 + f2 + eol)
    return out


def text_of_size(size, k, flags, seed):
    """legal text of exactly `size` bytes: lines (20,000 at the most), then empty lines"""
    out, n = [], 0
    for ln in good_lines(min(size // ((1 if flags & M.D_DECIMAL else k) + 1) + 1, 20000), k, flags, seed):
        if n + len(ln) > size:
            break
        out.append(ln)
        n += len(ln)
    return b"".join(out) + b"\n" * (size - n)


@pytest.mark.parametrize("flags", [0, M.D_TAXID])
def test_dump_line_endings(ctx, lib, flags):
    two = b"\t12" if flags else b""
    for text in (b"ACGTA" + two + b"\nCCGTA" + two + b"\n", b"ACGTA" + two + b"\r\nCCGTA" + two + b"\r\n", b"ACGTA" + two + b"\nCCGTA" + two,
                 b"ACGTA" + two + b"\r\nCCGTA" + two + b"\r", b"", b"\n", b"\n\n\r\n\n", b"\n\nACGTA" + two + b"\n\n"):
        want = check_dump(ctx, lib, text, 5, flags)
        assert want.bad_off is None and len(want.codes) == text.count(b"GTA")


LONGEST = b"A" * 32 + b"\t4294967295\r\n"


def test_dump_lines_at_every_offset_around_a_tile_boundary(ctx, lib):
    """a line of the longest legal length starts d bytes behind (in front of) the boundary, d = -LINE - 1 .. LINE: its LF
    is the last byte of a tile, the first of the next, and everywhere between; so for the shortest line"""
    assert len(LONGEST) == LINE
    for d in range(-LINE - 1, LINE + 1):
        for ln in (LONGEST, b"C" * 32 + b"\t7\n"):
            head = text_of_size(TILE + d, 32, M.D_TAXID, 7)
            text = head + ln + b"G" * 32 + b"\t1\n"
            want = check_dump(ctx, lib, text, 32, M.D_TAXID, where=("device",))
            assert want.bad_off is None and want.taxids[-2:] == [TOP32 if ln is LONGEST else 7, 1]
    for d in range(-3, 3):        # k = 1: two-byte lines, four records to a thread
        text = text_of_size(TILE + d, 1, 0, 8) + b"A\nC\nG\nT\nA"
        check_dump(ctx, lib, text, 1, 0, where=("device",))


@pytest.mark.parametrize("size", [TILE - 1, TILE, TILE + 1, 257 * TILE + 3])
def test_dump_sizes_around_the_tile(ctx, lib, size):
    for flags, k in ((M.D_TAXID, 31), (0, 3), (M.D_DECIMAL | M.D_TAXID, 0)):
        text = text_of_size(size, k, flags, 9)
        check_dump(ctx, lib, text, k, flags, where=("device",))
        check_dump(ctx, lib, text[:-1] + b"A" if not flags & M.D_DECIMAL else text[:-1] + b"7", k, flags, where=("device",))   # (no final LF; mostly a bad line)


@pytest.mark.parametrize("flags", [0, M.D_TAXID, M.D_DECIMAL, M.D_DECIMAL | M.D_TAXID, M.D_CANONICAL, M.D_CANONICAL | M.D_TAXID,
                                   M.D_CANONICAL_ONLY, M.D_CANONICAL_ONLY | M.D_TAXID, M.D_CANONICAL | M.D_CANONICAL_ONLY])
def test_dump_flags(ctx, lib, flags):
    for k in (1, 2, 21, 32):
        text = b"".join(good_lines(700, k, flags, 10 + k, eol=b"\r\n" if k == 21 else b"\n"))
        want = check_dump(ctx, lib, text, k, flags)
        assert want.bad_off is None
        if flags & M.D_TAXID:          # out_taxids == NULL: the second column is checked, not stored
            b = np.frombuffer(text, dtype=np.uint8)
            out = np.zeros(len(want.codes) + 1, dtype=np.uint64)
            n = C.c_uint64()
            assert ctx.L.ukm_dump(ctx.h, b.ctypes.data, len(b), k, flags, out.ctypes.data, None, len(out), C.byref(n), None) == lib.OK
            assert out[: n.value].tolist() == want.codes
            bad = text + b"A" * k + b"\t\n" if not flags & M.D_DECIMAL else text + b"5\t\n"
            b = np.frombuffer(bad, dtype=np.uint8)
            off = C.c_uint64()
            assert ctx.L.ukm_dump(ctx.h, b.ctypes.data, len(b), k, flags, out.ctypes.data, None, len(out), C.byref(n), C.byref(off)) == lib.ERR_FORMAT
            assert off.value == len(text)


# one line per reason: (the line, k, flags)
BAD = {
    "too short": (b"ACGT", 5, 0), "too long": (b"ACGTAC", 5, 0), "illegal byte": (b"ACXTA", 5, 0), "space": (b"ACGTA 5", 5, M.D_TAXID),
    "blank behind": (b"ACGTA ", 5, 0), "TAB without the flag": (b"ACGTA\t5", 5, 0), "no TAB with the flag": (b"ACGTA", 5, M.D_TAXID),
    "second TAB": (b"ACGTA\t5\t6", 5, M.D_TAXID), "sign": (b"-5", 0, M.D_DECIMAL), "21 digits": (b"1" * 21, 0, M.D_DECIMAL),
    "2^64": (b"18446744073709551616", 0, M.D_DECIMAL), "taxid 2^32": (b"ACGTA\t4294967296", 5, M.D_TAXID),
    "taxid of 11 digits": (b"ACGTA\t00000000001", 5, M.D_TAXID), "empty field2": (b"ACGTA\t", 5, M.D_TAXID),
    "letter in field2": (b"ACGTA\t5x", 5, M.D_TAXID), "two CR": (b"ACGTA\r", 5, 0), "a line without end": (b"A" * 100, 5, 0),
}


@pytest.mark.parametrize("why", list(BAD))
def test_dump_bad_lines(ctx, lib, why):
    ln, k, flags = BAD[why]
    body = good_lines(3 * TILE // 4, k, flags, 11)

    def with_bad_at(*targets):
        """the good lines, a bad line put in front of the first good line that starts at or behind each target offset"""
        out, n, todo = [], 0, sorted(targets)
        for g in body:
            if todo and n >= todo[0]:
                out.append(ln + b"\r\n")
                n += len(ln) + 2
                todo.pop(0)
            out.append(g)
            n += len(g)
        assert not todo
        return b"".join(out)
    total = sum(len(g) for g in body)
    assert total > 3 * TILE
    boundary = TILE - len(ln) // 2 - 1          # the bad line starts in front of the boundary and ends behind it
    for target in (0, 1, boundary, 2 * TILE + 7, total - len(body[-1])):
        want = check_dump(ctx, lib, with_bad_at(target), k, flags, where=("device",))
        assert want.bad_off is not None and want.bad_off >= target
    # the bad line as the last of the text, without LF; and alone
    check_dump(ctx, lib, b"".join(body) + ln, k, flags, where=("device",))
    assert check_dump(ctx, lib, ln + b"\r\n", k, flags).bad_off == 0
    # two bad lines: the lower offset, whichever tile sees it first
    want = check_dump(ctx, lib, with_bad_at(TILE + 100, 2 * TILE + 100), k, flags)
    assert TILE + 100 <= want.bad_off < TILE + 200


def test_dump_format_error_wins_over_capacity(ctx, lib):
    text = np.frombuffer(b"ACGTA\nACG\n", dtype=np.uint8)
    n, off = C.c_uint64(), C.c_uint64()
    assert ctx.L.ukm_dump(ctx.h, text.ctypes.data, len(text), 5, 0, None, None, 0, C.byref(n), C.byref(off)) == lib.ERR_FORMAT
    assert off.value == 6
    assert ctx.L.ukm_dump(ctx.h, text.ctypes.data, 6, 5, 0, None, None, 0, C.byref(n), C.byref(off)) == lib.ERR_CAPACITY and n.value == 1


@pytest.mark.parametrize("flags,k,text", [
    (M.D_TAXID, 4, b"ACGT\t5\r\n\nTTGA\t4294967295\nNNNN\t0\r\n\r\nacgu\t12\n"),
    (0, 3, b"ACG\nTTT\r\n\n\nGGA\r\nCCC"),
    (M.D_DECIMAL | M.D_TAXID, 0, b"18446744073709551615\t1\n0\t4294967295\r\n77\t3\n"),
    (M.D_CANONICAL_ONLY, 2, b"AA\nTT\nCG\nGT\nAC\n"),
])
def test_dump_every_prefix_like_the_model(ctx, lib, flags, k, text):
    for cut in range(len(text)):
        check_dump(ctx, lib, text[:cut], k, flags, where=("host",) if cut % 2 else ("device",))


# ---- both ---------------------------------------------------------------------------------------------------------------------
def test_round_trips(ctx, lib):
    import torch
    rng = np.random.default_rng(12)
    n = 5 * VIEW_RECS + 11
    codes = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    tax = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    dk, dt = dev(codes), dev(tax)
    text = ctx.view(dk, dt, k=31, fmt=lib.VIEW_KMER_TAXID)
    keys, tx = ctx.dump(text, k=31, flags=lib.DUMP_TAXID)
    assert np.array_equal(host(keys, np.uint64), codes) and np.array_equal(host(tx, np.uint32), tax)
    keys, tx = ctx.dump(ctx.view(dk, k=31), k=31)
    assert np.array_equal(host(keys, np.uint64), codes) and tx is None
    hashed = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    hk = dev(hashed)
    htext = ctx.view(hk, dt, k=64, hashed=True, fmt=lib.VIEW_KMER_TAXID)
    keys, tx = ctx.dump(htext, k=64, flags=lib.DUMP_TAXID | lib.DUMP_DECIMAL)
    assert np.array_equal(host(keys, np.uint64), hashed) and np.array_equal(host(tx, np.uint32), tax)
    # the text read from every offset 1..15 of a slab, other bytes around it
    for off in range(1, 16):
        slab = torch.full((len(text) + 64,), ord("A"), dtype=torch.uint8, device="cuda")
        slab[off: off + len(text)] = text
        keys, tx = ctx.dump(slab[off: off + len(text)], k=31, flags=lib.DUMP_TAXID)
        assert np.array_equal(host(keys, np.uint64), codes) and np.array_equal(host(tx, np.uint32), tax)


def test_argument_errors(ctx, lib):
    keys = np.arange(4, dtype=np.uint64)
    text = np.frombuffer(b"ACGT\n", dtype=np.uint8)

    def code(fn, *a, **kw):
        with pytest.raises(lib.UkmError) as e:
            fn(*a, **kw)
        return e.value.code
    for k, hashed in ((0, False), (33, False), (-1, False), (0, True), (65, True)):
        assert code(ctx.view, keys, k=k, hashed=hashed) == lib.ERR_K
    ctx.view(keys, k=64, hashed=True)
    for fmt in (7, 15, 32, 5 | 32, lib.VIEW_KMER | lib.VIEW_WITH_TAXID, lib.VIEW_KMER_TAXID | lib.VIEW_WITH_TAXID, lib.VIEW_CODE | lib.VIEW_WITH_TAXID):
        assert code(ctx.view, keys, k=5, fmt=fmt) == lib.ERR_INVALID
    for k in (0, 33, -1):
        assert code(ctx.dump, text, k=k) == lib.ERR_K
        assert code(ctx.dump, text[:0], k=k) == lib.ERR_K
    assert code(ctx.dump, text, k=4, flags=16) == lib.ERR_INVALID
    for f in (lib.DUMP_CANONICAL, lib.DUMP_CANONICAL_ONLY):
        assert code(ctx.dump, np.frombuffer(b"5\n", dtype=np.uint8), k=4, flags=lib.DUMP_DECIMAL | f) == lib.ERR_INVALID
    keys, tx = ctx.dump(np.frombuffer(b"5\n", dtype=np.uint8), k=0, flags=lib.DUMP_DECIMAL)        # k is ignored
    assert keys.tolist() == [5]
    n = C.c_uint64(7)
    assert ctx.L.ukm_view(ctx.h, None, None, 0, 0, 5, 0, 0, None, 0, C.byref(n)) == lib.OK and n.value == 0
    n = C.c_uint64(7)
    assert ctx.L.ukm_dump(ctx.h, None, 0, 5, 0, None, None, 0, C.byref(n), None) == lib.OK and n.value == 0
