"""ukm_deflate on the device, judged by zlib: a FINAL fragment must inflate (raw, window bits -15) to the input exactly, with
eof set and nothing left over; a fragment that is not final is followed by the next one or by the final empty block 03 00;
the returned CRC is zlib.crc32.  Every case from host arrays and from device tensors."""
import ctypes as C
import gzip
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_fixtures as F  # noqa: E402
import unik_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

CH = F.CH            # DFL_CHUNK
SCAN_WIDTH = 256     # NT of ukm_bytes.h: chunk sums the scan workgroup takes at a time
FINAL_BLOCK = b"\x03\x00"
# Bytes per chunk the device may take beyond zlib's Z_HUFFMAN_ONLY on the same chunks with a full flush behind each: the
# largest excess measured on the three fixtures (the Fibonacci chunk, the sorted body, the sorted body with taxids: printed by
# test_size_against_the_reference_coder, recorded in profiles/deflate.json and DESIGN.md 4.19) rounded up to a whole byte,
# plus one byte for tie-breaking differences
EXCESS_PER_CHUNK = 0 + 1


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
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8).copy()).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t, dtype=np.uint8)


def inflate_final(frag):
    d = zlib.decompressobj(-15)
    out = d.decompress(bytes(frag))
    assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b""
    return out


def nchunks(n):
    return (n + CH - 1) // CH


def check(ctx, data, crc=0):
    """every form of one input, host and device; returns the plain fragment's bytes"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    raw = data.tobytes()
    want_crc = zlib.crc32(raw, crc)
    frags = []
    for arr in (data, dev(data)):
        frag, c = ctx.deflate(arr, crc=crc)
        assert type(frag) is type(arr)
        f = host(frag).tobytes()
        assert c == want_crc
        assert len(f) <= F.STORED * nchunks(len(raw)) + len(raw)
        assert inflate_final(f + FINAL_BLOCK) == raw
        fin, c2 = ctx.deflate(arr, crc=crc, final=True)
        assert host(fin).tobytes() == f + FINAL_BLOCK and c2 == want_crc
        assert inflate_final(host(fin)) == raw
        frags.append(f)
    assert frags[0] == frags[1]
    return frags[0]


SIZES = [0, 1, 2, CH - 1, CH, CH + 1, 2 * CH + 1, (SCAN_WIDTH + 1) * CH + 3]


@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, n):
    rng = np.random.default_rng(n)
    assert check(ctx, np.zeros(n, dtype=np.uint8)) is not None
    check(ctx, np.full(n, 0xC3, dtype=np.uint8))
    f = check(ctx, rng.integers(0, 256, n, dtype=np.uint8))
    if n >= 1024:  # (a handful of random bytes does have a shorter dynamic form)
        assert len(f) == n + F.STORED * nchunks(n)
    # a skewed source: dynamic blocks, smaller than the input
    g = check(ctx, np.minimum(rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)) >> 2)
    if n >= 1024:
        assert len(g) < n


def test_uniform_random_chunks_are_stored(ctx):
    n = 3 * CH + 77
    data = np.random.default_rng(1).integers(0, 256, n, dtype=np.uint8)
    f = check(ctx, data)
    assert len(f) == n + F.STORED * 4
    at = 0
    for c in F.chunks_of(data):  # 00, LEN, NLEN, the bytes
        assert f[at: at + 5] == bytes([0, len(c) & 255, len(c) >> 8, ~len(c) & 255, (~len(c) >> 8) & 255]) and f[at + 5: at + 5 + len(c)] == c
        at += 5 + len(c)


def test_fibonacci_alone_and_between_stored_chunks(ctx):
    rng = np.random.default_rng(2)
    for fib in (F.fibonacci_chunk(), F.fibonacci_chain()):
        alone = check(ctx, fib)
        assert len(alone) < len(fib) // 2
        pad = np.full(CH - len(fib), fib[-1], dtype=np.uint8)  # fills the chunk with its most frequent value
        mid = np.concatenate([fib, pad])
        data = np.concatenate([rng.integers(0, 256, CH, dtype=np.uint8), mid, rng.integers(0, 256, CH, dtype=np.uint8)])
        f = check(ctx, data)
        assert f[:1] == b"\x00" and f[CH + 5: CH + 6] != b"\x00"   # stored, then a dynamic block
        assert len(f) == 2 * (CH + F.STORED) + len(check(ctx, mid))


def test_sorted_bodies_come_out_smaller(ctx):
    """the point of the feature: a real sorted body, and one with taxids, must shrink (zlib's Huffman-only coder does:
    tests/test_deflate_cpu.py)"""
    for body in F.sorted_bodies():
        f = check(ctx, body)
        print("sorted body: %d -> %d (%.4f)" % (len(body), len(f), len(f) / len(body)))
        assert len(f) < len(body)


def test_size_against_the_reference_coder(ctx):
    for name, data in (("fibonacci", F.fibonacci_chunk()), ("sorted", F.sorted_bodies()[0]), ("sorted+taxids", F.sorted_bodies()[1])):
        mine, ref = len(check(ctx, data)), len(F.huffman_only(data))
        k = nchunks(len(data))
        print("%s: %d bytes, %d chunks: device %d, zlib Z_HUFFMAN_ONLY %d, excess %.2f bytes per chunk, %.4f %% of the input"
              % (name, len(data), k, mine, ref, (mine - ref) / k, 100.0 * (mine - ref) / len(data)))
        assert mine <= ref + EXCESS_PER_CHUNK * k


def guarded(n, offset):
    """a device buffer of n bytes `offset` bytes behind a 16-byte boundary, inside guard bytes"""
    import torch
    whole = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    base = (-whole.data_ptr()) % 16 + 16 + offset
    return whole, whole[base: base + n], base


def mixed_input():
    rng = np.random.default_rng(3)
    return np.concatenate([F.fibonacci_chunk(), rng.integers(0, 256, CH - 28656 + 1000, dtype=np.uint8), np.zeros(333, dtype=np.uint8)])


@pytest.mark.parametrize("offset", range(1, 16))
def test_unaligned_buffers_and_guard_bytes(ctx, offset):
    data = mixed_input()
    want = check(ctx, data) + FINAL_BLOCK
    for so, do in ((offset, 0), (0, offset), (offset, 16 - offset), (offset, offset)):
        _, src, _ = guarded(len(data), so)
        src.copy_(dev(data))
        assert src.data_ptr() % 16 == so
        whole, out, base = guarded(len(want), do)
        assert out.data_ptr() % 16 == do
        frag, crc = ctx.deflate(src, final=True, out=out)
        assert host(frag).tobytes() == want and crc == zlib.crc32(data.tobytes())
        w = host(whole)
        assert (w[:base] == 0xA5).all() and (w[base + len(want):] == 0xA5).all()


def test_capacity_and_size_query(ctx, lib):
    data = mixed_input()
    want = check(ctx, data)
    n_out = len(want)
    L = ctx.L
    for src in (data, dev(data)):
        ps = src.ctypes.data if isinstance(src, np.ndarray) else src.data_ptr()
        m, c = C.c_uint64(), C.c_uint32(7)
        assert L.ukm_deflate(ctx.h, ps, len(data), 0, None, 0, C.byref(m), C.byref(c)) == lib.ERR_CAPACITY
        assert m.value == n_out and c.value == 7      # the size query; the CRC is written on success only
        for cap in (n_out - 1, 0):
            whole, out, base = guarded(n_out, 5)
            m = C.c_uint64()
            assert L.ukm_deflate(ctx.h, ps, len(data), 0, out.data_ptr(), cap, C.byref(m), C.byref(c)) == lib.ERR_CAPACITY
            assert m.value == n_out and (host(whole) == 0xA5).all()
        whole, out, base = guarded(n_out, 5)
        c = C.c_uint32(0)
        assert L.ukm_deflate(ctx.h, ps, len(data), 0, out.data_ptr(), n_out, C.byref(m), C.byref(c)) == lib.OK
        assert m.value == n_out and host(out).tobytes() == want and c.value == zlib.crc32(data.tobytes())
        hout = np.full(n_out + 8, 0xA5, dtype=np.uint8)   # a host output: nothing behind n_out is touched either
        assert L.ukm_deflate(ctx.h, ps, len(data), 0, hout.ctypes.data, n_out, C.byref(m), C.byref(c)) == lib.OK
        assert hout[:n_out].tobytes() == want and (hout[n_out:] == 0xA5).all()
    with pytest.raises(lib.CapacityError) as e:
        ctx.deflate(data, out=np.empty(n_out - 1, dtype=np.uint8))
    assert e.value.needed == n_out


def test_same_call_twice_same_bytes(ctx):
    data = dev(np.concatenate([mixed_input(), F.sorted_bodies()[0]]))
    a, ca = ctx.deflate(data, final=True)
    b, cb = ctx.deflate(data, final=True)
    assert host(a).tobytes() == host(b).tobytes() and ca == cb


@pytest.mark.parametrize("n", [1, CH + 1, (SCAN_WIDTH + 1) * CH + 3])
def test_calls_do_not_depend_on_what_the_workspace_held(ctx, lib, n):
    """sums, offsets, the scan's total, code lengths and CRCs all live in the workspace: one chunk, two, and more chunks than
    one round of the scan workgroup, over a workspace of zeros and of ones; host input, so the source is staged there too"""
    rng = np.random.default_rng(n)
    data = np.minimum(rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)) >> 2

    def run():
        got = []
        for gz in (False, True):
            frag, crc = ctx.deflate(data, gzip=gz)
            with pytest.raises(lib.CapacityError) as e:  # the size query
                ctx.deflate(data, gzip=gz, out=np.empty(0, dtype=np.uint8))
            got.append((frag.tobytes(), len(frag), crc, e.value.needed))
        return got
    want = run()
    assert all(size == needed and crc == zlib.crc32(data.tobytes()) for _, size, crc, needed in want)
    assert gzip.decompress(want[1][0]) == data.tobytes()
    for byte in (0x00, 0xFF):
        ctx.set_option("ws_poison", byte)
        try:
            assert run() == want
        finally:
            ctx.set_option("ws_poison", None)


def test_empty_input(ctx, lib):
    e = np.empty(0, dtype=np.uint8)
    for arr in (e, dev(e)):
        f, c = ctx.deflate(arr, crc=123)
        assert len(f) == 0 and c == 123
        f, c = ctx.deflate(arr, crc=123, final=True)
        assert host(f).tobytes() == FINAL_BLOCK and c == 123
        f, c = ctx.deflate(arr, gzip=True)
        assert gzip.decompress(host(f).tobytes()) == b"" and c == 0


def test_chaining(ctx):
    """fragments concatenate, behind zlib's own sync-flushed output too; the CRC runs through"""
    prefix = b"a header of some kind" * 3
    a, b = mixed_input(), F.sorted_bodies()[1][:70000]
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    stream = z.compress(prefix) + z.flush(zlib.Z_SYNC_FLUSH)
    crc = zlib.crc32(prefix)
    fa, crc = ctx.deflate(dev(a), crc=crc)
    fb, crc = ctx.deflate(b, crc=crc, final=True)
    assert crc == zlib.crc32(prefix + a.tobytes() + b.tobytes())
    assert inflate_final(stream + host(fa).tobytes() + host(fb).tobytes()) == prefix + a.tobytes() + b.tobytes()


def test_gzip_member(ctx, lib):
    for data in (mixed_input(), F.sorted_bodies()[0], np.frombuffer(b"x", dtype=np.uint8)):
        for arr in (data, dev(data)):
            f, c = ctx.deflate(arr, gzip=True)
            f = host(f).tobytes()
            assert f[:2] == b"\x1f\x8b" and gzip.decompress(f) == data.tobytes() and c == zlib.crc32(data.tobytes())
            assert len(f) <= lib.deflate_bound(len(data), gzip=True)
    with pytest.raises(lib.UkmError) as e:
        ctx.deflate(data, crc=1, gzip=True)
    assert e.value.code == lib.ERR_INVALID


@pytest.mark.parametrize("on_device", [False, True])
def test_unikfile_device_deflate(ctx, tmp_path, on_device):
    from unikmer_amd import unikfile as U
    rng = np.random.default_rng(4)
    keys = np.unique(rng.integers(0, 1 << 62, 60001, dtype=np.uint64))
    tax = rng.integers(1, 5000, len(keys)).astype(np.uint32)
    for flags, t in ((U.SORTED | U.CANONICAL, None), (U.SORTED | U.INCLUDE_TAXID, tax), (U.COMPACT, None)):
        h = {"k": 31, "flag": flags, "taxid_bytes": 2}
        kk, tt = keys, t
        if on_device:
            import torch
            kk = torch.from_numpy(keys.view(np.int64).copy()).cuda()
            tt = None if t is None else torch.from_numpy(t.view(np.int32).copy()).cuda()
        plain, gz_dev, gz_host = (str(tmp_path / n) for n in ("plain.unik", "dev.unik", "host.unik"))
        U.save(ctx, plain, h, kk, tt, compress=False)
        U.save(ctx, gz_dev, h, kk, tt, deflate="device")
        U.save(ctx, gz_host, h, kk, tt, deflate="host")
        want = open(plain, "rb").read()
        got = open(gz_dev, "rb").read()
        assert got[:2] == b"\x1f\x8b" and gzip.decompress(got) == want == gzip.decompress(open(gz_host, "rb").read())
        if flags & U.SORTED:
            assert len(got) < len(want)
        h2, k2, t2 = U.load(ctx, gz_dev, device=on_device)
        assert np.array_equal(host64(k2), keys) and h2["number"] == len(keys)
        if t is not None:
            assert np.array_equal(host(t2).view(np.uint32) if on_device else t2, t)


def host64(t):
    return t.cpu().numpy().view(np.uint64) if hasattr(t, "cpu") else np.asarray(t, dtype=np.uint64)
