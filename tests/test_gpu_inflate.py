"""ukm_inflate on the device: what ukm_deflate and zlib's Huffman-only coder write comes back byte for byte, with zlib's
CRC-32; where the device must stop is what tests/inflate_model.py says (held to zlib in tests/test_inflate_cpu.py).  Every
case from host arrays and from device tensors."""
import ctypes as C
import gzip
import os
import re
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_fixtures as F  # noqa: E402
import inflate_model as IM  # noqa: E402

pytestmark = pytest.mark.gpu

CH = F.CH
MARKER = IM.MARKER
EMPTY_STORED = b"\x00" + MARKER      # an empty stored block that begins on a byte boundary


def inflate_constant(name):
    src = open(os.path.join(F.ROOT, "unikmer_amd", "csrc", "ukm_inflate.hip")).read()
    m = re.search(r"constexpr int %s = (\d+);" % name, src)
    assert m, name
    return int(m.group(1))


TILE = inflate_constant("INF_CAND_TILE")   # source bytes per workgroup of the candidate search


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
    return torch.from_numpy(np.frombuffer(bytes(a), dtype=np.uint8).copy()).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t, dtype=np.uint8)


def run(ctx, frag, crc=0):
    """(out, consumed): the call on a host array and on a device tensor, which agree; the CRC is zlib's"""
    frag = bytes(frag)
    got = []
    for arr in (np.frombuffer(frag, dtype=np.uint8), dev(frag)):
        out, consumed, c = ctx.inflate(arr, crc=crc)
        assert type(out) is type(arr)
        o = host(out).tobytes()
        assert c == zlib.crc32(o, crc)
        got.append((o, consumed))
    assert got[0] == got[1]
    return got[0]


def skewed(n, seed=0):
    rng = np.random.default_rng(seed)
    return (np.minimum(rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)) >> 2).astype(np.uint8)


def random_bytes(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def stored(payload):
    n = len(payload)
    assert n <= 65535
    return bytes([0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + bytes(payload)


def round_trip_inputs():
    alt = np.empty(CH + 99, dtype=np.uint8)
    alt[0::2], alt[1::2] = 3, 200
    mix = np.concatenate([random_bytes(CH, 5), skewed(CH, 6), random_bytes(CH, 7), skewed(CH // 2, 8)])
    ins = {"len%d" % n: skewed(n, n) for n in (0, 1, CH - 1, CH, CH + 1, 3 * CH + 5)}
    ins.update({"fibonacci chain": F.fibonacci_chain(), "one value": np.full(2 * CH + 17, 0x41, dtype=np.uint8), "two values": alt,
                "random": random_bytes(2 * CH + 100), "alternating chunks": mix,
                "sorted": F.sorted_bodies()[0], "sorted+taxids": F.sorted_bodies()[1]})
    return ins


@pytest.mark.parametrize("name", list(round_trip_inputs()))
def test_round_trip(ctx, name):
    x = round_trip_inputs()[name]
    raw = x.tobytes()
    frag, crc = ctx.deflate(x)
    frag = host(frag).tobytes()
    assert run(ctx, frag) == (raw, len(frag))
    assert run(ctx, frag, crc=0x1234) == (raw, len(frag))
    fin, _ = ctx.deflate(x, final=True)
    fin = host(fin).tobytes()
    assert run(ctx, fin) == (raw, len(fin) - 2)


def test_round_trip_of_more_segments_than_one_scan_round(ctx):
    """about 9.5 MiB: more than 256 segments, so scan_sums_kernel runs more than one round"""
    import torch
    body = F.sorted_bodies()[0]
    x = np.tile(body, (9 * (1 << 20) + (1 << 19)) // len(body) + 1)
    assert len(x) // CH > 256
    frag, crc = ctx.deflate(dev(x))
    out, consumed, c = ctx.inflate(frag)
    assert consumed == frag.numel() and c == crc == zlib.crc32(x.tobytes())
    assert torch.equal(out, dev(x))


@pytest.mark.parametrize("mem_level", [9, 8, 1])
@pytest.mark.parametrize("name", list(round_trip_inputs()))
def test_zlib_made_streams(ctx, name, mem_level):
    """several bit-packed blocks per segment, fixed blocks, stored blocks at unaligned bit positions"""
    raw = round_trip_inputs()[name].tobytes()
    z = zlib.compressobj(6, zlib.DEFLATED, -15, mem_level, zlib.Z_HUFFMAN_ONLY)
    src = b"".join(z.compress(c) + z.flush(zlib.Z_FULL_FLUSH) for c in F.chunks_of(raw))
    if mem_level == 9:
        assert src == F.huffman_only(raw)
    assert run(ctx, src) == (raw, len(src))


def test_stops_in_front_of_matches(ctx):
    text = b"the quick brown fox jumps over the lazy dog, " * 4000
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    assert run(ctx, z.compress(text) + z.flush()) == (b"", 0)
    raw = F.sorted_bodies()[0].tobytes()
    frag = host(ctx.deflate(F.sorted_bodies()[0])[0]).tobytes()
    tail = raw[-5000:] + b"tail " * 1000
    z = zlib.compressobj(6, zlib.DEFLATED, -15, zdict=raw[-32768:])
    src = frag + z.compress(tail) + z.flush()
    out, consumed = run(ctx, src)
    assert (out, consumed) == (raw, len(frag)) == IM.inflate_prefix(src)[::-1]
    d = zlib.decompressobj(-15, zdict=out[-32768:])
    assert d.decompress(src[consumed:]) == tail and d.eof


def test_one_lane_is_not_asked_for_more_than_its_limit(ctx):
    """a Huffman-only stream that never flushes is ONE segment: the device leaves it to zlib in front of the block that takes
    it beyond 2^20 literals, and takes what stands in front of it"""
    head = skewed(CH + 5, 41)
    frag = host(ctx.deflate(head)[0]).tobytes()
    z = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
    run_ = z.compress(skewed(IM.LITERAL_LIMIT + 70000, 42).tobytes()) + z.flush(zlib.Z_SYNC_FLUSH)
    assert run(ctx, run_) == (b"", 0)          # (the model says the same: tests/test_inflate_cpu.py)
    assert run(ctx, frag + run_) == (head.tobytes(), len(frag))
    z = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
    below = skewed(IM.LITERAL_LIMIT - 5, 43).tobytes()
    src = z.compress(below) + z.flush(zlib.Z_SYNC_FLUSH)
    assert run(ctx, src) == (below, len(src))


def four_chunks(third_random):
    x = np.concatenate([skewed(CH, 11), skewed(CH, 12), random_bytes(CH, 13) if third_random else skewed(CH, 13), skewed(CH - 77, 14)])
    return x


def chunk_starts(frag):
    """where the chunks of a ukm_deflate fragment begin: a stored chunk ends behind its bytes, a dynamic one behind its marker"""
    at, starts = 0, []
    while at < len(frag):
        starts.append(at)
        if frag[at] & 6 == 0:
            at += F.STORED + (frag[at + 1] | frag[at + 2] << 8)
        else:
            end, _, early = IM.parse_segment(frag, at)
            assert not early
            at = end
    return starts


def test_cut_fragments_stop_where_the_model_stops(ctx):
    for third_random in (False, True):
        x = four_chunks(third_random)
        frag = host(ctx.deflate(x)[0]).tobytes()
        starts = chunk_starts(frag)
        assert len(starts) == 4
        last = starts[3]
        for cut in (last, last + 1, last + 7, last + 100, (last + len(frag)) // 2, len(frag) - 5, len(frag) - 1, starts[2] + 3, starts[2] + 1000):
            want = IM.inflate_prefix(frag[:cut])
            assert run(ctx, frag[:cut]) == want[::-1], cut
            assert x.tobytes().startswith(want[1])


def set_bits(buf, bit, value, n):
    for i in range(n):
        if (value >> i) & 1:
            buf[(bit + i) >> 3] |= 1 << ((bit + i) & 7)
        else:
            buf[(bit + i) >> 3] &= ~(1 << ((bit + i) & 7))


def test_damaged_headers_stop_the_device_without_a_fault(ctx):
    x = four_chunks(False)
    frag = host(ctx.deflate(x)[0]).tobytes()
    c = chunk_starts(frag)[2]
    assert frag[c] & 7 == 4                       # not final, dynamic
    cases = {}
    b = bytearray(frag)
    b[c] |= 6
    cases["BTYPE 11"] = bytes(b)
    b = bytearray(frag)
    b[c + 1] ^= 1 << 5                            # bit 13: the lowest of HCLEN
    cases["HCLEN"] = bytes(b)
    b = bytearray(frag)
    set_bits(b, 8 * c + 17, 0b001001001, 9)      # the code-length code's 16, 17 and 18: three codes of one bit
    cases["over-subscribed"] = bytes(b)
    b = bytearray(frag)
    b[c] |= 1
    cases["final"] = bytes(b)
    xs = four_chunks(True)
    fs = host(ctx.deflate(xs)[0]).tobytes()
    cs = chunk_starts(fs)[2]
    assert fs[cs] == 0 and fs[cs + 1] | fs[cs + 2] << 8 == CH
    b = bytearray(fs)
    b[cs + 3] ^= 0x10
    cases["NLEN"] = bytes(b)
    for name, src in cases.items():
        want = IM.inflate_prefix(src)
        assert run(ctx, src) == want[::-1], name
        if name in ("BTYPE 11", "over-subscribed", "final", "NLEN"):
            assert want[0] == (cs if name == "NLEN" else c), name
    # and bits flipped all over: whatever they make of the headers, the device stops where the model stops
    rng = np.random.default_rng(99)
    for _ in range(8):
        b = bytearray(frag)
        at = int(rng.integers(0, len(b)))
        b[at] ^= 1 << int(rng.integers(0, 8))
        assert run(ctx, bytes(b)) == IM.inflate_prefix(bytes(b))[::-1], at


def decoy_fragment():
    z = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
    return z.compress(b"other data, which parses but is off the chain " * 40) + z.flush(zlib.Z_FULL_FLUSH)


def test_false_candidates_inside_a_stored_payload(ctx):
    garbage = random_bytes(3000, 21).tobytes()
    for behind in (b"\x05" + garbage, decoy_fragment() + garbage):
        payload = skewed(700, 22).tobytes() + MARKER + behind
        src = stored(payload) + EMPTY_STORED
        assert run(ctx, src) == (payload, len(src))
        src = stored(payload) + stored(b"more") + EMPTY_STORED + host(ctx.deflate(skewed(5000, 23))[0]).tobytes()
        assert run(ctx, src) == (payload + b"more" + skewed(5000, 23).tobytes(), len(src))


@pytest.mark.parametrize("at", [TILE - 4, TILE - 3, TILE - 2, TILE - 1, TILE, 2 * TILE - 2])
def test_markers_across_the_candidate_tiles(ctx, at):
    """the pattern begins at each of the last four bytes of a tile of the candidate search and at the first byte of the next"""
    # a real marker: an empty stored block whose 00 00 FF FF begins at `at`; without it as a candidate the chain would end
    a, b = skewed(at - 6, 31).tobytes(), skewed(4000, 32).tobytes()
    src = stored(a) + EMPTY_STORED + stored(b) + EMPTY_STORED + host(ctx.deflate(skewed(3000, 33))[0]).tobytes()
    assert src[at: at + 4] == MARKER and src.find(MARKER) == at
    assert run(ctx, src) == (a + b + skewed(3000, 33).tobytes(), len(src))
    # a decoy: the same bytes at the same place inside a stored payload, a complete fragment behind them
    payload = bytearray(skewed(at + 3000, 34).tobytes())
    decoy = MARKER + decoy_fragment()
    payload[at - 5: at - 5 + len(decoy)] = decoy
    src = stored(payload) + EMPTY_STORED
    assert src[at: at + 4] == MARKER
    assert run(ctx, src) == (bytes(payload), len(src))


def guarded(n, offset):
    """a device buffer of n bytes `offset` bytes behind a 16-byte boundary, inside guard bytes"""
    import torch
    whole = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    base = (-whole.data_ptr()) % 16 + 16 + offset
    return whole, whole[base: base + n], base


def contract_input(ctx):
    x = np.concatenate([F.fibonacci_chunk(), random_bytes(CH - 28656 + 1000, 3), np.zeros(333, dtype=np.uint8), F.sorted_bodies()[1][:50000]])
    return x.tobytes(), host(ctx.deflate(x, final=True)[0]).tobytes()


def test_capacity_and_size_query(ctx, lib):
    raw, frag = contract_input(ctx)
    L = ctx.L
    for src in (np.frombuffer(frag, dtype=np.uint8), dev(frag)):
        ps = src.ctypes.data if isinstance(src, np.ndarray) else src.data_ptr()
        m, used, c = C.c_uint64(), C.c_uint64(), C.c_uint32(7)
        assert L.ukm_inflate(ctx.h, ps, len(frag), 0, None, 0, C.byref(m), C.byref(used), C.byref(c)) == lib.ERR_CAPACITY
        assert (m.value, used.value, c.value) == (len(raw), len(frag) - 2, 7)   # the CRC is written on success only
        for cap in (len(raw) - 1, 0):
            whole, out, base = guarded(len(raw), 5)
            m, used = C.c_uint64(), C.c_uint64()
            assert L.ukm_inflate(ctx.h, ps, len(frag), 0, out.data_ptr(), cap, C.byref(m), C.byref(used), C.byref(c)) == lib.ERR_CAPACITY
            assert (m.value, used.value) == (len(raw), len(frag) - 2) and (host(whole) == 0xA5).all()
        whole, out, base = guarded(len(raw), 5)
        c = C.c_uint32(0)
        assert L.ukm_inflate(ctx.h, ps, len(frag), 0, out.data_ptr(), len(raw), C.byref(m), C.byref(used), C.byref(c)) == lib.OK
        assert host(out).tobytes() == raw and c.value == zlib.crc32(raw)
        w = host(whole)
        assert (w[:base] == 0xA5).all() and (w[base + len(raw):] == 0xA5).all()
        hout = np.full(len(raw) + 8, 0xA5, dtype=np.uint8)
        assert L.ukm_inflate(ctx.h, ps, len(frag), 0, hout.ctypes.data, len(raw) + 8, C.byref(m), C.byref(used), C.byref(c)) == lib.OK
        assert hout[:len(raw)].tobytes() == raw and (hout[len(raw):] == 0xA5).all()
        assert L.ukm_inflate(ctx.h, ps, len(frag), 1, None, 0, C.byref(m), C.byref(used), C.byref(c)) == lib.ERR_INVALID
        assert L.ukm_inflate(ctx.h, ps, 0, 0, None, 0, C.byref(m), C.byref(used), C.byref(c)) == lib.OK and (m.value, used.value) == (0, 0)
    with pytest.raises(lib.CapacityError) as e:
        ctx.inflate(np.frombuffer(frag, dtype=np.uint8), out=np.empty(len(raw) - 1, dtype=np.uint8))
    assert e.value.needed == len(raw) and e.value.consumed == len(frag) - 2
    assert lib.inflate_bound(1000) == 8000 and lib.inflate_bound(0) == 0
    for name in ("ukm_inflate", "ukm_inflate_bound"):
        assert name in lib.SYMBOLS


@pytest.mark.parametrize("offset", [1, 3, 7])
def test_unaligned_buffers_inside_one_slab(ctx, offset):
    import torch
    raw, frag = contract_input(ctx)
    slab = torch.full((len(frag) + len(raw) + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    s0 = (-slab.data_ptr()) % 16 + 16 + offset
    o0 = s0 + len(frag) + (-(s0 + len(frag) + slab.data_ptr())) % 16 + 16 + offset
    src, out = slab[s0: s0 + len(frag)], slab[o0: o0 + len(raw)]
    assert src.data_ptr() % 16 == offset and out.data_ptr() % 16 == offset
    src.copy_(dev(frag))
    got, consumed, crc = ctx.inflate(src, out=out)
    assert host(got).tobytes() == raw and consumed == len(frag) - 2 and crc == zlib.crc32(raw)
    w = host(slab)
    assert w[s0: s0 + len(frag)].tobytes() == frag
    assert (w[:s0] == 0xA5).all() and (w[s0 + len(frag): o0] == 0xA5).all() and (w[o0 + len(raw):] == 0xA5).all()


def test_same_call_twice_and_any_workspace(ctx, lib):
    """candidates, segment results, chain, sums, checkpoints and CRCs all live in the workspace"""
    raw, frag = contract_input(ctx)
    z = zlib.compressobj(6, zlib.DEFLATED, -15, 1, zlib.Z_HUFFMAN_ONLY)
    small_blocks = b"".join(z.compress(c) + z.flush(zlib.Z_FULL_FLUSH) for c in F.chunks_of(raw))

    def once():
        return [run(ctx, f) for f in (frag, small_blocks, frag[:len(frag) // 2])]
    want = once()
    assert want[0] == (raw, len(frag) - 2) and want[1] == (raw, len(small_blocks))
    assert once() == want
    for byte in (0x00, 0xFF):
        ctx.set_option("ws_poison", byte)
        try:
            assert once() == want
        finally:
            ctx.set_option("ws_poison", None)


def host64(t):
    return t.cpu().numpy().view(np.uint64) if hasattr(t, "cpu") else np.asarray(t, dtype=np.uint64)


@pytest.mark.parametrize("on_device", [False, True])
def test_unikfile_device_inflate(ctx, lib, tmp_path, on_device, monkeypatch):
    from unikmer_amd import unikfile as U
    rng = np.random.default_rng(4)
    keys = np.unique(rng.integers(0, 1 << 62, 60001, dtype=np.uint64))
    unsorted = rng.permutation(keys)
    tax = rng.integers(1, 5000, len(keys)).astype(np.uint32)
    calls = []
    real = ctx.inflate
    monkeypatch.setattr(ctx, "inflate", lambda *a, **k: calls.append(1) or real(*a, **k))
    for flags, kk, t in ((U.SORTED | U.CANONICAL, keys, None), (U.SORTED | U.INCLUDE_TAXID, keys, tax), (U.COMPACT, unsorted, None),
                         (U.INCLUDE_TAXID, unsorted, tax), (U.SORTED, keys[:-1], None)):
        h = {"k": 31, "flag": flags, "taxid_bytes": 2, "description": "made by the test"}
        gz_dev, gz_host = str(tmp_path / "dev.unik"), str(tmp_path / "host.unik")
        U.save(ctx, gz_dev, h, kk, t if t is None else t[:len(kk)], deflate="device")
        U.save(ctx, gz_host, h, kk, t if t is None else t[:len(kk)], deflate="host")
        for path, through_device in ((gz_dev, True), (gz_host, False)):
            del calls[:]
            h2, k2, t2 = U.load(ctx, path, device=on_device, inflate="device")
            assert bool(calls) == through_device
            assert np.array_equal(host64(k2), kk) and h2["number"] == len(kk) and h2["description"] == "made by the test"
            if t is not None:
                assert np.array_equal(host(t2).view(np.uint32) if on_device else t2, t[:len(kk)])
            h3, k3, t3 = U.load(ctx, path, device=on_device)
            assert np.array_equal(host64(k3), kk)
    # the device path really carried the device-written files: the whole fragment but its final block
    raw = open(gz_dev, "rb").read()
    got = U._device_gunzip(ctx, gz_dev, on_device)
    assert got is not None and len(got[1]) == len(gzip.decompress(raw)) - len(U.header_bytes(got[0]))
    assert U._device_gunzip(ctx, gz_host, on_device) is None
    # one corrupted body byte: an error, never wrong records
    bad = bytearray(raw)
    bad[len(bad) // 2] ^= 0x40
    open(gz_dev, "wb").write(bytes(bad))
    assert U._device_gunzip(ctx, gz_dev, on_device) is None       # the device path declines: the trailer does not fit
    with pytest.raises((zlib.error, OSError, EOFError, ValueError, lib.UkmError)):   # zlib's own words, from the host path
        U.load(ctx, gz_dev, device=on_device, inflate="device")
    # a second member behind the first: the host's way
    open(gz_dev, "wb").write(raw + gzip.compress(b""))
    assert U._device_gunzip(ctx, gz_dev, on_device) is None
