"""The body of a `.unik` file in plain Python: what unik::Writer (write_code_with_taxid, flush) puts behind the header and
what unik::Reader::read takes from it (unikmer_amd/host/unik.hpp), statement by statement.  The reference of the codec
tests; it imports nothing of the code under test.  tests/test_unik_codec_cpu.py pins it to unik.hpp through the driver's
CPU-only commands."""
import struct

import numpy as np

COMPACT, CANONICAL, SORTED, INCLUDE_TAXID, HASHED, SCALED = 1, 2, 4, 8, 16, 32
M64 = (1 << 64) - 1


def put_be(v, n):
    """unik.hpp put_be: the low n bytes, big-endian"""
    return (int(v) & ((1 << (8 * n)) - 1)).to_bytes(n, "big")


def byte_len(v):
    n = 1
    v >>= 8
    while v:
        n += 1
        v >>= 8
    return n


def record_bytes(k, flags):
    return (k + 3) // 4 if flags & COMPACT else 8


def encode(codes, taxids, k, flags, tb):
    """bytes behind the header for these records; taxids None = zeros (Writer::write_code).  ValueError where the
    Writer throws."""
    codes = [int(c) for c in codes]
    tax = [0] * len(codes) if taxids is None else [int(t) for t in taxids]
    tx = bool(flags & INCLUDE_TAXID)
    out = bytearray()
    if not flags & SORTED:
        n = record_bytes(k, flags)
        for c, t in zip(codes, tax):
            out += put_be(c, n)
            if tx:
                out += put_be(t, tb)
        return bytes(out)
    prev = 0
    for j in range(0, len(codes) - 1, 2):
        first, code = codes[j], codes[j + 1]
        if first < prev or code < first:
            raise ValueError("codes written to a sorted .unik must be ascending")
        d0, d1 = first - prev, code - first
        l0, l1 = byte_len(d0), byte_len(d1)
        out.append(((l0 - 1) << 3) | (l1 - 1))
        out += put_be(d0, l0) + put_be(d1, l1)
        if tx:
            out += put_be(tax[j], tb) + put_be(tax[j + 1], tb)
        prev = code
    if len(codes) & 1:
        out.append(128)
        out += put_be(codes[-1], 8)
        if tx:
            out += put_be(tax[-1], tb)
    return bytes(out)


def decode(body, k, flags, tb):
    """(codes uint64, taxids uint32 or None) as Reader::read returns them; ValueError where it throws"""
    body = bytes(body)
    tx = bool(flags & INCLUDE_TAXID)
    codes, tax = [], []
    pos = 0

    def must(n):
        nonlocal pos
        if pos + n > len(body):
            raise ValueError("unexpected EOF")
        b = body[pos:pos + n]
        pos += n
        return int.from_bytes(b, "big")

    if not flags & SORTED:
        n = record_bytes(k, flags)
        while pos < len(body):
            if pos + n > len(body):
                raise ValueError("truncated record")
            codes.append(must(n))
            if tx:
                tax.append(must(tb))
    else:
        prev = 0
        while pos < len(body):
            ctrl = must(1)
            if ctrl & 128:
                prev = must(8)
                codes.append(prev)
                if tx:
                    tax.append(must(tb))
                continue
            l0, l1 = ((ctrl >> 3) & 7) + 1, (ctrl & 7) + 1
            if pos + l0 + l1 > len(body):
                raise ValueError("unexpected EOF")
            c0 = (prev + must(l0)) & M64
            c1 = (c0 + must(l1)) & M64
            prev = c1
            codes += [c0, c1]
            if tx:
                tax.append(must(tb))
                tax.append(must(tb))
    return np.array(codes, dtype=np.uint64), (np.array(tax, dtype=np.uint32) if tx else None)


def header(k, flags, number=M64, global_taxid=0, tb=4, description=b"", scale=1, max_hash=M64):
    """unik::Writer::write_header"""
    return (b".unikmer" + bytes([5, 0, k, 0]) + struct.pack(">IQIB3x", flags, number, global_taxid, tb)
            + struct.pack(">I", len(description)) + description + struct.pack(">IQ", scale, max_hash) + bytes(52))
