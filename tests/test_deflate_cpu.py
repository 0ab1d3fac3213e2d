"""ukm_deflate without a GPU: the code construction, block header and CRC arithmetic of unikmer_amd/csrc/ukm_huff.h as a
stand-alone program under the address and undefined-behaviour sanitizers (tests/deflate_units.cpp, with zlib's inflate as the
judge), and the two pure-host entry points ukm_crc32_combine / ukm_deflate_bound."""
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_fixtures as F  # noqa: E402

ROOT = F.ROOT
CH = F.CH


@pytest.fixture(scope="module")
def lib():
    from unikmer_amd import build, lib as L
    build.build()
    return L


def test_code_construction_under_sanitizers(tmp_path):
    """no Python-loaded code runs under a sanitizer: the header is plain C++ and gets a main() of its own.  The sorted body's
    first chunk goes in as a file."""
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the driver; it must be here"
    assert CH <= 65535
    exe = str(tmp_path / "deflate_units")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DDFL_CHUNK=%d" % CH,
           "-I", os.path.join(ROOT, "unikmer_amd", "csrc"), "-I", os.path.join(ROOT, "unikmer_amd", "host"), os.path.join(ROOT, "tests", "deflate_units.cpp"), "-o", exe, "-lz"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    work = tmp_path / "work"
    work.mkdir()
    body = F.sorted_bodies()[0]
    assert len(body) > CH
    (work / "body.bin").write_bytes(bytes(body[:CH]))
    r = subprocess.run([exe, str(work)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.returncode, r.stdout, r.stderr)
    assert "sorted body" in r.stderr


def test_symbols_listed(lib):
    for name in ("ukm_deflate", "ukm_deflate_bound", "ukm_crc32_combine"):
        assert name in lib.SYMBOLS and hasattr(lib.load(), name)


def test_crc32_combine(lib):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
    ca = zlib.crc32(a)
    assert lib.crc32_combine(ca, zlib.crc32(b""), 0) == ca
    for n in (0, 1, 255, CH):
        b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert lib.crc32_combine(ca, zlib.crc32(b), n) == zlib.crc32(a + b) == zlib.crc32(b, ca), n
        assert lib.crc32_combine(0, zlib.crc32(b), n) == zlib.crc32(b)
    # len(b) = 2^32 + 5, never materialised: b = 4096 copies of a block of 2^20 bytes and 5 more.  crc(b) and crc(a + b) by
    # chaining steps of lengths checked above in kind; the one call with the whole length must agree
    blk, tail = rng.integers(0, 256, 1 << 20, dtype=np.uint8).tobytes(), b"\x01\x02\x03\x04\x05"
    assert lib.crc32_combine(ca, zlib.crc32(blk), len(blk)) == zlib.crc32(blk, ca)
    cb, cab = 0, ca
    for _ in range(4096):
        cb, cab = lib.crc32_combine(cb, zlib.crc32(blk), len(blk)), lib.crc32_combine(cab, zlib.crc32(blk), len(blk))
    cb, cab = lib.crc32_combine(cb, zlib.crc32(tail), 5), lib.crc32_combine(cab, zlib.crc32(tail), 5)
    assert lib.crc32_combine(ca, cb, (1 << 32) + 5) == cab


def test_crc32_chain_against_zlib_at_a_size_zlib_can_hash(lib):
    blk = np.random.default_rng(6).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    c = 0
    for _ in range(64):
        c = lib.crc32_combine(c, zlib.crc32(blk), len(blk))
    assert c == zlib.crc32(blk * 64)


def test_deflate_bound(lib):
    L = lib.load()
    prev = 0
    for n in (0, 1, 2, CH - 1, CH, CH + 1, 2 * CH, 2 * CH + 1, 257 * CH + 3, (1 << 32) + 5, 1 << 40):
        want = n + F.STORED * ((n + CH - 1) // CH)
        assert L.ukm_deflate_bound(n, 0) == want == lib.deflate_bound(n)
        assert L.ukm_deflate_bound(n, lib.DEFLATE_FINAL) == want + 2 == lib.deflate_bound(n, final=True)
        assert L.ukm_deflate_bound(n, lib.DEFLATE_GZIP) == L.ukm_deflate_bound(n, lib.DEFLATE_GZIP | lib.DEFLATE_FINAL) == want + 2 + 18
        assert want >= prev
        prev = want
    assert F.STORED == 5
    for n in range(0, 3 * CH, 997):
        assert L.ukm_deflate_bound(n + 1, 0) > L.ukm_deflate_bound(n, 0)


def test_huffman_coding_alone_shrinks_a_sorted_body():
    """the condition the GPU test puts on the device's output, met by zlib's Huffman-only coder on the same chunks: a test
    that passed while the device stored every chunk would hide the whole feature"""
    for body in F.sorted_bodies():
        z = F.huffman_only(body)
        assert zlib.decompressobj(-15).decompress(z + b"\x03\x00") == bytes(body)
        assert len(z) < len(body), (len(z), len(body))
        print("Huffman only: %d -> %d (%.3f)" % (len(body), len(z), len(z) / len(body)))
