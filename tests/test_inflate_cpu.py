"""tests/inflate_model.py, the model the GPU tests of ukm_inflate compare against, held to zlib; and the host pieces of the
driver's device gunzip path (tests/inflate_units.cpp, a sanitized stand-alone program).  No GPU."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import deflate_fixtures as F
import inflate_model as IM

ROOT = F.ROOT


def flushed(data, mem_level, flush=zlib.Z_FULL_FLUSH):
    """zlib, Huffman coding only, a flush behind every chunk: what deflate_fixtures.huffman_only writes at memLevel 9"""
    z = zlib.compressobj(6, zlib.DEFLATED, -15, mem_level, zlib.Z_HUFFMAN_ONLY)
    return b"".join(z.compress(c) + z.flush(flush) for c in F.chunks_of(data))


def inputs():
    rng = np.random.default_rng(20)
    skewed = np.minimum(rng.geometric(0.08, 2 * F.CH + 777), 255).astype(np.uint8)
    # a stretch that does not compress, in the middle of a chunk: at memLevel 1 (blocks of 127 symbols) zlib stores it,
    # behind a Huffman block and with no flush between: a stored block at an unaligned bit position
    skewed[5000:6000] = rng.integers(0, 256, 1000, dtype=np.uint8)
    return {"skewed": skewed.tobytes(), "random": rng.integers(0, 256, 2 * F.CH + 5, dtype=np.uint8).tobytes(),
            "three": b"abc", "sorted": F.sorted_bodies()[0].tobytes()[:3 * F.CH + 11]}


def test_model_inflates_flushed_huffman_only_streams():
    seen = set()
    for name, raw in inputs().items():
        for mem_level in (9, 8, 1):
            src = flushed(raw, mem_level)
            assert zlib.decompressobj(-15).decompress(src) == raw
            consumed, out = IM.inflate_prefix(src, seen)
            assert consumed == len(src), (name, mem_level, consumed, len(src))
            assert out == raw, (name, mem_level)
    assert {"stored", "fixed", "dynamic", "stored unaligned", "marker"} <= seen, seen


def test_model_matches_huffman_only_fixture():
    raw = inputs()["skewed"]
    assert F.huffman_only(raw) == flushed(raw, 9)


def test_model_stops_in_front_of_a_stream_with_matches():
    text = b"the quick brown fox jumps over the lazy dog, " * 400
    assert IM.inflate_prefix(zlib.compress(text, 6)[2:-4]) == (0, b"")
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    assert IM.inflate_prefix(z.compress(text) + z.flush()) == (0, b"")


def test_model_hands_over_to_zlib_with_a_dictionary():
    raw = inputs()["sorted"]
    prefix = flushed(raw, 9)
    text = raw[-5000:] + b"tail " * 1000           # matches reach back into the prefix's output
    z = zlib.compressobj(6, zlib.DEFLATED, -15, zdict=raw[-32768:])
    rest = z.compress(text) + z.flush()
    consumed, out = IM.inflate_prefix(prefix + rest)
    assert consumed == len(prefix) and out == raw
    d = zlib.decompressobj(-15, zdict=out[-32768:])
    assert d.decompress((prefix + rest)[consumed:]) == text and d.eof


def test_model_stops_at_the_last_safe_point():
    raw = inputs()["random"]                       # stored chunks
    src = flushed(raw, 9)
    full = IM.inflate_prefix(src)
    assert full == (len(src), raw)
    cut = src[: len(src) - 10]                     # inside the last blocks
    consumed, out = IM.inflate_prefix(cut)
    assert 0 < consumed < len(cut) and raw.startswith(out)
    assert zlib.decompressobj(-15).decompress(cut[:consumed]) == out
    # a final block, even an empty one, is not taken
    assert IM.inflate_prefix(src + b"\x03\x00") == full
    assert IM.inflate_prefix(b"\x03\x00") == (0, b"")
    assert IM.inflate_prefix(b"") == (0, b"")


def test_model_leaves_a_stream_that_never_flushes_to_zlib():
    """one segment is one lane's work: beyond 2^20 literals of Huffman blocks it stops in front of the block that crosses"""
    rng = np.random.default_rng(42)
    raw = np.minimum(rng.geometric(0.08, IM.LITERAL_LIMIT + 70000), 255).astype(np.uint8).tobytes()
    z = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
    src = z.compress(raw) + z.flush(zlib.Z_SYNC_FLUSH)
    assert IM.inflate_prefix(src) == (0, b"")
    head = flushed(raw[:F.CH], 9)
    assert IM.inflate_prefix(head + src) == (len(head), raw[:F.CH])


def test_model_ignores_a_marker_inside_a_stored_payload():
    payload = b"front" + IM.MARKER + b"\x05garbage that is no block" + bytes(range(200))
    z = zlib.compressobj(0, zlib.DEFLATED, -15)
    src = z.compress(payload) + z.flush(zlib.Z_SYNC_FLUSH)
    assert len(IM.candidates(src)) == 3
    assert IM.inflate_prefix(src) == (len(src), payload)
    decoy = flushed(b"other data " * 50, 9)
    payload = b"front" + IM.MARKER + decoy
    z = zlib.compressobj(0, zlib.DEFLATED, -15)
    src = z.compress(payload) + z.flush(zlib.Z_SYNC_FLUSH)
    assert IM.inflate_prefix(src) == (len(src), payload)


def test_driver_host_pieces_under_sanitizers(tmp_path):
    """tests/inflate_units.cpp: gzip framing, the Z_BLOCK search for the body's start, the dictionary resume, the trailer
    check and the refusals of unik::device_gunzip, with the block parser the kernels use (csrc/ukm_inflate.h, compiled for
    the host) standing in for the device; also that parser against zlib.  Its own process, address and UB sanitizers."""
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the driver; it must be here"
    exe = str(tmp_path / "inflate_units")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "unikmer_amd", "csrc"),
           "-I", os.path.join(ROOT, "unikmer_amd", "host"), os.path.join(ROOT, "tests", "inflate_units.cpp"), "-o", exe, "-lz", "-pthread"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "inflate_units: ok" in r.stdout
