"""The `.unik` codec without a GPU: tests/unik_model.py is pinned to unikmer_amd/host/unik.hpp through the driver's CPU-only
commands (`dump` writes with unik::Writer, `view` reads with unik::Reader), the new entry points are declared, the pure
host bound holds, and Reader::read_body / Writer::write_body run under the address and undefined-behaviour sanitizers
as a stand-alone program."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unik_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")


@pytest.fixture(scope="module")
def cli():
    from unikmer_amd import build
    build.build()

    def run(*args, stdin=None):
        return subprocess.run([BIN] + [str(a) for a in args], input=stdin, capture_output=True)
    return run


def kmer_of(code, k):
    return "".join("ACGT"[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def sorted_codes(rng, n, k):
    """ascending codes of k bases whose deltas take every byte length the k allows, duplicates included"""
    d = [int(rng.integers(0, 1 << int(rng.integers(0, 2 * k - 8)))) for _ in range(n)]
    c = np.cumsum(np.array(d, dtype=object))
    assert c[-1] < 1 << (2 * k)
    return [int(x) for x in c]


def test_dump_writes_what_the_model_encodes(cli, tmp_path):
    rng = np.random.default_rng(5)
    k = 31
    for n in (1, 2, 7, 500):
        codes = sorted_codes(rng, n, k)
        tax = [int(t) for t in rng.integers(1, 1 << 32, n)]
        # -t: a global taxid, records without taxids
        out = tmp_path / ("g%d" % n)
        text = "".join(kmer_of(c, k) + "\n" for c in codes).encode()
        assert cli("dump", "-s", "-C", "-t", 562, "-o", out, stdin=text).returncode == 0
        data = open(str(out) + ".unik", "rb").read()
        assert data[:100] == M.header(k, M.SORTED, global_taxid=562)
        assert data[100:] == M.encode(codes, None, k, M.SORTED, 4)
        # taxids per record, at every width the header can state
        for tb, max_taxid in ((4, 0xFFFFFFFF), (3, 0xFFFFFF), (2, 0xFFFF), (1, 0xFF)):
            out = tmp_path / ("t%d_%d" % (n, tb))
            text = "".join("%s\t%d\n" % (kmer_of(c, k), t) for c, t in zip(codes, tax)).encode()
            assert cli("dump", "-s", "-C", "--max-taxid", max_taxid, "-o", out, stdin=text).returncode == 0
            data = open(str(out) + ".unik", "rb").read()
            assert data[:100] == M.header(k, M.SORTED | M.INCLUDE_TAXID, tb=tb)
            assert data[100:] == M.encode(codes, tax, k, M.SORTED | M.INCLUDE_TAXID, tb)   # (taxids cut to their low bytes)


def test_dump_hashed_values_above_2_63(cli, tmp_path):
    codes = [5, (1 << 63) + 1, (1 << 63) + 1, (1 << 64) - 2, (1 << 64) - 1]
    for n in (4, 5):
        out = tmp_path / ("h%d" % n)
        text = "".join("%d\n" % c for c in codes[:n]).encode()
        assert cli("dump", "-s", "-C", "--hashed", "-k", 31, "-o", out, stdin=text).returncode == 0
        data = open(str(out) + ".unik", "rb").read()
        assert data[:100] == M.header(31, M.SORTED | M.CANONICAL | M.HASHED)
        assert data[100:] == M.encode(codes[:n], None, 31, M.SORTED, 4)
        c, t = M.decode(data[100:], 31, M.SORTED, 4)
        assert [int(x) for x in c] == codes[:n] and t is None


def view_records(cli, path, hashed=False):
    p = cli("view", "-N", path)
    assert p.returncode == 0, p.stderr
    codes = [int(x) for x in p.stdout.split()]
    p = cli("view", "-T", path)
    assert p.returncode == 0, p.stderr
    return codes, [int(x) for x in p.stdout.split()]


def test_view_reads_what_the_model_encodes(cli, tmp_path):
    rng = np.random.default_rng(6)
    n = 301
    for k in (11, 21, 32):
        srt = sorted_codes(rng, n, min(k, 31))
        uns = [int(x) for x in rng.integers(0, 1 << min(2 * k, 63), n, dtype=np.uint64)]
        tax = [int(t) for t in rng.integers(1, 1 << 32, n)]
        for flags, codes in ((M.SORTED, srt), (0, uns), (M.COMPACT, uns)):
            for tb in (0, 1, 2, 3, 4):
                fl = flags | (M.INCLUDE_TAXID if tb else 0)
                body = M.encode(codes, tax if tb else None, k, fl, tb)
                path = tmp_path / "v.unik"
                path.write_bytes(M.header(k, fl, tb=tb or 4, global_taxid=0 if tb else 9606) + body)
                got_c, got_t = view_records(cli, path)
                assert got_c == codes, (k, flags, tb)
                assert got_t == ([t & ((1 << (8 * tb)) - 1) for t in tax] if tb else [9606] * n), (k, flags, tb)
                mc, mt = M.decode(body, k, fl, tb)
                assert [int(x) for x in mc] == codes and (mt is None) == (tb == 0)
                assert tb == 0 or [int(x) for x in mt] == got_t


def test_view_reads_a_single_in_the_middle(cli, tmp_path):
    """ctrl = 128 is one full code wherever it stands and resets prev; bit 6 of a pair's control byte is ignored; the sum
    wraps mod 2^64 -- the Reader's details, as the model has them"""
    tb = 2
    body = (bytes([0x09, 0x10, 0x00, 0x02, 0x00]) + b"\xAA\x01\xBB\x02"          # pair: l0 = 2, l1 = 2 -> 4096, 4608
            + bytes([128]) + (77).to_bytes(8, "big") + b"\xCC\x03"                # single 77: prev = 77
            + bytes([0x40 | 0x00, 0x03, 0x00]) + b"\x00\x04\x00\x05"              # bit 6 set: a pair all the same -> 80, 80
            + bytes([0xFF]) + ((1 << 64) - 1).to_bytes(8, "big") + b"\x00\x06"    # any byte >= 128 is a single
            + bytes([0x00, 0x02, 0x01]) + b"\x00\x07\x00\x08")                    # wraps: 1, 2
    want = [4096, 4608, 77, 80, 80, (1 << 64) - 1, 1, 2]
    want_t = [0xAA01, 0xBB02, 0xCC03, 4, 5, 6, 7, 8]
    c, t = M.decode(body, 31, M.SORTED | M.INCLUDE_TAXID, tb)
    assert [int(x) for x in c] == want and [int(x) for x in t] == want_t
    path = tmp_path / "mid.unik"
    path.write_bytes(M.header(31, M.SORTED | M.INCLUDE_TAXID | M.HASHED | M.CANONICAL, tb=tb) + body)
    assert view_records(cli, path) == (want, want_t)
    # every proper prefix: the model raises exactly where the Reader throws
    for cut in range(len(body)):
        path.write_bytes(M.header(31, M.SORTED | M.INCLUDE_TAXID | M.HASHED | M.CANONICAL, tb=tb) + body[:cut])
        p = cli("view", "-N", path)
        try:
            M.decode(body[:cut], 31, M.SORTED | M.INCLUDE_TAXID, tb)
            assert p.returncode == 0, cut
        except ValueError as e:
            assert p.returncode != 0 and str(e).encode() in p.stderr, (cut, p.stderr)


def test_codec_symbols_and_constants_exist():
    from unikmer_amd import lib
    hdr = open(os.path.join(ROOT, "include", "unikmer_hip.h")).read()
    for name in ("ukm_unik_decode", "ukm_unik_encode", "ukm_unik_encode_bound"):
        assert name in lib.SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, hdr)
    for name, value in (("UKM_UNIK_COMPACT", 1), ("UKM_UNIK_SORTED", 4), ("UKM_UNIK_INCLUDE_TAXID", 8)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, value), hdr)
    assert re.search(r"#define\s+UKM_ERR_FORMAT\s+\(-10\)", hdr)
    assert (lib.UNIK_COMPACT, lib.UNIK_SORTED, lib.UNIK_INCLUDE_TAXID) == (M.COMPACT, M.SORTED, M.INCLUDE_TAXID) == (1, 4, 8)
    assert lib.ERR_FORMAT == -10 and issubclass(lib.FormatError, lib.UkmError)


def value_cases():
    """(codes, taxids) of the value cases of tests/test_gpu_unik_codec.py that need no device"""
    top = (1 << 64) - 1
    cases = [[], [0], [0, 0], [0, 0, 0], [7, 7, 7, 7], [top - 1, top], [top, top, top]]
    for l0 in range(1, 9):
        for l1 in range(1, 9):
            lo0, lo1 = (1 << (8 * (l0 - 1))) if l0 > 1 else 0, (1 << (8 * (l1 - 1))) if l1 > 1 else 0
            hi0, hi1 = (1 << (8 * l0)) - 1, (1 << (8 * l1)) - 1
            high = (hi0, hi1) if hi0 + hi1 <= top else (hi0 >> 1, hi1 >> 1)   # (an 8-byte delta leaves no room for both)
            for d0, d1 in ((lo0, lo1), high):
                cases.append([d0, d0 + d1])
    return cases


def test_encode_bound_through_ctypes(cli):
    from unikmer_amd import lib
    L = lib.load()
    for codes in value_cases():
        n = len(codes)
        tax = list(range(n))
        for tb in (0, 1, 2, 3, 4):
            t = M.INCLUDE_TAXID if tb else 0
            assert L.ukm_unik_encode_bound(n, 31, M.SORTED | t, tb) >= len(M.encode(codes, tax, 31, M.SORTED | t, tb))
            for k in (1, 11, 21, 32):
                for fl in (0, M.COMPACT):
                    assert L.ukm_unik_encode_bound(n, k, fl | t, tb) == len(M.encode(codes, tax, k, fl | t, tb))
                    assert lib.unik_encode_bound(n, k, fl | t, tb) == n * (M.record_bytes(k, fl) + tb)
    # the stated form of the sorted bound
    for n in (0, 1, 2, 3, 1001):
        for tb in (1, 4):
            assert L.ukm_unik_encode_bound(n, 31, M.SORTED | M.INCLUDE_TAXID, tb) <= (n + 1) // 2 * (17 + 2 * tb)


def test_read_body_write_body_under_sanitizers(tmp_path):
    """no Python-loaded code runs under a sanitizer: the two functions are header-only C++ and get a main() of their own"""
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the driver; it must be here"
    exe = str(tmp_path / "unik_body_roundtrip")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "unikmer_amd", "host"), os.path.join(ROOT, "tests", "unik_body_roundtrip.cpp"), "-o", exe, "-lz"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.returncode, r.stdout, r.stderr)
