"""ukm_unik_decode / ukm_unik_encode against tests/unik_model.py (the Reader and Writer of host/unik.hpp restated; pinned to
them by tests/test_unik_codec_cpu.py): decode equals the model record for record, encode equals it byte for byte, from
host arrays and from device tensors, in every case."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unik_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

# from the kernels' source (unikmer_amd/csrc/ukm_unik.hip)
TILE = 2048          # DEC_TILE: body bytes per tile of the sorted decode
SCAN_GROUP = 256     # SCAN_GROUP: tiles one scan workgroup composes
ENC_PAIRS = 1024     # ENC_PAIRS: pairs per tile of the sorted encode
FIX_RECS = 1024      # FIX_RECS: records per tile of the fixed-size layouts

S, T, CP = M.SORTED, M.INCLUDE_TAXID, M.COMPACT
TOP = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")


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


def as_arrays(codes, tax):
    return np.array([int(c) for c in codes], dtype=np.uint64), (None if tax is None else np.array([int(t) for t in tax], dtype=np.uint32))


def check_decode(ctx, body, k, flags, tb, want):
    """want = (codes, taxids or None) of the model; host and device"""
    b = np.frombuffer(body, dtype=np.uint8)
    for arr in (b, dev(b)):
        keys, tax = ctx.unik_decode(arr, k, flags, tb)
        assert np.array_equal(host(keys, np.uint64), want[0])
        assert (tax is None) == (want[1] is None)
        if tax is not None:
            assert np.array_equal(host(tax, np.uint32), want[1])


def check_encode(ctx, codes, tax, k, flags, tb, want):
    codes, tax = as_arrays(codes, tax)
    for kk, tt in ((codes, tax), (dev(codes), dev(tax))):
        out = ctx.unik_encode(kk, k, flags, taxids=tt, taxid_bytes=tb)
        assert host(out, np.uint8).tobytes() == want


def check(ctx, codes, tax, k, flags, tb):
    """one case: the model encodes and decodes, the device must agree with both"""
    body = M.encode(codes, tax, k, flags, tb)
    want = M.decode(body, k, flags, tb)
    check_decode(ctx, body, k, flags, tb, want)
    check_encode(ctx, codes, tax if flags & T else None, k, flags, tb, body)
    return body, want


# ---- 1. smallest bodies -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codes", [[], [0], [5], [0, 0], [3, 9], [0, 0, 0], [1, 2, 3], [7, 7, 7, 7], [TOP - 1, TOP], [TOP, TOP, TOP],
                                   [0, TOP - 1, TOP]])
def test_smallest_bodies(ctx, codes):
    tax = [0xA1B2C3D4 + i for i in range(len(codes))]
    for flags, tb in ((S, 0), (S | T, 4), (S | T, 1), (0, 0), (T, 3), (CP, 0), (CP | T, 2)):
        check(ctx, codes, tax, 32, flags, tb)


# ---- 2. every control byte --------------------------------------------------------------------------------------------------
def control_byte_codes():
    """all 64 (l0, l1), each with deltas at the low and at the high end of its byte length; a single (ctrl = 128, which
    resets prev) in front of every pair keeps the codes below 2^64"""
    codes = []
    for l0 in range(1, 9):
        for l1 in range(1, 9):
            lo0, lo1 = (1 << (8 * (l0 - 1))) if l0 > 1 else 0, (1 << (8 * (l1 - 1))) if l1 > 1 else 0
            hi0, hi1 = (1 << (8 * l0)) - 1, (1 << (8 * l1)) - 1
            high = (hi0, hi1) if hi0 + hi1 <= TOP else ((hi0, 0) if l1 == 1 else (hi0 >> 1, hi1 >> 1))
            for d0, d1 in ((lo0, lo1), high):
                codes.append([d0, d0 + d1])
    return codes


@pytest.mark.parametrize("tb", [0, 1, 2, 3, 4])
def test_every_control_byte(ctx, tb):
    rng = np.random.default_rng(tb)
    flags = S | (T if tb else 0)
    body = bytearray()
    codes, tax = [], []
    for c0, c1 in control_byte_codes():
        t = [int(x) | 0x81000000 for x in rng.integers(0, 1 << 32, 2)]        # high bytes non-zero
        part = M.encode([c0, c1], t, 31, flags, tb)                            # prev = 0: the deltas are the codes'
        assert part[0] < 128
        # each pair alone, then all of them in one body behind resetting singles
        check(ctx, [c0, c1], t, 31, flags, tb)
        body += M.encode([0], [t[0]], 31, flags, tb) + part
        codes += [0, c0, c1]
        tax += [t[0]] + t
    want = M.decode(bytes(body), 31, flags, tb)
    assert [int(x) for x in want[0]] == codes
    check_decode(ctx, bytes(body), 31, flags, tb, want)


# ---- 3. tile boundaries -----------------------------------------------------------------------------------------------------
def fill_to(nbytes):
    """record lengths (pairs with 4-byte taxids: 11..25 bytes) that add up to nbytes >= 11: narrow ones, the last absorbs"""
    assert nbytes >= 11
    return [11] * (nbytes // 11 - 1) + [11 + nbytes % 11]


def body_of_lengths(lengths, seed):
    """a sorted body with 4-byte taxids whose pair i takes lengths[i] bytes"""
    rng = np.random.default_rng(seed)
    codes, prev = [], 0
    for ln in lengths:
        extra = ln - 11
        l0 = 1 + (extra // 2 if ln < 25 else 7)
        l1 = 1 + extra - (l0 - 1)
        d0 = (1 << (8 * (l0 - 1))) if l0 > 1 else int(rng.integers(0, 256))
        d1 = (1 << (8 * (l1 - 1))) if l1 > 1 else int(rng.integers(0, 256))
        codes += [prev + d0, prev + d0 + d1]
        prev += d0 + d1
    assert prev <= TOP
    tax = [int(x) for x in rng.integers(0, 1 << 32, len(codes))]
    body = M.encode(codes, tax, 31, S | T, 4)
    assert len(body) == sum(lengths)
    return codes, tax, body


@pytest.mark.parametrize("j", range(25))
def test_record_starts_at_every_offset_behind_a_tile_boundary(ctx, j):
    """two tiles exactly: a 25-byte record from TILE + j - 25 on (it straddles the boundary, or ends at it for j = 0), the
    next record starts at offset j of the second tile; narrow records in front, wide ones behind"""
    lengths = fill_to(TILE + j - 25) + [25] + [25] * 3 + fill_to(2 * TILE - (TILE + j) - 75)
    codes, tax, body = body_of_lengths(lengths, j)
    assert len(body) == 2 * TILE
    starts = np.cumsum([0] + lengths)
    assert TILE + j in starts and TILE + j - 25 in starts
    check(ctx, codes, tax, 31, S | T, 4)


@pytest.mark.parametrize("nbytes", [TILE - 1, TILE, TILE + 1, TILE + 24, TILE + 25, 2 * TILE - 1, 2 * TILE + 1])
def test_bodies_around_the_tile_size(ctx, nbytes):
    for tail in (11, 25):     # the last record narrow or wide
        lengths = fill_to(nbytes - tail) + [tail]
        codes, tax, body = body_of_lengths(lengths, nbytes)
        assert len(body) == nbytes
        check(ctx, codes, tax, 31, S | T, 4)


# ---- 4. chains that never merge ---------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def never_merging(n):
    codes = [64 * j for j in range(1, n + 1) for _ in (0, 1)]
    body = M.encode(codes, None, 31, S, 0)
    assert set(body) == {0x00, 0x40} and len(body) == 3 * n
    return codes, body, M.decode(body, 31, S, 0)


def test_never_merging_model_has_three_disjoint_chains():
    """parsed from offsets 0, 1 and 2 the body gives three chains that share no position and decode to different codes"""
    n = 2000
    _, body, _ = never_merging(n)
    seen = []
    for e in (0, 1, 2):
        pos, at = e, set()
        while pos < len(body):
            at.add(pos)
            ctrl = body[pos]
            assert ctrl < 128
            pos += 1 + ((ctrl >> 3) & 7) + 1 + (ctrl & 7) + 1
        seen.append(at)
    assert not (seen[0] & seen[1]) and not (seen[0] & seen[2]) and not (seen[1] & seen[2])
    assert all(len(s) >= n - 1 for s in seen)
    firsts = [(body[e + 1], body[e + 1] + body[e + 2]) for e in (0, 1, 2)]     # every record here is ctrl, d0, d1 of one byte each
    assert firsts == [(64, 64), (0, 0), (0, 64)]


@pytest.mark.parametrize("n", [2100, (SCAN_GROUP * TILE) // 3 + 1000])
def test_chains_that_never_merge(ctx, n):
    """3 n bytes: at least 3 tiles, then more tiles than one scan workgroup covers; TILE is no multiple of the 3-byte
    period, so the entry offset differs from tile to tile"""
    codes, body, want = never_merging(n)
    assert len(body) > (3 * TILE if n < 10000 else SCAN_GROUP * TILE) and TILE % 3 != 0
    check_decode(ctx, body, 31, S, 0, want)
    check_encode(ctx, codes, None, 31, S, 0, body)


# ---- 5. random sets ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def random_case(which):
    rng = np.random.default_rng(77)
    if which == "k31":
        codes = np.sort(rng.integers(0, 1 << 62, 200_000, dtype=np.uint64))
        tax, k, flags, tb = None, 31, S, 0
    elif which == "k11":
        codes = np.sort(rng.integers(0, 1 << 22, 200_000, dtype=np.uint64))       # dense: duplicates included
        assert len(np.unique(codes)) < len(codes)
        tax, k, flags, tb = rng.integers(0, 1 << 32, len(codes), dtype=np.uint64).astype(np.uint32), 11, S | T, 4
    else:
        layout, k = which
        codes = rng.integers(0, 1 << min(2 * k, 63), 100_003, dtype=np.uint64) * np.uint64(2 if k == 32 else 1)
        tax = rng.integers(0, 1 << 32, len(codes), dtype=np.uint64).astype(np.uint32)
        flags, tb = (CP if layout == "compact" else 0) | T, 3
    codes_l = [int(c) for c in codes]
    tax_l = None if tax is None else [int(t) for t in tax]
    body = M.encode(codes_l, tax_l, k, flags, tb)
    return codes_l, tax_l, k, flags, tb, body, M.decode(body, k, flags, tb)


@pytest.mark.parametrize("which", ["k31", "k11"] + [(lay, k) for lay in ("unsorted", "compact") for k in (11, 21, 32)])
def test_random_sets(ctx, which):
    codes, tax, k, flags, tb, body, want = random_case(which)
    if which == "k31":
        assert 6.5 < len(body) / (len(codes) / 2) < 13.5     # a pair is 1 + two deltas of 5-6 bytes
    check_decode(ctx, body, k, flags, tb, want)
    check_encode(ctx, codes, tax, k, flags, tb, body)


# ---- 6. more than one scan level --------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def two_level_case():
    """block "k11" of the random sets, tiled with a growing base where it is too short, cut to the smallest body that needs
    more than SCAN_GROUP tiles (a pair of it takes 11 bytes)"""
    codes, tax, k, flags, tb, body, _ = random_case("k11")
    reps = (SCAN_GROUP * TILE) // len(body) + 1
    all_codes, all_tax = [], []
    for r in range(reps):
        all_codes += [c + (r << 22) for c in codes]
        all_tax += tax
    n = 2 * ((SCAN_GROUP * TILE) // 11 + 1)
    all_codes, all_tax = all_codes[:n], all_tax[:n]
    body = M.encode(all_codes, all_tax, k, flags, tb)
    assert SCAN_GROUP * TILE < len(body) <= SCAN_GROUP * TILE + 11
    return all_codes, all_tax, k, flags, tb, body, M.decode(body, k, flags, tb)


def test_more_than_one_scan_level(ctx):
    codes, tax, k, flags, tb, body, want = two_level_case()
    check_decode(ctx, body, k, flags, tb, want)
    check_encode(ctx, codes, tax, k, flags, tb, body)


# ---- 7. singles in the middle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tb", [0, 2])
def test_singles_in_the_middle(ctx, tb):
    rng = np.random.default_rng(3)
    flags = S | (T if tb else 0)
    a = [int(x) for x in np.sort(rng.integers(0, 1 << 40, 2001, dtype=np.uint64))]
    b = [int(x) for x in np.sort(rng.integers(0, 1 << 30, 1501, dtype=np.uint64))]
    ta, tb_ = [int(x) for x in rng.integers(0, 1 << 32, len(a))], [int(x) for x in rng.integers(0, 1 << 32, len(b))]
    body = M.encode(a, ta, 31, flags, tb) + M.encode(b, tb_, 31, flags, tb)
    want = M.decode(body, 31, flags, tb)
    # a's trailing single set prev = a[-1]: b's first delta counts from there, and b's own single stands in the middle too
    assert [int(x) for x in want[0]] == a + [x + a[-1] for x in b[:-1]] + [b[-1]]
    check_decode(ctx, body, 31, flags, tb, want)
    # singles only: every record a full code, in any order
    singles = [int(x) for x in rng.integers(0, 1 << 64, 1000, dtype=np.uint64)]
    ts = [int(x) for x in rng.integers(0, 1 << 32, len(singles))]
    body = b"".join(M.encode([c], [t], 31, flags, tb) for c, t in zip(singles, ts))
    want = M.decode(body, 31, flags, tb)
    assert [int(x) for x in want[0]] == singles and len(body) == len(singles) * (9 + tb) > TILE
    check_decode(ctx, body, 31, flags, tb, want)


# ---- 8. malformed input -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,tb", [(S | T, 2), (T, 2), (S, 0), (CP | T, 1)])
def test_every_proper_prefix_decodes_or_fails_like_the_model(ctx, lib, flags, tb):
    """no word outside the body is loaded (ukm_unik.hip: load_image), so no prefix can fault"""
    codes = [3, 300, 70000, 1 << 40, (1 << 40) + 5]
    tax = [0x0101, 0x0202, 0x0303, 0x0404, 0x0505]
    body = M.encode(codes, tax, 13, flags, tb)
    slab = dev(np.frombuffer(body, dtype=np.uint8))
    for cut in range(len(body)):
        try:
            want = M.decode(body[:cut], 13, flags, tb)
        except ValueError:
            want = None
        for arr in (np.frombuffer(body[:cut], dtype=np.uint8), slab[:cut]):
            if want is None:
                with pytest.raises(lib.FormatError):
                    ctx.unik_decode(arr, 13, flags, tb)
            else:
                keys, t = ctx.unik_decode(arr, 13, flags, tb)
                assert np.array_equal(host(keys, np.uint64), want[0])
                assert (t is None and want[1] is None) or np.array_equal(host(t, np.uint32), want[1])


# ---- 9. neighbours have no influence ----------------------------------------------------------------------------------------
def test_neighbours_have_no_influence(ctx):
    import torch
    rng = np.random.default_rng(9)
    tb, flags = 3, S | T
    codes = [int(x) for x in np.sort(rng.integers(0, 1 << 44, 1501, dtype=np.uint64))]
    tax = [int(x) for x in rng.integers(0, 1 << 24, len(codes))]
    body = M.encode(codes, tax, 31, flags, tb)
    want = M.decode(body, 31, flags, tb)
    n, nb = len(codes), len(body)
    assert nb > 2 * TILE
    dk, dt = dev(np.array(codes, dtype=np.uint64)), dev(np.array(tax, dtype=np.uint32))
    G = 64
    for fill in (0x00, 0xFF):
        for off in range(16):
            # decode: the body packed at address offset `off`, outputs inside guarded slabs of exactly n records
            slab = torch.full((nb + 64,), fill, dtype=torch.uint8, device="cuda")
            assert slab.data_ptr() % 16 == 0
            slab[off:off + nb] = torch.from_numpy(np.frombuffer(body, dtype=np.uint8).copy()).cuda()
            before = slab.clone()
            ks = torch.full((n + 2 * G,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
            ts = torch.full((n + 2 * G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            keys, t = ctx.unik_decode(slab[off:off + nb], 31, flags, tb, out=ks[G:G + n], out_taxids=ts[G:G + n])
            assert np.array_equal(host(keys, np.uint64), want[0]) and np.array_equal(host(t, np.uint32), want[1])
            assert torch.equal(slab, before)
            for g, sent in ((ks, -0x5A5A5A5A5A5A5A5B), (ts, 0x5A5A5A5A)):
                assert bool((g[:G] == sent).all()) and bool((g[G + n:] == sent).all())
            # encode: out_bytes at address offset `off`, out_cap exact
            oslab = torch.full((nb + 64,), fill, dtype=torch.uint8, device="cuda")
            out = ctx.unik_encode(dk, 31, flags, taxids=dt, taxid_bytes=tb, out=oslab[off:off + nb])
            assert out.cpu().numpy().tobytes() == body
            assert bool((oslab[:off] == fill).all()) and bool((oslab[off + nb:] == fill).all())


# ---- 10. capacity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,tb", [(S | T, 4), (S, 0), (T, 2), (CP, 0)])
def test_capacity(ctx, lib, flags, tb):
    rng = np.random.default_rng(10)
    n = 3001
    codes = np.sort(rng.integers(0, 1 << 22, n, dtype=np.uint64))
    tax = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    body = M.encode(codes, tax, 11, flags, tb)
    want = M.decode(body, 11, flags, tb)
    b = np.frombuffer(body, dtype=np.uint8)
    m = C.c_uint64()
    for bb in (b, dev(b)):
        p = bb.ctypes.data if isinstance(bb, np.ndarray) else bb.data_ptr()
        assert ctx.L.ukm_unik_decode(ctx.h, p, len(body), 11, flags, tb, None, None, 0, C.byref(m)) == lib.ERR_CAPACITY
        assert m.value == n
        with pytest.raises(lib.CapacityError) as e:
            ctx.unik_decode(bb, 11, flags, tb, out=np.empty(n - 1, dtype=np.uint64), out_taxids=np.empty(n - 1, dtype=np.uint32) if tb else None)
        assert e.value.needed == n
        keys, t = ctx.unik_decode(bb, 11, flags, tb, out=np.empty(n, dtype=np.uint64), out_taxids=np.empty(n, dtype=np.uint32) if tb else None)
        assert np.array_equal(keys, want[0]) and (not tb or np.array_equal(t, want[1]))
    txs = tax if tb else None
    assert ctx.L.ukm_unik_encode(ctx.h, codes.ctypes.data, tax.ctypes.data if tb else None, n, 11, flags, tb, None, 0, C.byref(m)) == lib.ERR_CAPACITY
    assert m.value == len(body)
    with pytest.raises(lib.CapacityError) as e:
        ctx.unik_encode(codes, 11, flags, taxids=txs, taxid_bytes=tb, out=np.empty(len(body) - 1, dtype=np.uint8))
    assert e.value.needed == len(body)
    guard = np.full(len(body) + 64, 0xA5, dtype=np.uint8)
    out = ctx.unik_encode(codes, 11, flags, taxids=txs, taxid_bytes=tb, out=guard[:len(body)])
    assert out.tobytes() == body and (guard[len(body):] == 0xA5).all()
    # an empty result: UKM_OK with *n_out == 0
    assert ctx.L.ukm_unik_decode(ctx.h, None, 0, 11, flags, tb, None, None, 0, C.byref(m)) == lib.OK and m.value == 0
    assert ctx.L.ukm_unik_encode(ctx.h, None, None, 0, 11, flags, tb, None, 0, C.byref(m)) == lib.OK and m.value == 0


def test_argument_errors(ctx, lib):
    m = C.c_uint64()
    b = np.zeros(8, dtype=np.uint8)
    for tb in (0, 5):
        assert ctx.L.ukm_unik_decode(ctx.h, b.ctypes.data, 8, 31, S | T, tb, None, None, 0, C.byref(m)) == lib.ERR_INVALID
    for k in (0, 33):
        assert ctx.L.ukm_unik_decode(ctx.h, b.ctypes.data, 8, k, CP, 0, None, None, 0, C.byref(m)) == lib.ERR_K
    assert ctx.L.ukm_unik_decode(ctx.h, b.ctypes.data, 8, 0, 0, 9, None, None, 0, C.byref(m)) == lib.ERR_CAPACITY and m.value == 1


# ---- 11. workspace ----------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_workspace(ctx, lib):
    codes, tax, k, flags, tb, body, want = random_case("k11")
    codes, tax = as_arrays(codes[:50_001], tax[:50_001])
    body = M.encode(codes, tax, k, flags, tb)
    want = M.decode(body, k, flags, tb)
    b = np.frombuffer(body, dtype=np.uint8)

    def both(c):
        keys, t = c.unik_decode(b, k, flags, tb)
        assert np.array_equal(keys, want[0]) and np.array_equal(t, want[1])
        assert c.unik_encode(codes, k, flags, taxids=tax, taxid_bytes=tb).tobytes() == body

    fresh = lib.Context(0)
    both(fresh)
    fresh.trim()
    both(fresh)
    fresh.sort_u64(np.random.default_rng(1).integers(0, 1 << 64, 1_000_000, dtype=np.uint64))
    both(fresh)
    for byte in (0x00, 0xFF, 0xA5):
        fresh.set_option("ws_poison", byte)
        both(fresh)
    fresh.set_option("ws_poison", None)
    fresh.close()


# ---- 12. unsorted encode ----------------------------------------------------------------------------------------------------
def test_unsorted_encode(ctx, lib):
    n = 2 * ENC_PAIRS + 10
    base = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(1000)
    bad = {"inside a pair": (11, base[10] - np.uint64(1)),                               # second of pair 5 below its first
           "between pairs": (12, base[11] - np.uint64(1)),                               # first of pair 6 below the previous pair's second
           "across the encode tile boundary": (2 * ENC_PAIRS, base[2 * ENC_PAIRS - 1] - np.uint64(1))}
    for what, (i, v) in bad.items():
        c = base.copy()
        c[i] = v
        for arr in (c, dev(c)):
            with pytest.raises(lib.UnsortedError):
                ctx.unik_encode(arr, 31, S)
        with pytest.raises(ValueError):
            M.encode(c, None, 31, S, 0)
        out = ctx.unik_encode(c, 31, 0)                                         # the same array without SORTED
        assert out.tobytes() == M.encode(c, None, 31, 0, 0), what
    # equal codes are fine, and the trailing single of an odd count is not looked at (Writer::flush)
    c = np.array([5, 5, 5, 5, 1], dtype=np.uint64)
    assert ctx.unik_encode(c, 31, S).tobytes() == M.encode(c, None, 31, S, 0)


# ---- 13. -I -----------------------------------------------------------------------------------------------------------------
def test_decode_without_taxid_output(ctx):
    codes, tax, k, flags, tb, body, want = random_case("k11")
    b = np.frombuffer(body, dtype=np.uint8)
    for arr in (b, dev(b)):
        keys, t = ctx.unik_decode(arr, k, flags, tb, with_taxids=False)
        assert t is None and np.array_equal(host(keys, np.uint64), want[0])
    codes, tax, k, flags, tb, body, want = random_case(("unsorted", 21))
    keys, t = ctx.unik_decode(np.frombuffer(body, dtype=np.uint8), k, flags, tb, with_taxids=False)
    assert t is None and np.array_equal(keys, want[0])


# ---- 14. unikfile -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compress", [True, False])
def test_unikfile_round_trip(ctx, tmp_path, compress):
    from unikmer_amd import unikfile
    rng = np.random.default_rng(14)
    codes = np.sort(rng.integers(0, 1 << 42, 5001, dtype=np.uint64))
    tax = rng.integers(1, 1 << 24, len(codes), dtype=np.uint64).astype(np.uint32)
    path = str(tmp_path / "f.unik")
    hdr = {"k": 21, "flag": S | T | M.CANONICAL, "taxid_bytes": 3}
    unikfile.save(ctx, path, hdr, codes, tax, compress=compress)
    raw = open(path, "rb").read()
    assert (raw[:2] == b"\x1f\x8b") == compress
    if not compress:
        assert raw == M.header(21, S | T | M.CANONICAL, number=len(codes), tb=3) + M.encode(codes, tax, 21, S | T, 3)
    h = unikfile.read_header(path)
    assert (h["k"], h["flag"], h["taxid_bytes"], h["number"]) == (21, S | T | M.CANONICAL, 3, len(codes))
    for device in (True, False):
        h2, keys, t = unikfile.load(ctx, path, device=device)
        assert h2 == h and np.array_equal(host(keys, np.uint64), codes) and np.array_equal(host(t, np.uint32), tax)
    _, keys, t = unikfile.load(ctx, path, device=False, ignore_taxid=True)
    assert t is None and np.array_equal(keys, codes)
    p = subprocess.run([BIN, "view", "-N", path], capture_output=True)
    assert p.returncode == 0 and [int(x) for x in p.stdout.split()] == [int(c) for c in codes]
    p = subprocess.run([BIN, "view", "-T", path], capture_output=True)
    assert p.returncode == 0 and [int(x) for x in p.stdout.split()] == [int(x) for x in tax]
