"""ukm_fastx against tests/fastx_model.py (pinned to the driver's parse_fastx by tests/test_fastx_cpu.py): bases, record
offsets, header offsets, the bytes consumed and the reason for stopping equal the model's, from host arrays and from device
tensors."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fastx_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "unikmer_amd", "csrc", "ukm_fastx.hip")).read()
T = int(re.search(r"constexpr int FASTX_TILE = (\d+);", _SRC).group(1))   # text bytes per tile
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
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint8): np.uint8}[a.dtype]
    return torch.from_numpy(a.view(signed).copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype) if hasattr(t, "cpu") else np.asarray(t, dtype=dtype)


def results(got):
    b, r, h, consumed, stop = got
    return host(b, np.uint8).tobytes(), host(r, np.uint64).tolist(), host(h, np.uint64).tolist(), consumed, stop


def wanted(text, fastq, last):
    b, r, h, consumed, stop = M.device(text, fastq, last)
    return b, [int(x) for x in r], [int(x) for x in h], consumed, stop


def check(ctx, text, fastq, last, where=("host", "device"), what=""):
    want = wanted(text, fastq, last)
    arr = np.frombuffer(text, dtype=np.uint8)
    for w in where:
        got = results(ctx.fastx(arr if w == "host" else dev(arr), fastq=fastq, last=last))
        for i, nm in enumerate(("bases", "rec_off", "hdr_off", "consumed", "stop")):
            assert got[i] == want[i], (nm, w, fastq, last, what, len(text), got[3:], want[3:])
    return want


def check_all(ctx, text, fastq, where=("device",), what=""):
    return [check(ctx, text, fastq, last, where, what) for last in (True, False)]


BASES = np.frombuffer(b"ACGTacgtNRYKM", dtype=np.uint8)


def seq(n, seed):
    return np.random.default_rng(seed).choice(BASES[:4], n).tobytes()


def fasta(size, width, seed, eol=b"\n", rec_lines=37):
    """FASTA of exactly `size` bytes: records of rec_lines lines of `width` bases (the last record is cut where the size ends)"""
    s = seq(size, seed)
    out, n, i, at = [], 0, 0, 0
    while n < size:
        part = [b">r%d some words" % i + eol] + [s[at + j * width: at + (j + 1) * width] + eol for j in range(rec_lines)]
        at += rec_lines * width
        i += 1
        for p in part:
            out.append(p[: size - n])
            n += len(out[-1])
            if n == size:
                break
    return b"".join(out)


def fastq_groups(n, length, seed, eol=b"\n"):
    s = seq(n * length, seed)
    return [b"@read%d/1" % i + eol + s[i * length:(i + 1) * length] + eol + b"+" + eol + b"I" * length + eol for i in range(n)]


# ---- the corpus the CPU tests pin to the host parser ----------------------------------------------------------------------------
def test_small_corpus_in_both_formats(ctx):
    texts = dict(M.CORPUS_FASTA)
    texts.update(M.CORPUS_FASTQ)
    texts.update(M.FASTQ_DEVIATIONS)
    for name, text in texts.items():
        for fastq in (False, True):
            check_all(ctx, text, fastq, where=("host", "device"), what=name)


def test_golden_genomes(ctx):
    for name, text in M.golden_texts().items():
        (b, r, h, consumed, stop), _ = check_all(ctx, text, False, what=name)
        assert consumed == len(text) and len(h) >= 1 and len(b) > 1000000
        check(ctx, text, False, True, where=("host",), what=name)
        check(ctx, text, True, True, what=name)     # as FASTQ: refused at offset 0


# ---- sizes and placement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [0, 1, T - 1, T, T + 1, 2 * T + 1])
def test_sizes_around_the_tile(ctx, size):
    check_all(ctx, fasta(size, 60, 1), False, where=("host", "device"))
    check_all(ctx, fasta(size, 60, 2, eol=b"\r\n"), False)
    q = b"".join(fastq_groups(size // 300 + 1, 147, 3))[:size]
    check_all(ctx, q, True, where=("host", "device"))
    whole = b"".join(fastq_groups(max(size // 310, 1), 150, 4))
    check_all(ctx, whole, True)


def test_more_tiles_than_the_scan_workgroup_has_threads(ctx):
    text = fasta(257 * T + 3, 60, 5, rec_lines=1501)
    w = check(ctx, text, False, True, where=("host", "device"))
    assert len(w[2]) > 10
    check(ctx, text, False, False, where=("device",))
    # the same bases on one line: a line of more than 256 tiles
    one = b">chromosome\n" + w[0]
    w1 = check_all(ctx, one, False)
    assert w1[0][0] == w[0] and w1[0][1] == [0, len(w[0])] and w1[1][3] == 0
    check_all(ctx, one + b"\n>next\nAC\n", False)


def test_header_longer_than_a_tile(ctx):
    name = b">" + b"x y\tz>" * ((2 * T + 5) // 6)
    name = name[: 2 * T + 4] + b"\n"
    assert len(name) == 2 * T + 5
    check_all(ctx, name + b"ACGT\n" + name + b"GG\n", False, where=("host", "device"))
    check_all(ctx, b">a\nAC\n" + name[:-1], False)
    for d in range(-2, 3):     # the header begins around a tile edge and ends around another
        check_all(ctx, fasta(T + d, 60, 6)[:T + d - 1] + b"\n" + name + b"ACGT\n", False)


def test_placement_on_tile_edges(ctx):
    head = fasta(T - 1, 60, 7)[: T - 2] + b"A"           # T - 1 bytes that end inside a sequence line
    assert len(head) == T - 1
    texts = {
        "lf_last_gt_first": head + b"\n>r\nACGT\n",
        "lf_last_seq_first": head + b"\nACGT\n>r\nAC\n",
        "cr_last_lf_first": head[:-1] + b"A\r\nACGT\r\n",
        "cr_last_no_lf": head[:-1] + b"A\rACGT\n",
        "blanks_across": head[:-3] + b"A \t \t  \t ACGT\n",
        "gt_last_byte": head[:-1] + b"\n>" + b"name\nAC\n",
        "no_lf_in_tile_seq": b">r\n" + seq(3 * T, 8) + b"\n>s\nAC\n",
        "no_lf_in_tile_header": b">" + b"n" * (3 * T) + b"\nACGT\n",
        "empty_lines_across": head + b"\n\n\n\r\n\nACGT\n",
    }
    for name, text in texts.items():
        check_all(ctx, text, False, where=("host", "device"), what=name)
        check(ctx, text[:-1], False, True, where=("device",), what=name)     # no final LF


def test_fastq_reads_across_tiles_and_a_long_read(ctx):
    groups = fastq_groups(3 * T // 310 + 1, 150, 9)
    text = b"".join(groups)
    w = check_all(ctx, text, True, where=("host", "device"))
    assert w[0][3] == len(text) and len(w[0][2]) == len(groups)
    check_all(ctx, text[:-1], True)                       # the last quality line lacks its LF
    check_all(ctx, b"".join(fastq_groups(40, 150, 10, eol=b"\r\n")), True)
    s = seq(2 * T + 1, 11)
    long_read = b"@long\n" + s[:-1] + b"\n+\n" + b"J" * (2 * T) + b"\n"
    assert len(s[:-1] + b"\n") == 2 * T + 1
    w = check_all(ctx, groups[0] + long_read + groups[1], True, where=("host", "device"))
    assert len(w[0][2]) == 3


S150, Q150 = seq(150, 12), b"I" * 150
DEVIANT = {
    "two_line_seq": b"@d\n" + S150[:70] + b"\n" + S150[70:] + b"\n+\n" + Q150 + b"\n",
    "two_line_qual": b"@d\n" + S150 + b"\n+\n" + Q150[:70] + b"\n" + Q150[70:] + b"\n",
    "short_qual": b"@d\n" + S150 + b"\n+\n" + Q150[:-1] + b"\n",
    "blank_in_seq": b"@d\n" + S150[:149] + b" \n+\n" + Q150 + b"\n",
    "empty_between": b"\n@d\n" + S150 + b"\n+\n" + Q150 + b"\n",
    "header_without_at": b"d\n" + S150 + b"\n+\n" + Q150 + b"\n",
    "seq_begins_plus": b"@d\n+" + S150 + b"\n+\n" + Q150 + b"I\n",
    "no_plus_line": b"@d\n" + S150 + b"\n-\n" + Q150 + b"\n",
}


@pytest.mark.parametrize("kind", sorted(DEVIANT))
def test_fastq_deviation_in_the_first_a_middle_and_the_last_group(ctx, kind):
    groups = fastq_groups(3 * T // 310 + 1, 150, 13)
    starts = np.cumsum([0] + [len(g) for g in groups])
    mid = next(i for i in range(len(groups)) if starts[i] < T < starts[i + 1])    # the group that straddles the tile edge
    for g in (0, mid, len(groups) - 1):
        text = b"".join(groups[:g]) + DEVIANT[kind] + b"".join(groups[g + 1:])
        for last in (True, False):
            b, r, h, consumed, stop = check(ctx, text, True, last, where=("host", "device") if g == mid else ("device",), what=kind)
            assert stop == M.STOP_GRAMMAR and consumed == starts[g] and len(h) == g


def test_fastq_trailing_empty_line(ctx):
    text = b"".join(fastq_groups(30, 150, 14)) + b"\n"
    b, r, h, consumed, stop = check(ctx, text, True, True, where=("host", "device"))
    assert stop == M.STOP_GRAMMAR and consumed == len(text) - 1 and len(h) == 30
    assert check(ctx, text, True, False)[4] == M.STOP_TAIL


@pytest.mark.parametrize("fastq", [False, True])
def test_chunked_use(ctx, fastq):
    """the driver's loop: pieces of T + 7 bytes, the unconsumed tail carried in front of the next piece, LAST on the final one"""
    if fastq:
        text = b"".join(fastq_groups(50, 150, 15) + [b"@long\n" + seq(2 * T, 16) + b"\n+\n" + b"J" * (2 * T) + b"\n"] + fastq_groups(20, 99, 17))[:-1]
    else:
        text = fasta(3 * T, 60, 18, eol=b"\r\n", rec_lines=7) + b">long\n" + seq(2 * T + 100, 19) + b"\n>e\n\n>f\nAC GT\n" + fasta(2 * T, 80, 20)
    piece = T + 7
    bases, rec_off, hdr_off, carry, base_at, calls = b"", [0], [], b"", 0, 0
    for at in range(0, len(text), piece):
        buf = carry + text[at: at + piece]
        final = at + piece >= len(text)
        b, r, h, consumed, stop = results(ctx.fastx(dev(np.frombuffer(buf, dtype=np.uint8)), fastq=fastq, last=final))
        calls += 1
        assert stop == (M.STOP_NONE if consumed == len(buf) else M.STOP_TAIL)
        rec_off += [x + len(bases) for x in r[1:]]
        hdr_off += [x + base_at for x in h]
        bases += b
        carry = buf[consumed:]
        base_at += consumed
    assert carry == b"" and base_at == len(text)
    one = results(ctx.fastx(dev(np.frombuffer(text, dtype=np.uint8)), fastq=fastq, last=True))
    assert (bases, rec_off, hdr_off) == one[:3] and one[3:] == (len(text), M.STOP_NONE)
    assert one[:3] == wanted(text, fastq, True)[:3]


# ---- the contract -----------------------------------------------------------------------------------------------------------
def raw(ctx, lib, text, flags, bases, bcap, rec_off, hdr_off, rcap):
    """the entry point on device tensors (or None), capacities as given: (rc, n_bases, n_rec, consumed, stop)"""
    nb, nr, used, stop = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    rc = ctx.L.ukm_fastx(ctx.h, p(text), 0 if text is None else text.numel(), flags, p(bases), bcap, p(rec_off), p(hdr_off), rcap,
                         C.byref(nb), C.byref(nr), C.byref(used), C.byref(stop))
    return rc, nb.value, nr.value, used.value, stop.value


@pytest.mark.parametrize("fastq", [False, True])
def test_size_query_capacity_and_untouched_memory(ctx, lib, fastq):
    import torch
    text = b"".join(fastq_groups(40, 150, 21)) if fastq else fasta(3 * T + 11, 60, 22, rec_lines=5)
    flags = (lib.FASTX_FASTQ if fastq else 0) | lib.FASTX_LAST
    wb, wr, wh, wc, ws = wanted(text, fastq, True)
    nb, nr = len(wb), len(wh)
    dt = dev(np.frombuffer(text, dtype=np.uint8))
    assert raw(ctx, lib, dt, flags, None, 0, None, None, 0) == (lib.ERR_CAPACITY, nb, nr, wc, ws)      # the size query
    slab_b = torch.full((nb + 128,), PAT, dtype=torch.uint8, device="cuda")
    slab_r = torch.full((nr + 17,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
    slab_h = slab_r.clone()
    assert int(slab_r[0].cpu().numpy().view(np.uint64)) == 0xA5A5A5A5A5A5A5A5
    ob, orr, oh = slab_b[64:], slab_r[8:], slab_h[8:]
    for bcap, rcap in ((nb - 1, nr), (nb, nr - 1), (0, nr), (nb, 0)):      # each capacity one short: both needs, nothing written
        assert raw(ctx, lib, dt, flags, ob, bcap, orr, oh, rcap) == (lib.ERR_CAPACITY, nb, nr, wc, ws)
        assert (slab_b == PAT).all() and (slab_r == slab_r[0]).all() and (slab_h == slab_r[0]).all()
    assert raw(ctx, lib, dt, flags, ob, nb, orr, oh, nr) == (lib.OK, nb, nr, wc, ws)
    sb, sr, sh = slab_b.cpu().numpy(), slab_r.cpu().numpy().view(np.uint64), slab_h.cpu().numpy().view(np.uint64)
    assert sb[64: 64 + nb].tobytes() == wb and sr[8: 8 + nr + 1].tolist() == wr and sh[8: 8 + nr].tolist() == wh
    assert (sb[:64] == PAT).all() and (sb[64 + nb:] == PAT).all()
    guard = 0xA5A5A5A5A5A5A5A5
    assert (sr[:8] == guard).all() and (sr[8 + nr + 1:] == guard).all() and (sh[:8] == guard).all() and (sh[8 + nr:] == guard).all()
    # out_hdr_off may be NULL
    slab_r.fill_(0)
    assert raw(ctx, lib, dt, flags, ob, nb, orr, None, nr)[0] == lib.OK
    assert slab_r.cpu().numpy().view(np.uint64)[8: 8 + nr + 1].tolist() == wr
    # a stop in front of the first record writes out_rec_off[0] and nothing else
    slab_r.fill_(-1)
    bad = dev(np.frombuffer(b"@r\nAC GT\n+\nIIIII\n" if fastq else b"xyz\n>r\nAC\n", dtype=np.uint8))
    assert raw(ctx, lib, bad, flags, ob, nb, orr, oh, nr) == (lib.OK, 0, 0, 0, lib.FASTX_STOP_GRAMMAR)
    assert slab_r.cpu().numpy()[7:10].tolist() == [-1, 0, -1]


def test_unknown_flags_and_empty_text(ctx, lib):
    dt = dev(np.frombuffer(b">r\nAC\n", dtype=np.uint8))
    for flags in (4, 8, 1 << 31, 7):
        assert raw(ctx, lib, dt, flags, None, 0, None, None, 0)[0] == lib.ERR_INVALID
    for flags in (0, 1, 2, 3):
        assert raw(ctx, lib, None, flags, None, 0, None, None, 0) == (lib.OK, 0, 0, 0, lib.FASTX_STOP_NONE)


@pytest.mark.parametrize("fastq", [False, True])
def test_every_alignment(ctx, lib, fastq):
    import torch
    text = b"".join(fastq_groups(30, 150, 23)) if fastq else fasta(2 * T + 3, 60, 24, eol=b"\r\n", rec_lines=9)
    flags = (lib.FASTX_FASTQ if fastq else 0) | lib.FASTX_LAST
    wb, wr, wh, wc, ws = wanted(text, fastq, True)
    nb, nr = len(wb), len(wh)
    arr = np.frombuffer(text, dtype=np.uint8)
    for off in range(1, 16):
        tin = torch.zeros(len(arr) + 32, dtype=torch.uint8, device="cuda")
        assert tin.data_ptr() % 16 == 0
        tin[off: off + len(arr)] = dev(arr)
        slab_b = torch.full((nb + 64,), PAT, dtype=torch.uint8, device="cuda")
        slab_r = torch.full((nr + 8,), -1, dtype=torch.int64, device="cuda")
        slab_h = torch.full((nr + 8,), -1, dtype=torch.int64, device="cuda")
        ob, orr, oh = slab_b[16 - off:], slab_r[1 + off % 2:], slab_h[1 + (off + 1) % 2:]      # bytes: every offset; u64: 8-aligned
        assert raw(ctx, lib, tin[off: off + len(arr)], flags, ob, nb, orr, oh, nr) == (lib.OK, nb, nr, wc, ws), off
        sb = slab_b.cpu().numpy()
        assert sb[16 - off: 16 - off + nb].tobytes() == wb and (sb[: 16 - off] == PAT).all() and (sb[16 - off + nb:] == PAT).all(), off
        assert orr[: nr + 1].cpu().numpy().tolist() == wr and oh[:nr].cpu().numpy().tolist() == wh, off
        assert int(orr[nr + 1]) == -1 and int(oh[nr]) == -1 and int(slab_r[off % 2]) == -1 and int(slab_h[(off + 1) % 2]) == -1, off


def test_calls_do_not_depend_on_what_the_workspace_held(ctx):
    fa = fasta(5 * T + 9, 60, 25, rec_lines=11)
    fq = b"".join(fastq_groups(70, 150, 26))
    bad = b"".join(fastq_groups(20, 150, 27)) + DEVIANT["short_qual"] + b"".join(fastq_groups(5, 150, 28))
    for byte in (0x00, 0xFF, 0xAA):
        ctx.set_option("ws_poison", byte)
        try:
            for text, fastq in ((fa, False), (fq, True), (bad, True), (b"\n\nxyz\n>r\nAC\n", False)):
                check_all(ctx, text, fastq, where=("host", "device"), what="poison %#x" % byte)
        finally:
            ctx.set_option("ws_poison", None)


def test_the_outputs_feed_encode_kmers(ctx):
    head = fasta(3 * T + 5, 60, 29, eol=b"\r\n", rec_lines=13)
    text = head[: head.rfind(b"\n") + 1] + b">short\nACGT\n>e\n"      # (cut at a line end: a lone CR would be an illegal base)
    wb, wr, wh, wc, ws = wanted(text, False, True)
    bases, rec_off, hdr_off, consumed, stop = ctx.fastx(dev(np.frombuffer(text, dtype=np.uint8)), last=True)
    got = ctx.encode_kmers(bases, rec_off, 31, canonical=True)
    want = ctx.encode_kmers(np.frombuffer(wb, dtype=np.uint8), np.array(wr, dtype=np.uint64), 31, canonical=True)
    got, want = host(got, np.uint64), host(want, np.uint64)
    assert len(want) == sum(max(0, wr[i + 1] - wr[i] - 30) for i in range(len(wh))) and len(want) > 3 * T * 0.8
    assert np.array_equal(got, want)
