"""The FASTA/Q reader without a device: tests/fastx_model.py (the restatement the GPU tests compare ukm_fastx with) against
the driver's own parser (unikmer_amd/host/seqtext.hpp: parse_fastx), which runs in a stand-alone program under the address and
undefined-behaviour sanitizers (tests/fastx_units.cpp; nothing is loaded into Python); the handover property the driver relies
on; the new overload of parse_fastx; and the new symbol."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fastx_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def corpus():
    """(name, text) of every corpus text, the deviations and the golden genomes included"""
    out = [("fa:" + k, v) for k, v in M.CORPUS_FASTA.items()]
    out += [("fq:" + k, v) for k, v in M.CORPUS_FASTQ.items()]
    out += [("dev:" + k, v) for k, v in M.FASTQ_DEVIATIONS.items()]
    out += [("golden:" + k, v) for k, v in M.golden_texts().items()]
    return out


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the driver; it must be here"
    d = tmp_path_factory.mktemp("fastx_units")
    exe = str(d / "fastx_units")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "unikmer_amd", "host"), os.path.join(ROOT, "tests", "fastx_units.cpp"), "-o", exe, "-lz"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return exe, d


def model_text(text):
    """parse() in the form fastx_units writes"""
    try:
        bases, rec_off, names = M.parse(text)
    except M.HostError as e:
        return ("ERR", str(e))
    o = [int(x) for x in rec_off]
    return b"".join(nm + b"\n" + bases[o[i]:o[i + 1]] + b"\n" for i, nm in enumerate(names))


def test_model_equals_host_parser(units):
    exe, d = units
    texts = corpus()
    work = d / "parse"
    work.mkdir()
    for i, (_, t) in enumerate(texts):
        (work / ("%d.in" % i)).write_bytes(t)
    r = subprocess.run([exe, "parse", str(work), str(len(texts))], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.returncode, r.stdout, r.stderr[-2000:])
    died = 0
    for i, (name, t) in enumerate(texts):
        got = (work / ("%d.out" % i)).read_bytes()
        want = model_text(t)
        if isinstance(want, tuple):
            died += 1
            want = ("ERR %s %s\n" % (want[1], work / ("%d.in" % i))).encode()
        assert got == want, name
    assert died >= 5   # the texts the host dies on are part of the corpus


def test_parse_fastx_overload_at_every_split(units):
    exe, d = units
    work = d / "split"
    work.mkdir()
    files = []
    for name, t in (("a.fa", M.CORPUS_FASTA["crlf"]), ("b.fa", M.CORPUS_FASTA["blanks_in_seq"] + b">r3\nAC\r"),
                    ("c.fq", M.CORPUS_FASTQ["crlf"] + M.FASTQ_DEVIATIONS["two_line_seq"])):
        (work / name).write_bytes(t)
        files.append(str(work / name))
    r = subprocess.run([exe, "split", str(work)] + files, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.returncode, r.stdout, r.stderr[-2000:])


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("last", [True, False])
def test_handover(last):
    """what the device takes plus the host parser on the rest, in the format already decided, is the host parser on the whole"""
    for name, text in corpus():
        fastq = M.is_fastq(text)
        bases, rec_off, hdr_off, consumed, stop = M.device(text, fastq, last)
        assert 0 <= consumed <= len(text) and len(rec_off) == len(hdr_off) + 1 and int(rec_off[-1]) == len(bases), name
        assert all(text[int(h):int(h) + 1] == (b"@" if fastq else b">") for h in hdr_off), name
        assert (stop == M.STOP_NONE) == (consumed == len(text)) or not last, name
        if not last and stop == M.STOP_NONE:
            assert consumed == len(text), name
        try:
            want = M.parse(text, fastq)
        except M.HostError as e:
            want = str(e)
        try:
            rb, ro, rn = M.parse(text[consumed:], fastq)
            names = [text[int(h) + 1:].split(b"\n", 1)[0] for h in hdr_off]
            names = [nm[:-1] if nm.endswith(b"\r") and text[int(h) + 1 + len(nm):int(h) + 2 + len(nm)] == b"\n" else nm
                     for nm, h in zip(names, hdr_off)]
            got = (bases + rb, np.concatenate([rec_off, ro[1:] + rec_off[-1]]), names + rn)
        except M.HostError as e:
            got = str(e)
        if isinstance(want, str) or isinstance(got, str):
            assert got == want, name
        else:
            assert same(got, want), name


@pytest.mark.parametrize("last", [True, False])
def test_deviations_stop_at_their_group(last):
    for name, text in M.FASTQ_DEVIATIONS.items():
        bases, rec_off, hdr_off, consumed, stop = M.device(text, True, last)
        # (one exception: without LAST the lone empty line at the end is a group that lacks three lines -- a tail, as the
        # rule for texts with more behind them says; the call that ends the input refuses it)
        assert stop == (M.STOP_TAIL if name == "trailing_empty" and not last else M.STOP_GRAMMAR), name
        assert len(hdr_off) == 1 and consumed == len(b"@r1\nACGT\n+\nIIII\n") or name in ("short_qual", "blank_in_seq"), name
        if name in ("short_qual", "blank_in_seq"):
            assert consumed == 0 and len(hdr_off) == 0, name
    for name in ("garbage_first", "garbage_after_empty", "blank_line_first", "cr_only_first"):
        bases, rec_off, hdr_off, consumed, stop = M.device(M.CORPUS_FASTA[name], False, last)
        assert stop == M.STOP_GRAMMAR and len(hdr_off) == 0 and bases == b"", name
        assert consumed == {"garbage_after_empty": 2}.get(name, 0), name


def test_symbol_is_declared_and_exported():
    from unikmer_amd import lib
    assert "ukm_fastx" in lib.SYMBOLS
    from unikmer_amd import build
    so = build.build()
    tool = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    nm = subprocess.run([tool, "-D", "--defined-only", so], capture_output=True, text=True)
    assert nm.returncode == 0, nm.stderr
    assert any(line.split()[-1] == "ukm_fastx" for line in nm.stdout.splitlines() if line.strip())
    with open(os.path.join(ROOT, "include", "unikmer_hip.h")) as f:
        assert "int ukm_fastx(" in f.read()
