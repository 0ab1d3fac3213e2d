"""`unikmer count` with its input parsed on the device (UNIKMER_DEVICE_FASTX=1: raw chunks through ukm_fastx into the encode
kernels, what is outside the device's grammar handed to parse_fastx from the byte ukm_fastx names) against the host parser
(UNIKMER_HOST_FASTX=1): the same .unik files byte for byte, the same messages, and UNIKMER_FASTX_REPORT=1 says which path
carried each input."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")
SWITCHES = ("UNIKMER_DEVICE_FASTX", "UNIKMER_HOST_FASTX", "UNIKMER_FASTX_REPORT", "UNIKMER_CHUNK_MB")
DEVICE = {"UNIKMER_DEVICE_FASTX": "1", "UNIKMER_FASTX_REPORT": "1"}
HOST = {"UNIKMER_HOST_FASTX": "1", "UNIKMER_FASTX_REPORT": "1"}
GENOMES = sorted(f for f in os.listdir(GOLDEN) if f.endswith(".fasta.gz"))


def run(env_add, *args, ok=True):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_add)
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, env=env)
    if ok:
        assert p.returncode == 0, (args, p.stderr.decode(errors="replace"))
    return p


def report(p):
    return [ln for ln in p.stderr.decode(errors="replace").splitlines() if ln.startswith("fastx: ")]


def others(p):
    return [ln for ln in p.stderr.decode(errors="replace").splitlines() if not ln.startswith("fastx: ")]


def both(tmp_path, args, files, extra=None, ok=True):
    """count on `files` both ways: the two results, whose outputs and messages (the report aside) must be equal"""
    outs = []
    for how, env in (("device", DEVICE), ("host", HOST)):
        e = dict(env)
        e.update(extra or {})
        out = str(tmp_path / ("out_" + how))
        p = run(e, "count", *args, *files, "-o", out, ok=ok)
        outs.append((p, out + ".unik"))
    (pd, fd), (ph, fh) = outs
    assert pd.returncode == ph.returncode and others(pd) == others(ph)
    if pd.returncode == 0:
        assert open(fd, "rb").read() == open(fh, "rb").read()
        assert os.path.getsize(fd) > 60
    for ln, f in zip(report(ph), files):
        assert ln == "fastx: %s: host (not asked for)" % f
    return pd, ph


def seq(n, seed):
    return np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes()


def fastq(n, length, seed):
    s = seq(n * length, seed)
    return b"".join(b"@r%d\n" % i + s[i * length:(i + 1) * length] + b"\n+\n" + b"I" * length + b"\n" for i in range(n))


def on_device(p, files, chunks=None):
    rep = report(p)
    assert len(rep) == len(files)
    for ln, f in zip(rep, files):
        m = re.fullmatch(r"fastx: %s: device, (\d+) chunk\(s\)" % re.escape(str(f)), ln)
        assert m, ln
        if chunks is not None:
            assert int(m.group(1)) >= chunks, ln


@pytest.mark.parametrize("genome", GENOMES)
def test_golden_genomes(tmp_path, genome):
    f = os.path.join(GOLDEN, genome)
    pd, _ = both(tmp_path, ["-k", 31, "-K", "-s"], [f], extra={"UNIKMER_CHUNK_MB": "1"})
    on_device(pd, [f], chunks=2)


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastx_cli")
    files = {}
    # CRLF FASTA with blanks, empty lines and empty records, 2.5 MB: under UNIKMER_CHUNK_MB=1 chunk edges fall inside records
    s, out, at = seq(2500000, 1), [], 0
    i = 0
    while at < len(s):
        n = int(200 + (i * 7919) % 90000)
        out.append(b">rec%d words\r\n" % i)
        for j in range(at, min(at + n, len(s)), 70):
            out.append(s[j: min(j + 35, at + n)] + b" \t" + s[j + 35: min(j + 70, at + n)] + b"\r\n")
            if (j // 70) % 50 == 0:
                out.append(b"\r\n")
        at += n
        i += 1
        if i % 9 == 0:
            out.append(b">empty%d\r\n" % i)
    files["crlf"] = b"".join(out)
    files["long"] = b">short\nACGTACGTACGTACGTACGTACGTACGTACGTACGT\n>one record longer than a chunk\n" + b"\n".join(
        s[j: j + 80] for j in range(0, 2300000, 80)) + b"\n>after\n" + s[:500] + b"\n"
    files["fastq"] = fastq(9000, 150, 2)
    files["fasta_small"] = b">a\n" + s[:3000] + b"\n>b\n" + s[5000:5100] + b"\n"
    files["multiline_fastq"] = fastq(4000, 150, 3) + b"@m\n" + s[:80] + b"\n" + s[80:160] + b"\n+\n" + b"I" * 80 + b"\n" + b"I" * 80 + b"\n" + fastq(4000, 120, 4)
    files["trailing_empty_fastq"] = fastq(100, 150, 5) + b"\n"
    files["garbage"] = b"\n\nACGT garbage\n>a\n" + s[:3000] + b"\n"
    files["bad_fastq"] = fastq(50, 150, 6) + b"r\nACGT\n+\nIIII\n"
    paths = {}
    for k, v in files.items():
        paths[k] = str(d / (k + (".fq" if "fastq" in k else ".fa")))
        with open(paths[k], "wb") as fh:
            fh.write(v)
    paths["fastq_gz"] = str(d / "reads.fq.gz")
    with gzip.open(paths["fastq_gz"], "wb", compresslevel=1) as fh:
        fh.write(files["fastq"])
    return paths


def test_chunk_edges_inside_records(tmp_path, texts):
    pd, _ = both(tmp_path, ["-k", 31, "-K", "-s"], [texts["crlf"]], extra={"UNIKMER_CHUNK_MB": "1"})
    on_device(pd, [texts["crlf"]], chunks=3)


def test_a_record_longer_than_a_chunk(tmp_path, texts):
    pd, _ = both(tmp_path, ["-k", 31, "-K", "-s"], [texts["long"]], extra={"UNIKMER_CHUNK_MB": "1"})
    on_device(pd, [texts["long"]], chunks=3)


def test_four_line_fastq(tmp_path, texts):
    pd, _ = both(tmp_path, ["-k", 31, "-K", "-s"], [texts["fastq"]], extra={"UNIKMER_CHUNK_MB": "1"})
    on_device(pd, [texts["fastq"]], chunks=3)
    pd, _ = both(tmp_path, ["-k", 21, "-s"], [texts["fastq_gz"]])
    on_device(pd, [texts["fastq_gz"]], chunks=1)


@pytest.mark.parametrize("mode", [["-K", "-s"], ["-H"], ["-K", "-W", "15"], ["--circular"], ["-K", "-u", "-s"], ["-l"]])
def test_modes(tmp_path, texts, mode):
    files = [texts["crlf"], texts["fastq"]]       # two input files in one command, one FASTA and one FASTQ
    pd, _ = both(tmp_path, ["-k", 31] + mode, files, extra={"UNIKMER_CHUNK_MB": "1"})
    on_device(pd, files)


@pytest.mark.parametrize("which", ["multiline_fastq", "trailing_empty_fastq"])
def test_handover_to_the_host_parser(tmp_path, texts, which):
    f = texts[which]
    pd, _ = both(tmp_path, ["-k", 31, "-K", "-s"], [f, texts["fasta_small"]], extra={"UNIKMER_CHUNK_MB": "1"})
    rep = report(pd)
    text = open(f, "rb").read()
    at = len(fastq(4000, 150, 3)) if which == "multiline_fastq" else len(text) - 1
    assert re.fullmatch(r"fastx: %s: device, \d+ chunk\(s\), host from byte %d \(grammar\)" % (re.escape(f), at), rep[0]), rep
    assert re.fullmatch(r"fastx: %s: device, 1 chunk\(s\)" % re.escape(texts["fasta_small"]), rep[1]), rep


@pytest.mark.parametrize("which", ["garbage", "bad_fastq"])
def test_the_host_parsers_errors(tmp_path, texts, which):
    pd, ph = both(tmp_path, ["-k", 31, "-K", "-s"], [texts[which]], ok=False)
    assert pd.returncode != 0
    want = "invalid FASTA/Q format: " if which == "garbage" else "invalid FASTQ record in "
    assert any(want + texts[which] in ln for ln in others(pd))


def test_where_the_host_parser_stays(tmp_path, texts):
    f = texts["fasta_small"]
    ref = str(tmp_path / "ref")
    run(HOST, "count", "-k", 21, "-K", "-s", f, "-o", ref)
    cases = (({"UNIKMER_DEVICE_FASTX": "1"}, ["-B", "^b"], "-B"),
             ({"UNIKMER_DEVICE_FASTX": "1", "UNIKMER_HOST_FASTX": "1"}, [], "not asked for"),
             ({}, [], "not asked for"))
    for env, args, reason in cases:
        e = dict(env, UNIKMER_FASTX_REPORT="1")
        out = str(tmp_path / "out")
        p = run(e, "count", "-k", 21, "-K", "-s", *args, f, "-o", out)
        assert report(p) == ["fastx: %s: host (%s)" % (f, reason)]
        if not args:
            assert open(out + ".unik", "rb").read() == open(ref + ".unik", "rb").read()
        else:
            h = str(tmp_path / "out_h")
            run(HOST, "count", "-k", 21, "-K", "-s", *args, f, "-o", h)
            assert open(out + ".unik", "rb").read() == open(h + ".unik", "rb").read()
    # without UNIKMER_FASTX_REPORT nothing is said
    p = run({"UNIKMER_DEVICE_FASTX": "1"}, "count", "-k", 21, "-K", "-s", f, "-o", str(tmp_path / "quiet"))
    assert report(p) == [] and open(str(tmp_path / "quiet.unik"), "rb").read() == open(ref + ".unik", "rb").read()


def test_parse_taxid_stays_with_the_host_parser(tmp_path):
    f = str(tmp_path / "t.fa")
    with open(f, "wb") as fh:
        fh.write(b">s1 taxid=3\n" + seq(400, 7) + b"\n>s2 taxid=5\n" + seq(300, 8) + b"\n")
    tax = tmp_path / "tax"
    tax.mkdir()
    with open(str(tax / "nodes.dmp"), "w") as fh:
        for c, p in ((1, 1), (2, 1), (3, 2), (5, 2)):
            fh.write("%d\t|\t%d\t|\tno rank\t|\n" % (c, p))
    outs = []
    for env in ({"UNIKMER_DEVICE_FASTX": "1"}, {"UNIKMER_HOST_FASTX": "1"}):
        out = str(tmp_path / ("o%d" % len(outs)))
        p = run(dict(env, UNIKMER_FASTX_REPORT="1"), "count", "-k", 21, "-K", "-s", "-T", "-r", r"taxid=(\d+)", "--data-dir", str(tax), f, "-o", out)
        outs.append((report(p), open(out + ".unik", "rb").read()))
    assert outs[0][0] == ["fastx: %s: host (-T)" % f] and outs[1][0] == ["fastx: %s: host (not asked for)" % f]
    assert outs[0][1] == outs[1][1]
