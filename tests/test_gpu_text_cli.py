"""The driver with the device text path (UNIKMER_DEVICE_TEXT=1: `view` through ukm_view, `dump` through ukm_dump) against the
same commands on the host loops of cmd_cpu.hpp (UNIKMER_HOST_TEXT=1): stdout and every output file, inflated, are the same."""
import gzip
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import AMUC, GOLDEN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")
PATHS = {"device": {"UNIKMER_DEVICE_TEXT": "1"}, "host": {"UNIKMER_HOST_TEXT": "1"}}


def run(path, *args, stdin=None):
    env = {k: v for k, v in os.environ.items() if k not in ("UNIKMER_DEVICE_TEXT", "UNIKMER_HOST_TEXT")}
    env.update(PATHS[path])
    p = subprocess.run([BIN] + [str(a) for a in args], input=stdin, capture_output=True, env=env)
    assert p.returncode == 0, (args, p.stderr.decode(errors="replace"))
    return p


def inflated(path):
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """`count -k 23 -K -s -t` of one golden genome (a global taxid), and a small file with per-record taxids"""
    d = tmp_path_factory.mktemp("textcli")
    run("host", "count", "-k", 23, "-K", "-s", "-t", 349741, os.path.join(GOLDEN, AMUC), "-o", d / "am")
    rng = np.random.default_rng(7)
    k = 13
    codes = np.unique(rng.integers(0, 1 << 26, 6000).astype(np.uint64))
    tax = rng.integers(0, 1 << 32, len(codes), dtype=np.uint64)
    text = "".join("%s\t%d\n" % ("".join("ACGT"[(int(c) >> (2 * (k - 1 - i))) & 3] for i in range(k)), t) for c, t in zip(codes, tax)).encode()
    run("host", "dump", "-s", "-o", d / "taxed", stdin=text)
    return {"genome": str(d / "am.unik"), "taxed": str(d / "taxed.unik"), "text": text}


VIEW_FLAGS = [c for r in range(3) for c in itertools.combinations(["-n", "-N", "-t", "-T", "-a", "-q"], r)]


@pytest.mark.parametrize("flags", VIEW_FLAGS, ids=lambda f: "".join(f) or "plain")
def test_view_in_every_flag_combination(files, flags):
    extras = ((), ("-I",)) if len(flags) < 2 else ((),)          # -I: the header's taxid is printed all the same
    for extra in extras:
        a, b = run("device", "view", files["taxed"], *flags, *extra), run("host", "view", files["taxed"], *flags, *extra)
        assert a.stdout == b.stdout and len(b.stdout) > 1000, (flags, extra)


@pytest.mark.parametrize("flags", [(), ("-t",), ("-a", "-t", "-I")], ids=lambda f: "".join(f) or "plain")
def test_view_of_a_genomes_kmers(files, flags):
    a, b = run("device", "view", files["genome"], *flags), run("host", "view", files["genome"], *flags)
    assert a.stdout == b.stdout and b.stdout.count(b"\n") > 1 << 20


def test_view_to_a_gzipped_file_and_of_two_files(tmp_path, files):
    for path in PATHS:
        run(path, "view", "-a", files["taxed"], files["taxed"], "-o", tmp_path / (path + ".fa.gz"))
    assert inflated(tmp_path / "device.fa.gz") == inflated(tmp_path / "host.fa.gz")


DUMPS = [(), ("-s",), ("-u",), ("-K",), ("-O",), ("-u", "-K"), ("-s", "-C"), ("-c",), ("-t", 562), ("-s", "--max-taxid", 0xFFFFFF)]


@pytest.mark.parametrize("column", ["taxids", "plain"])
@pytest.mark.parametrize("flags", DUMPS, ids=lambda f: "".join(str(x) for x in f) or "plain")
def test_dump_in_every_flag_combination(tmp_path, files, flags, column):
    base = files["text"] if column == "taxids" else b"".join(ln.split(b"\t")[0] + b"\r\n" for ln in files["text"].splitlines())
    # -s wants ascending codes; everything else gets repeated lines behind them (for -u)
    src = base if "-s" in flags else base + b"".join(base.splitlines(True)[:2000])
    for path in PATHS:
        run(path, "dump", *flags, "-o", tmp_path / path, stdin=src)
    a, b = inflated(tmp_path / "device.unik"), inflated(tmp_path / "host.unik")
    assert a == b and len(b) > 1000


def test_dump_of_hashed_codes_and_of_files(tmp_path, files):
    hashed = run("host", "view", "-N", files["genome"]).stdout          # decimal codes, one per line
    assert hashed.count(b"\n") > 1 << 20
    for path in PATHS:
        run(path, "dump", "--hashed", "-k", 23, "-s", "-o", tmp_path / ("h_" + path), stdin=hashed)
    assert inflated(tmp_path / "h_device.unik") == inflated(tmp_path / "h_host.unik")
    # the text of `view -t` back through dump, from two files (one of them gzipped)
    with open(tmp_path / "a.txt", "wb") as fh:
        fh.write(files["text"])
    with gzip.open(tmp_path / "b.txt.gz", "wb") as fh:
        fh.write(b"".join(files["text"].splitlines(True)[:3000]))
    for path in PATHS:
        run(path, "dump", "-u", tmp_path / "a.txt", tmp_path / "b.txt.gz", "-o", tmp_path / ("f_" + path))
    assert inflated(tmp_path / "f_device.unik") == inflated(tmp_path / "f_host.unik")
    a, b = run("device", "view", "-t", tmp_path / "f_device.unik").stdout, run("host", "view", "-t", tmp_path / "f_host.unik").stdout
    assert a == b == files["text"]
