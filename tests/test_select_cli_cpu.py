"""`grep` / `filter` / `sample`: what can be checked without a GPU -- the three entry points exist in header, binding and
library, `--help` lists the commands, and bad invocations are refused (with the reference's messages) before a device
context is created."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")
NEW = ("ukm_grep", "ukm_filter", "ukm_sample")


@pytest.fixture(scope="module")
def cli():
    from unikmer_amd import build
    build.build()
    assert os.path.exists(BIN)

    def run(*args, stdin=None):
        return subprocess.run([BIN] + [str(a) for a in args], input=stdin, capture_output=True)
    return run


def test_entry_points_declared_listed_exported(cli):
    from unikmer_amd import lib
    header = open(os.path.join(ROOT, "include", "unikmer_hip.h")).read()
    so = ctypes.CDLL(lib.SO_PATH)
    for name in NEW:
        assert re.search(r"^int %s\(ukm_ctx \*ctx," % name, header, re.M), name
        assert name in lib.SYMBOLS
        assert hasattr(so, name)
        assert callable(getattr(lib.Context, name[4:]))
    assert re.search(r"^#define UKM_F_INVERT 8u", header, re.M) and re.search(r"^#define UKM_F_QUERY_TAXID 16u", header, re.M)
    assert (lib.F_INVERT, lib.F_QUERY_TAXID) == (8, 16)
    assert '"grep_lds"' in header


def test_help_lists_the_commands(cli):
    p = cli("--help")
    text = (p.stdout + p.stderr).decode()
    assert p.returncode == 0
    for cmd in ("grep", "filter", "sample"):
        assert re.search(r"\b%s\b" % cmd, text), cmd


@pytest.fixture(scope="module")
def unik_files(cli, tmp_path_factory):
    d = tmp_path_factory.mktemp("selectcli")
    kmers = b"ACGTACGTTGC\nCGTACGTTGCA\nAAAAAAAAAAA\n"
    assert cli("dump", "-K", "-o", d / "canon", stdin=kmers).returncode == 0
    assert cli("dump", "-K", "-o", d / "other", stdin=kmers[:12]).returncode == 0
    assert cli("dump", "-K", "-o", d / "taxed", stdin=b"ACGTACGTTGC\t9606\nCGTACGTTGCA\t562\n").returncode == 0
    assert cli("dump", "-K", "-t", 562, "-o", d / "global", stdin=kmers).returncode == 0
    return tuple(str(d / n) + ".unik" for n in ("canon", "other", "taxed", "global"))


def failed(p, message):
    return p.returncode != 0 and p.stderr.startswith(b"[ERRO] ") and message in p.stderr


def test_grep_needs_a_query(cli, unik_files):
    canon = unik_files[0]
    assert failed(cli("grep", canon), b"one of flags -q/--query, -f/--query-file and -F/--query-unik-file needed")
    assert failed(cli("grep", "-v", "-s", canon), b"one of flags -q/--query, -f/--query-file and -F/--query-unik-file needed")


def test_grep_query_lengths(cli, unik_files, tmp_path):
    canon = unik_files[0]
    p = cli("grep", "-q", "ACGTACGTTGC", "-q", "ACGT", canon)
    assert failed(p, b"length of query sequence are inconsistent: (4) != (11): ACGT")
    qf = tmp_path / "q.txt"
    qf.write_text("ACGTACGTTGC\nACGTACGTTGCA\n")
    assert failed(cli("grep", "-f", qf, canon), b"length of query sequence are inconsistent: (12) != (11): ACGTACGTTGCA")
    assert failed(cli("grep", "-q", "ACGTACGTTGCAA", canon), b"K (11) of binary file '%s' not equal to query K (13)" % canon.encode())
    assert failed(cli("grep", "-D", "-q", "ACGTACGTTGZ", canon), b"fail to extend degenerate sequence 'ACGTACGTTGZ'")
    assert failed(cli("grep", "-t", "-q", "abc", canon), b"query taxid should be positive integer in range of [1, 4294967295]: abc")
    assert failed(cli("grep", "-t", "-q", "0", canon), b"query taxid should be positive integer in range of [1, 4294967295]: 0")
    assert failed(cli("grep", "-t", "-F", unik_files[1], canon), b"no taxids found in file: %s" % unik_files[1].encode())


def test_grep_refuses_multiple_outfiles(cli, unik_files, tmp_path):
    canon = unik_files[0]
    for flags in (["-m"], ["-m", "-O", tmp_path / "out"], ["-O", tmp_path / "out"], ["--force"], ["-m", "-s"]):
        p = cli("grep", "-q", "ACGTACGTTGC", *flags, canon)
        assert failed(p, b"-m/--multiple-outfiles") and b"not supported" in p.stderr
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("flag", ["-u", "-d"])
def test_grep_unique_refused_with_taxids(cli, unik_files, flag):
    canon, other, taxed, glob = unik_files
    for f in (taxed, glob):
        p = cli("grep", "-q", "ACGTACGTTGC", flag, f)
        assert failed(p, b"-u/--unique and -d/--repeated are not supported for inputs with taxids")


def test_grep_taxid_mix_refused(cli, unik_files):
    canon, other, taxed, glob = unik_files
    p = cli("grep", "-q", "ACGTACGTTGC", canon, taxed)
    assert failed(p, b"taxid information not found in previous files, but found in this: %s" % taxed.encode())
    p = cli("grep", "-q", "ACGTACGTTGC", taxed, canon)
    assert failed(p, b"taxid information found in previous files, but missing in this: %s" % canon.encode())


def test_filter_refusals(cli, unik_files):
    canon, other = unik_files[:2]
    assert failed(cli("filter", canon, other), b"no more than one file should be given")
    assert failed(cli("filter", "-t", -1, canon), b"value of flag --threshold should be greater than or equal to 0")
    assert failed(cli("filter", "-w", 0, canon), b"value of flag --window should be greater than 0")


def test_sample_refusals(cli, unik_files):
    canon, other, taxed, glob = unik_files
    assert failed(cli("sample", "-s", 0, canon), b"value of flag --start should be greater than 0")
    assert failed(cli("sample", "-w", 0, canon), b"value of flag --window should be greater than 0")
    p = cli("sample", canon, taxed)
    assert failed(p, b"taxid information not found in previous files, but found in this: %s" % taxed.encode())
    p = cli("sample", glob, canon)
    assert failed(p, b"taxid information found in previous files, but missing in this: %s" % canon.encode())
