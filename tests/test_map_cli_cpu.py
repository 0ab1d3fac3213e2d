"""`locate` / `map`: what can be checked without a GPU -- the two entry points exist in header, binding and library, and
both commands refuse bad invocations (with the reference's messages) before a device context is created."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")
NEW = ("ukm_locate", "ukm_map")


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


def test_help_lists_both_commands(cli):
    p = cli("--help")
    text = (p.stdout + p.stderr).decode()
    assert p.returncode == 0 and re.search(r"\blocate\b", text) and re.search(r"\bmap\b", text)


@pytest.fixture(scope="module")
def unik_files(cli, tmp_path_factory):
    d = tmp_path_factory.mktemp("mapcli")
    fa = d / "g.fa"
    fa.write_text(">r1 first\nACGTACGTTGCAACGTAGCTAGCTAGGATCGATCGTAGCTAGCTAGCATCGA\n")
    kmers = b"ACGTACGTTGC\nCGTACGTTGCA\n"
    assert cli("dump", "-K", "-o", d / "canon", stdin=kmers).returncode == 0
    assert cli("dump", "-o", d / "plain", stdin=kmers).returncode == 0
    return str(fa), str(d / "canon") + ".unik", str(d / "plain") + ".unik"


@pytest.mark.parametrize("cmd", ["locate", "map", "uniqs"])
def test_genome_flag_needed(cli, unik_files, cmd):
    fa, canon, plain = unik_files
    p = cli(cmd, canon)
    assert p.returncode != 0 and b"flag -g/--genome needed" in p.stderr


@pytest.mark.parametrize("cmd", ["locate", "map"])
def test_canonical_flag_needed(cli, unik_files, cmd):
    fa, canon, plain = unik_files
    p = cli(cmd, "-g", fa, plain)
    assert p.returncode != 0 and b"'canonical' flag is needed" in p.stderr and plain.encode() in p.stderr


def test_map_refuses_gaps_circular_and_M_with_W(cli, unik_files):
    fa, canon, plain = unik_files
    p = cli("map", "-x", 1, "-X", 1, "-g", fa, canon)
    assert p.returncode != 0 and b"--max-gap-size" in p.stderr and b"--max-gap-num" in p.stderr
    p = cli("map", "-X", 2, "-g", fa, canon)
    assert p.returncode != 0 and b"--max-gap-num" in p.stderr
    p = cli("map", "--circular", "-g", fa, canon)
    assert p.returncode != 0 and b"--circular" in p.stderr
    p = cli("map", "-M", "-W", "-g", fa, canon)
    assert p.returncode != 0
    assert b"flag -M/--allow-multiple-mapped-kmers and -W/--seqs-in-a-file-as-one-genome are not compatible" in p.stderr
    p = cli("map", "-m", 0, "-g", fa, canon)
    assert p.returncode != 0 and b"--min-len" in p.stderr
