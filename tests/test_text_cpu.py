"""`view` / `dump` text without a GPU: ukm_view_bound (pure host code) against tests/text_model.py, and the model pinned to the
host loops of unikmer_amd/host/cmd_cpu.hpp -- which are what runs on a machine without a device and under
UNIKMER_HOST_TEXT=1 -- so that the GPU tests can hold ukm_view / ukm_dump to the model alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")
ENVS = {"default": {}, "host": {"UNIKMER_HOST_TEXT": "1"}}
VIEW_FLAGS = {M.KMER: [], M.KMER_CODE: ["-n"], M.CODE: ["-N"], M.KMER_TAXID: ["-t"], M.TAXID: ["-T"], M.FASTA: ["-a"], M.FASTQ: ["-q"],
              M.FASTA | M.WITH_TAXID: ["-a", "-t"], M.FASTQ | M.WITH_TAXID: ["-q", "-t"]}


@pytest.fixture(scope="module")
def cli():
    from unikmer_amd import build
    build.build()

    def run(env, *args, stdin=None):
        e = {k: v for k, v in os.environ.items() if k not in ("UNIKMER_HOST_TEXT", "UNIKMER_DEVICE_TEXT")}
        e.update(ENVS[env])
        return subprocess.run([BIN] + [str(a) for a in args], input=stdin, capture_output=True, env=e)
    return run


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_view_bound_is_the_models(fmt):
    from unikmer_amd import build, lib
    build.build()
    L = lib.load()
    assert hasattr(L, "ukm_view_bound")
    for hashed in (0, 1):
        for k in (1, 31, 32, 64):
            if k > 32 and not hashed:
                continue
            for n in (0, 1, 1 << 33):
                assert L.ukm_view_bound(n, k, hashed, fmt) == M.bound(n, k, bool(hashed), fmt) == lib.view_bound(n, k, hashed, fmt)
    # exact where every line has one length
    assert L.ukm_view_bound(1 << 33, 31, 0, M.KMER) == (1 << 33) * 32


def some_text(n, k, seed, taxids=True):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 1 << (2 * k), n, dtype=np.uint64)
    tax = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    tax[:4] = (0, 9, 10, (1 << 32) - 1)
    lines = [M.kmer_text(int(c), k) + ("\t%d" % t if taxids else "") for c, t in zip(codes, tax)]
    return ("\n".join(lines) + "\n").encode()


@pytest.fixture(scope="module")
def dumped(cli, tmp_path_factory):
    """a file with per-record taxids made by `dump` from 2,000 lines, and the records the model reads from them"""
    d = tmp_path_factory.mktemp("textcpu")
    text = some_text(2000, 21, 1)
    p = cli("host", "dump", "-o", d / "t", stdin=text)
    assert p.returncode == 0, p.stderr
    want = M.parse(text, 21, M.D_TAXID)
    assert want.bad_off is None and len(want.codes) == 2000
    return str(d / "t.unik"), want


@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_view_prints_the_models_text(cli, dumped, env, fmt):
    f, want = dumped
    p = cli(env, "view", f, *VIEW_FLAGS[fmt])
    assert p.returncode == 0, p.stderr
    assert p.stdout == M.render(want.codes, want.taxids, 0, 21, False, fmt)


@pytest.mark.parametrize("env", list(ENVS))
def test_view_of_hashed_codes_and_a_global_taxid(cli, tmp_path, env):
    codes = [0, 9, 10, 10 ** 19 - 1, 10 ** 19, (1 << 64) - 1, 12345]
    text = "".join("%d\n" % c for c in codes).encode()
    assert cli("host", "dump", "--hashed", "-k", 64, "-t", 562, "-o", tmp_path / "h", stdin=text).returncode == 0
    for fmt in M.FORMATS:
        for ignore in ([], ["-I"]):       # the header's taxid is printed also when taxids are ignored
            p = cli(env, "view", tmp_path / "h.unik", *VIEW_FLAGS[fmt], *ignore)
            assert p.returncode == 0, p.stderr
            assert p.stdout == M.render(codes, None, 562, 64, True, fmt), (fmt, ignore)


@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("flags,args", [(0, []), (M.D_CANONICAL, ["-K"]), (M.D_CANONICAL_ONLY, ["-O"])])
def test_dump_reads_the_models_records(cli, tmp_path, env, flags, args):
    k = 17
    for taxids in (True, False):
        text = some_text(1500, k, 2, taxids).replace(b"\n", b"\r\n", 700) + b"\n\n" + M.kmer_text(5, k).encode() + (b"\t7" if taxids else b"")
        want = M.parse(text, k, flags | (M.D_TAXID if taxids else 0))
        assert want.bad_off is None
        assert cli(env, "dump", *args, "-o", tmp_path / "d", stdin=text).returncode == 0
        p = cli("host", "view", "-N", "-t", tmp_path / "d.unik")      # (-t wins: k-mer and taxid)
        assert p.stdout == M.render(want.codes, want.taxids, 0, k, False, M.KMER_TAXID)
        p = cli("host", "view", "-N", tmp_path / "d.unik")
        assert p.stdout == M.render(want.codes, None, 0, k, False, M.CODE)


@pytest.mark.parametrize("env", list(ENVS))
def test_dump_reads_decimal_codes(cli, tmp_path, env):
    text = b"0\t1\n18446744073709551615\t4294967295\r\n007\t08\n\n10000000000000000000\t10"
    want = M.parse(text, 0, M.D_DECIMAL | M.D_TAXID)
    assert want.codes == [0, (1 << 64) - 1, 7, 10 ** 19] and want.taxids == [1, (1 << 32) - 1, 8, 10]
    assert cli(env, "dump", "--hashed", "-k", 40, "-o", tmp_path / "d", stdin=text).returncode == 0
    p = cli("host", "view", "-t", tmp_path / "d.unik")
    assert p.stdout == M.render(want.codes, want.taxids, 0, 40, True, M.KMER_TAXID)


LENIENT = {
    "space separator": b"ACGTA 5\nCCGTA 6\n",
    "trailing blanks": b"ACGTA\t5  \nCCGTA\t6 \r\n",
    "missing second column": b"ACGTA\t5\nCCGTA\nGGGTA\t7\n",
    "length mismatch": b"ACGTA\nCCG\n",
    "illegal base": b"ACGTA\nAC!TA\n",
    "k above 32": b"A" * 33 + b"\n",
    "nothing": b"\n\n",
}


@pytest.mark.parametrize("what", list(LENIENT))
def test_text_outside_the_strict_grammar_is_read_as_before(cli, tmp_path, what):
    """illegal for ukm_dump, accepted (or refused in its own words) by the host loop: the same output and stderr either way"""
    text = LENIENT[what]
    assert M.parse(text, 5, M.D_TAXID if b"5" in text[:8] else 0).bad_off is not None or what in ("k above 32", "nothing")
    got = {}
    for env in ENVS:
        p = cli(env, "dump", "-o", tmp_path / ("o_" + env), stdin=text)
        out = tmp_path / ("o_" + env + ".unik")
        v = cli("host", "view", "-t", "-n", out) if p.returncode == 0 else None
        got[env] = (p.returncode, p.stderr.replace(env.encode(), b"ENV"), v.stdout if v else None)
    assert got["default"] == got["host"]
    if what in ("space separator", "trailing blanks", "missing second column"):
        assert got["host"][0] == 0 and got["host"][2].count(b"\n") == text.count(b"\n")
