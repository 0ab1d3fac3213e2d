"""The driver's compressed .unik outputs with the body deflated on the device (UNIKMER_DEVICE_GZIP=1: ukm_deflate, one gzip
member assembled by unik::OutStream) against zlib everywhere (UNIKMER_HOST_GZIP=1) and against -C: all three inflate to the
same bytes, both compressed forms are gzip, and the driver's own gzread reads the device form back (view, num -n)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import AMUC, GOLDEN, MG1655, synth_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")
MODES = {"device": {"UNIKMER_DEVICE_GZIP": "1"}, "host": {"UNIKMER_HOST_GZIP": "1"}}


def run(mode, *args, stdin=None):
    env = {k: v for k, v in os.environ.items() if k not in ("UNIKMER_DEVICE_GZIP", "UNIKMER_HOST_GZIP", "UNIKMER_HOST_CODEC")}
    env.update(MODES[mode])
    p = subprocess.run([BIN] + [str(a) for a in args], input=stdin, capture_output=True, env=env)
    assert p.returncode == 0, (args, p.stderr.decode(errors="replace"))
    return p


def files_below(d):
    return {os.path.relpath(os.path.join(b, n), d): open(os.path.join(b, n), "rb").read() for b, _, ns in os.walk(d) for n in ns}


def three_ways(tmp_path, name, make, min_files=1):
    """make(mode, directory, extra flags) writes into the directory: device gzip, host gzip and -C must hold the same bytes
    once inflated, and both compressed forms are gzip.  Returns {relative path: (device path, host path)}."""
    got, dirs = {}, {}
    for mode, flags in (("device", []), ("host", []), ("plain", ["-C"])):
        d = tmp_path / (name + "_" + mode)
        d.mkdir()
        make("host" if mode == "plain" else mode, str(d), flags)
        got[mode], dirs[mode] = files_below(str(d)), str(d)
    assert got["device"].keys() == got["host"].keys() == got["plain"].keys() and len(got["plain"]) >= min_files
    for f, want in got["plain"].items():
        assert want[:8] == b".unikmer" and len(want) > 100
        for mode in MODES:
            raw = got[mode][f]
            assert raw[:2] == b"\x1f\x8b", (name, mode, f)
            assert gzip.decompress(raw) == want, (name, mode, f)
    return {f: (os.path.join(dirs["device"], f), os.path.join(dirs["host"], f)) for f in got["plain"]}


def reads_back_the_same(pair, view=False):
    """the driver's own reader on the device-gzip file: what num -n prints and, for a small file, view"""
    dev, host = pair
    for cmd in ([["view"]] if view else []) + [["num", "-n"]]:
        a, b = run("host", *cmd, dev).stdout, run("host", *cmd, host).stdout
        if cmd[0] == "num":  # "<count>\t<file>"
            a, b = a.split(b"\t")[0], b.split(b"\t")[0]
        assert a == b and len(a) > 0, cmd


@pytest.fixture(scope="module")
def counted(tmp_path_factory):
    d = tmp_path_factory.mktemp("counted")
    out = {}
    for name, fa in (("am", AMUC), ("mg", MG1655)):
        run("host", "count", "-k", 23, "-K", "-s", os.path.join(GOLDEN, fa), "-o", d / name, "-C")
        out[name] = str(d / (name + ".unik"))
    run("host", "count", "-k", 23, "-K", os.path.join(GOLDEN, AMUC), "-o", d / "am_unsorted", "-C")
    out["am_unsorted"] = str(d / "am_unsorted.unik")
    return out


def test_count(tmp_path):
    fa = os.path.join(GOLDEN, AMUC)
    files = three_ways(tmp_path, "count", lambda m, d, fl: run(m, "count", "-k", 23, "-K", "-s", fa, "-o", d + "/o", *fl))
    dev, host = files["o.unik"]
    assert os.path.getsize(dev) < len(gzip.decompress(open(dev, "rb").read()))   # a sorted body does shrink
    reads_back_the_same(files["o.unik"])
    three_ways(tmp_path, "count_unsorted", lambda m, d, fl: run(m, "count", "-k", 23, "-K", fa, "-o", d + "/o", *fl))


def test_sort(tmp_path, counted):
    files = three_ways(tmp_path, "sort", lambda m, d, fl: run(m, "sort", "-u", counted["am_unsorted"], "-o", d + "/o", *fl))
    reads_back_the_same(files["o.unik"])


def test_union(tmp_path, counted):
    files = three_ways(tmp_path, "union", lambda m, d, fl: run(m, "union", "-s", counted["am"], counted["mg"], "-o", d + "/o", *fl))
    reads_back_the_same(files["o.unik"])


@pytest.fixture(scope="module")
def taxed(tmp_path_factory):
    """two small sorted files with per-record taxids and a taxonomy they belong to"""
    d = str(tmp_path_factory.mktemp("taxed"))
    child, parent = synth_tree(depth=4, arity=4)
    os.makedirs(d + "/tax")
    with open(d + "/tax/nodes.dmp", "w") as fh:
        for c, p in zip(child, parent):
            fh.write("%d\t|\t%d\t|\tno rank\t|\n" % (c, p))
    rng = np.random.default_rng(5)
    k = 13
    fs = []
    for f in range(2):
        codes = np.unique(rng.integers(0, 30000, 15000).astype(np.uint64))
        t = rng.integers(1, len(child) + 1, len(codes)).astype(np.uint32)
        kmers = ["".join("ACGT"[(int(c) >> (2 * (k - 1 - i))) & 3] for i in range(k)) for c in codes]
        txt = "".join("%s\t%d\n" % (km, tt) for km, tt in zip(kmers, t)).encode()
        run("host", "dump", "-s", "--max-taxid", 0xFFFF, "-o", d + "/f%d" % f, "-C", stdin=txt)
        fs.append(d + "/f%d.unik" % f)
    return d + "/tax", fs


def test_union_with_taxids_and_tsplit(tmp_path, taxed):
    tax, fs = taxed
    files = three_ways(tmp_path, "union_t", lambda m, d, fl: run(m, "union", "-s", "--data-dir", tax, *fs, "-o", d + "/o", *fl))
    reads_back_the_same(files["o.unik"], view=True)
    three_ways(tmp_path, "tsplit", lambda m, d, fl: run(m, "tsplit", fs[0], "-O", d + "/groups", *fl), min_files=100)


def test_compression_level_0_stays_on_zlib(tmp_path, counted):
    want = open(counted["am"], "rb").read()
    out = str(tmp_path / "o")
    run("device", "union", "-s", counted["am"], counted["am"], "-o", out, "--compression-level", 0)
    raw = open(out + ".unik", "rb").read()
    assert raw[:2] == b"\x1f\x8b" and len(raw) > len(want)   # level 0: stored blocks
    got = gzip.decompress(raw)
    assert got[:8] == b".unikmer" and abs(len(got) - len(want)) < 64
    assert run("host", "num", "-n", out + ".unik").stdout.split(b"\t")[0] == run("host", "num", "-n", counted["am"]).stdout.split(b"\t")[0]
