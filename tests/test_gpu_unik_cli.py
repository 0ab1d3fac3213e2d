"""The driver with the device codec (UNIKMER_DEVICE_CODEC=1: .unik bodies through ukm_unik_decode / ukm_unik_encode) against
the same commands on the host codec of unik.hpp (UNIKMER_HOST_CODEC=1): every output file is the same after inflating --
gzip bytes are not compared.  With and without -C, plain files and files with taxids."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import AMUC, GOLDEN, IAI39, MG1655, synth_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")
CODECS = {"device": {"UNIKMER_DEVICE_CODEC": "1"}, "host": {"UNIKMER_HOST_CODEC": "1"}}


def run(codec, *args, stdin=None, ok=True, cwd=None):
    env = {k: v for k, v in os.environ.items() if k not in ("UNIKMER_DEVICE_CODEC", "UNIKMER_HOST_CODEC")}
    env.update(CODECS[codec])
    p = subprocess.run([BIN] + [str(a) for a in args], input=stdin, capture_output=True, env=env, cwd=cwd)
    if ok:
        assert p.returncode == 0, (args, p.stderr.decode(errors="replace"))
    return p


def inflated(path):
    raw = open(path, "rb").read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def tree(d):
    """{relative path: inflated bytes} of every file below d"""
    out = {}
    for base, _, names in os.walk(d):
        for n in names:
            p = os.path.join(base, n)
            out[os.path.relpath(p, d)] = inflated(p)
    return out


def same_outputs(tmp_path, name, make):
    """make(codec, directory) runs a command that writes into the directory: both codecs must leave the same files"""
    got = {}
    for codec in CODECS:
        d = tmp_path / (name + "_" + codec)
        d.mkdir()
        make(codec, str(d))
        got[codec] = tree(str(d))
    assert got["device"].keys() == got["host"].keys() and len(got["host"]) > 0
    for f in got["host"]:
        assert len(got["host"][f]) > 100, f
        assert got["device"][f] == got["host"][f], (name, f)
    return got["host"]


@pytest.fixture(scope="module", params=["gz", "plain"])
def counted(request, tmp_path_factory):
    """`count -s` of the three FASTA fixtures under both codecs (the outputs must agree), with or without -C"""
    d = tmp_path_factory.mktemp("counted_" + request.param)
    flag = ["-C"] if request.param == "plain" else []
    files = {}
    for name, fa, taxid in (("mg", MG1655, 511145), ("ia", IAI39, 585057), ("am", AMUC, 349741)):
        for codec in CODECS:
            run(codec, "count", "-k", 23, "-K", "-s", "-t", taxid, os.path.join(GOLDEN, fa), "-o", d / (name + "_" + codec), *flag)
        a, b = inflated(str(d / (name + "_device.unik"))), inflated(str(d / (name + "_host.unik")))
        assert a == b and len(a) > 1 << 20
        files[name] = str(d / (name + "_host.unik"))
    # and one file that is not sorted: count without -s (the records are in sorted order, the layout is the unsorted one)
    run("host", "count", "-k", 23, "-K", os.path.join(GOLDEN, AMUC), "-o", d / "am_unsorted", *flag)
    files["am_unsorted"] = str(d / "am_unsorted.unik")
    return flag, files


def test_count_unsorted_and_compact(tmp_path, counted):
    flag, _ = counted
    same_outputs(tmp_path, "count_l", lambda c, d: run(c, "count", "-k", 23, "-K", os.path.join(GOLDEN, AMUC), "-o", d + "/u", *flag))
    same_outputs(tmp_path, "count_c", lambda c, d: run(c, "count", "-k", 23, "-K", "-c", os.path.join(GOLDEN, AMUC), "-o", d + "/c", *flag))


@pytest.mark.parametrize("cmd", ["union", "union -s", "inter", "diff", "diff -s"])
def test_set_operations(tmp_path, counted, cmd):
    flag, f = counted
    args = cmd.split()
    inputs = [f["mg"], f["ia"], f["am"]] if args[0] == "union" else [f["mg"], f["ia"]]
    same_outputs(tmp_path, args[0], lambda c, d: run(c, *args, "-I", *inputs, "-o", d + "/o", *flag))


SORTS = {"sort": ["sort", "-I"], "sort -u": ["sort", "-I", "-u"],
         # a small chunk size: chunk files are written and merged in two rounds (-M 3), and kept (-k) to be compared as well
         "sort -m": ["sort", "-I", "-m", 400000, "-M", 3, "-k"],
         "split": ["split", "-I", "-m", 1000000]}


@pytest.mark.parametrize("cmd", list(SORTS))
def test_sort_and_chunked_sort(tmp_path, counted, cmd):
    flag, f = counted
    src = f["am_unsorted"]
    if cmd == "split":
        same_outputs(tmp_path, "split", lambda c, d: run(c, *SORTS[cmd], "-O", d + "/chunks", src, *flag))
    elif cmd == "sort -m":
        same_outputs(tmp_path, "sort_m", lambda c, d: run(c, *SORTS[cmd], "-t", d, src, "-o", d + "/s", *flag))
    else:
        same_outputs(tmp_path, "sort", lambda c, d: run(c, *SORTS[cmd], src, "-o", d + "/s", *flag))


@pytest.fixture(scope="module")
def taxed(tmp_path_factory):
    """three small sorted files with per-record taxids (3-byte taxids: --max-taxid) and a taxonomy they belong to"""
    d = str(tmp_path_factory.mktemp("taxed"))
    child, parent = synth_tree(depth=4, arity=4)
    os.makedirs(d + "/tax")
    with open(d + "/tax/nodes.dmp", "w") as fh:
        for c, p in zip(child, parent):
            fh.write("%d\t|\t%d\t|\tno rank\t|\n" % (c, p))
    rng = np.random.default_rng(5)
    k = 13
    fs = []
    for f in range(3):
        codes = np.unique(rng.integers(0, 30000, 15000).astype(np.uint64))
        t = rng.integers(1, len(child) + 1, len(codes)).astype(np.uint32)
        kmers = ["".join("ACGT"[(int(c) >> (2 * (k - 1 - i))) & 3] for i in range(k)) for c in codes]
        txt = "".join("%s\t%d\n" % (km, tt) for km, tt in zip(kmers, t)).encode()
        run("host", "dump", "-s", "--max-taxid", 0xFFFFFF if f else 0xFFFF, "-o", d + "/f%d" % f, stdin=txt)
        fs.append(d + "/f%d.unik" % f)
    return d + "/tax", fs


@pytest.mark.parametrize("flag", [[], ["-C"]], ids=["gz", "plain"])
def test_files_with_taxids(tmp_path, taxed, flag):
    tax, fs = taxed
    same_outputs(tmp_path, "union", lambda c, d: run(c, "union", "-s", "--data-dir", tax, *fs, "-o", d + "/o", *flag))
    same_outputs(tmp_path, "inter", lambda c, d: run(c, "inter", "--data-dir", tax, *fs, "-o", d + "/o", *flag))
    same_outputs(tmp_path, "diff", lambda c, d: run(c, "diff", "-s", "-t", "--data-dir", tax, *fs, "-o", d + "/o", *flag))
    same_outputs(tmp_path, "sortu", lambda c, d: run(c, "sort", "-u", "-m", 5000, "-M", 3, "-t", d, "--data-dir", tax, *fs, "-o", d + "/o", *flag))
    same_outputs(tmp_path, "sample", lambda c, d: run(c, "sample", "-s", 3, "-w", 7, fs[0], "-o", d + "/o", *flag))
    same_outputs(tmp_path, "filter", lambda c, d: run(c, "filter", fs[1], "-o", d + "/o", *flag))
    split = same_outputs(tmp_path, "tsplit", lambda c, d: run(c, "tsplit", fs[0], "-O", d + "/groups", *flag))
    assert len(split) > 100


def test_truncated_file_fails_with_the_readers_message(tmp_path, counted):
    flag, f = counted
    whole = inflated(f["am"])
    cut = str(tmp_path / "cut.unik")
    with open(cut, "wb") as fh:
        fh.write(whole[:-1])          # a sorted body: the last record is at least 3 bytes, one of them is gone
    for codec in CODECS:
        p = run(codec, "union", "-I", f["am"], cut, "-o", tmp_path / ("o_" + codec), ok=False)
        assert p.returncode != 0 and b"unexpected EOF" in p.stderr and cut.encode() in p.stderr, (codec, p.stderr)
