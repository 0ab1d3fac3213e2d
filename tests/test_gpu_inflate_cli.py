"""The driver's gzip .unik inputs with the body inflated on the device (UNIKMER_DEVICE_GUNZIP=1: zlib reads the header,
ukm_inflate the body, zlib the bytes behind it) against zlib everywhere (UNIKMER_HOST_GUNZIP=1): the commands give the same
outputs byte for byte, UNIKMER_GUNZIP_REPORT=1 says which path carried each input, and files zlib's own writer made go the
host's way."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import AMUC, GOLDEN, MG1655, synth_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")
SWITCHES = ("UNIKMER_DEVICE_GZIP", "UNIKMER_HOST_GZIP", "UNIKMER_HOST_CODEC", "UNIKMER_DEVICE_GUNZIP", "UNIKMER_HOST_GUNZIP",
            "UNIKMER_GUNZIP_REPORT", "UNIKMER_DEVICE_TEXT", "UNIKMER_HOST_TEXT")


def run(env_add, *args, stdin=None):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_add)
    p = subprocess.run([BIN] + [str(a) for a in args], input=stdin, capture_output=True, env=env)
    assert p.returncode == 0, (args, p.stderr.decode(errors="replace"))
    return p


@pytest.fixture(scope="module")
def tax_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tax"))
    child, parent = synth_tree(depth=4, arity=4)
    with open(d + "/nodes.dmp", "w") as fh:
        for c, p in zip(child, parent):
            fh.write("%d\t|\t%d\t|\tno rank\t|\n" % (c, p))
    return d, len(child)


@pytest.fixture(scope="module", params=["device", "host"])
def written(request, tmp_path_factory, tax_dir):
    """count, sort and union (plain and with taxids) written with the body deflated on the device, or by zlib"""
    how = request.param
    w = {"UNIKMER_DEVICE_GZIP": "1"} if how == "device" else {"UNIKMER_HOST_GZIP": "1"}
    d = str(tmp_path_factory.mktemp("written_" + how))
    tax, ntax = tax_dir
    run(w, "count", "-k", 23, "-K", "-s", os.path.join(GOLDEN, AMUC), "-o", d + "/am")
    run(w, "count", "-k", 23, "-K", "-s", os.path.join(GOLDEN, MG1655), "-o", d + "/mg")
    run(w, "count", "-k", 23, "-K", os.path.join(GOLDEN, AMUC), "-o", d + "/am_unsorted")
    run(w, "sort", "-u", d + "/am_unsorted.unik", "-o", d + "/am_sorted")
    run(w, "union", "-s", d + "/am.unik", d + "/mg.unik", "-o", d + "/un")
    rng = np.random.default_rng(5)
    k = 13
    for f in range(2):
        codes = np.unique(rng.integers(0, 30000, 15000 + f).astype(np.uint64))
        t = rng.integers(1, ntax + 1, len(codes)).astype(np.uint32)
        kmers = ["".join("ACGT"[(int(c) >> (2 * (k - 1 - i))) & 3] for i in range(k)) for c in codes]
        txt = "".join("%s\t%d\n" % (km, tt) for km, tt in zip(kmers, t)).encode()
        run(w, "dump", "-s", "--max-taxid", 0xFFFF, "-o", d + "/raw%d" % f, "-C", stdin=txt)    # (dump writes through zlib)
        run(w, "union", "-s", "--data-dir", tax, d + "/raw%d.unik" % f, d + "/raw%d.unik" % f, "-o", d + "/t%d" % f)
    run(w, "union", "-s", "--data-dir", tax, d + "/t0.unik", d + "/t1.unik", "-o", d + "/tun")
    names = ("am", "mg", "am_unsorted", "am_sorted", "un", "t0", "t1", "tun")
    files = {n: d + "/" + n + ".unik" for n in names}
    for f in files.values():
        assert open(f, "rb").read(2) == b"\x1f\x8b", f
    return how, files


def commands(files, tax):
    return {"sort": (["sort", "-u", files["am_unsorted"]], [files["am_unsorted"]]),
            "inter": (["inter", files["am"], files["un"]], [files["am"], files["un"]]),
            "union": (["union", "-s", files["am_sorted"], files["mg"]], [files["am_sorted"], files["mg"]]),
            "union with taxids": (["union", "-s", "--data-dir", tax, files["t0"], files["t1"], files["tun"]], [files["t0"], files["t1"], files["tun"]]),
            "view": (["view", "-t", files["tun"]], [files["tun"]])}


@pytest.mark.parametrize("name", ["sort", "inter", "union", "union with taxids", "view"])
def test_commands_read_the_same_records_either_way(tmp_path, written, tax_dir, name):
    how, files = written
    cmd, inputs = commands(files, tax_dir[0])[name]
    got = {}
    for mode in ("device", "host"):
        env = {"UNIKMER_DEVICE_GUNZIP" if mode == "device" else "UNIKMER_HOST_GUNZIP": "1", "UNIKMER_GUNZIP_REPORT": "1"}
        if name == "view":
            env["UNIKMER_DEVICE_TEXT"] = "1"      # the text path that loads whole files
            p = run(env, *cmd)
            got[mode] = p.stdout
        else:
            out = str(tmp_path / mode)
            p = run(env, *cmd, "-C", "-o", out)
            got[mode] = open(out + ".unik", "rb").read()
        report = [ln for ln in p.stderr.decode().splitlines() if ln.startswith("gunzip: ")]
        assert len(report) == len(inputs), report
        for f, ln in zip(inputs, report):
            if mode == "device" and how == "device":
                m = re.fullmatch(r"gunzip: %s: device (\d+) of (\d+) bytes" % re.escape(f), ln)
                assert m, ln
                upto, size = int(m.group(1)), int(m.group(2))
                assert size == os.path.getsize(f) and 0 <= size - upto <= 64, ln
            else:
                assert re.fullmatch(r"gunzip: %s: host \(.+\)" % re.escape(f), ln), ln
    assert got["device"] == got["host"] and len(got["host"]) > 100


def test_no_report_and_no_device_path_unless_asked(tmp_path, written):
    how, files = written
    p = run({}, "union", "-s", files["am"], files["mg"], "-C", "-o", str(tmp_path / "a"))
    assert b"gunzip:" not in p.stderr
    p = run({"UNIKMER_GUNZIP_REPORT": "1"}, "union", "-s", files["am"], files["mg"], "-C", "-o", str(tmp_path / "b"))
    assert p.stderr.count(b"gunzip: ") == 2 and b": device " not in p.stderr      # the default is off
    p = run({"UNIKMER_DEVICE_GUNZIP": "1", "UNIKMER_HOST_GUNZIP": "1", "UNIKMER_GUNZIP_REPORT": "1"}, "union", "-s", files["am"], files["mg"],
            "-C", "-o", str(tmp_path / "c"))
    assert b": device " not in p.stderr
    assert open(str(tmp_path / "a") + ".unik", "rb").read() == open(str(tmp_path / "b") + ".unik", "rb").read() == open(str(tmp_path / "c") + ".unik", "rb").read()


def test_plain_files_and_stdin_go_the_hosts_way(tmp_path, written):
    how, files = written
    plain = str(tmp_path / "plain")
    run({}, "sort", "-u", files["am"], "-C", "-o", plain)
    env = {"UNIKMER_DEVICE_GUNZIP": "1", "UNIKMER_GUNZIP_REPORT": "1"}
    p = run(env, "sort", "-u", plain + ".unik", "-C", "-o", str(tmp_path / "a"))
    assert b"host (not gzip)" in p.stderr
    p = run(env, "sort", "-u", "-", "-C", "-o", str(tmp_path / "b"), stdin=open(files["am"], "rb").read())
    assert b"host (stdin)" in p.stderr
    assert open(str(tmp_path / "a") + ".unik", "rb").read() == open(str(tmp_path / "b") + ".unik", "rb").read() == open(plain + ".unik", "rb").read()
