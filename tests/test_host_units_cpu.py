"""The driver's device-free layer (unikmer_amd/host/base.hpp, seqtext.hpp: flag parser, byte sizes, FASTA/Q parser, k-mer
text, degenerate bases, rank-order file, nodes.dmp lines) under the address and undefined-behaviour sanitizers, as a
stand-alone program: tests/host_units.cpp includes the headers, needs neither the library nor a device, and prints OK."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_free_layer_under_sanitizers(tmp_path):
    """no Python-loaded code runs under a sanitizer: the layer is header-only C++ and gets a main() of its own"""
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the driver; it must be here"
    exe = str(tmp_path / "host_units")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "unikmer_amd", "host"), os.path.join(ROOT, "tests", "host_units.cpp"), "-o", exe, "-lz"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.returncode, r.stdout, r.stderr)
