"""The tile order of the set operation's table passes without a GPU: the plain arithmetic of
unikmer_amd/csrc/ukm_setop_order.h (grid size, block -> tile) as a stand-alone program under the address and
undefined-behaviour sanitizers (tests/setop_order_units.cpp): for every tile count from 1 to 4200 and for the 205 593 tiles of
2 x 1e9 codes the grid is a multiple of 8, every tile has exactly one block, no block runs a tile that does not exist, a die's
consecutive blocks run consecutive tiles, and with the knob off the map is the identity."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_order_arithmetic_under_sanitizers(tmp_path):
    """no Python-loaded code runs under a sanitizer: the header is plain C++ and gets a main() of its own"""
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the driver; it must be here"
    exe = str(tmp_path / "setop_order_units")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
           "-I", os.path.join(ROOT, "unikmer_amd", "csrc"), os.path.join(ROOT, "tests", "setop_order_units.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.returncode, r.stdout, r.stderr)


def test_header_is_a_dependency_of_the_build():
    from unikmer_amd import build
    assert "ukm_setop_order.h" in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "ukm_setop_order.h"))
