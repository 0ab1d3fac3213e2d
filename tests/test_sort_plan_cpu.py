"""The radix sort's host decisions without a GPU: unikmer_amd/csrc/ukm_sort_plan.h and ukm_sort_state.h are plain C++, and
tests/sort_plan_units.cpp runs it as a stand-alone program under the address and undefined-behaviour sanitizers: the bucket
route's plan over every power of two from 2^23 to 2^32 - 1 and its neighbours, the admission test against what
ukm_sort_first_shift answers for every key width, knob and state, the size classes over every bucket size up to 4097, the
route choice at every threshold, and the counting-step policy a context keeps from one sort to the next."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sort_plan_under_sanitizers(tmp_path):
    """no Python-loaded code runs under a sanitizer: the header is plain C++ and gets a main() of its own"""
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the driver; it must be here"
    exe = str(tmp_path / "sort_plan_units")
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
           "-I", os.path.join(ROOT, "unikmer_amd", "csrc"), os.path.join(ROOT, "tests", "sort_plan_units.cpp"), "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.returncode, r.stdout, r.stderr)


def test_headers_are_dependencies_of_the_build():
    from unikmer_amd import build
    for h in ("ukm_sort_state.h", "ukm_sort_plan.h", "ukm_sort_kernels.h", "ukm_sort_buckets.h"):
        assert h in build.HEADERS
        assert os.path.exists(os.path.join(build.CSRC, h))
