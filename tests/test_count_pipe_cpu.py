"""The chunk pipeline of `count` without a device (unikmer_amd/host/count_pipe.hpp: the pipe between the reader thread and the
device thread, the handover of a file to the host parser, the two reader bodies, the double-buffered loop) as a stand-alone
two-thread program, tests/count_pipe_units.cpp: built once under the address and undefined-behaviour sanitizers and once under
the thread sanitizer, and run under a time limit -- a deadlock fails, it does not hang.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZERS = {"asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-fsanitize=thread"]}
CASES = ["raw reader", "handover at every position", "double-buffered loop", "parsing reader", "reader errors", "abandoned pipeline"]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """the program under each set of sanitizers, compiled side by side"""
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the driver; it must be here"
    d = tmp_path_factory.mktemp("count_pipe_units")
    procs = {}
    for name, flags in SANITIZERS.items():
        exe = str(d / ("count_pipe_units_" + name))
        cmd = [gxx, "-std=c++17", "-g", "-O0"] + flags + ["-I", os.path.join(ROOT, "unikmer_amd", "host"),
                                                         os.path.join(ROOT, "tests", "count_pipe_units.cpp"), "-o", exe, "-lz", "-pthread"]
        procs[name] = (exe, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    out = {}
    for name, (exe, p) in procs.items():
        _, err = p.communicate()
        assert p.returncode == 0, err
        out[name] = exe
    return out, d


@pytest.mark.parametrize("sanitizer", sorted(SANITIZERS))
def test_count_pipe_units(programs, sanitizer):
    exes, d = programs
    work = d / ("work_" + sanitizer)
    work.mkdir()
    r = subprocess.run([exes[sanitizer], str(work)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-4000:])
    assert r.stdout.splitlines() == ["OK " + c for c in CASES] + ["OK"], (r.stdout, r.stderr[-4000:])
