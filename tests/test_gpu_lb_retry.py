"""The look-back watchdog's retry, on every kernel that has one (ukm_lb_launch in ukm_ctx.hip,
fold_chained in ukm_nway.hip).

A tile whose predecessor does not publish gives up, writes at a wrong base and raises a flag; the host repeats the launch
with ticketed tile ids and keeps the context on tickets.  No device here dispatches workgroups out of order, so the
suite reaches that path through a second library, libunikmer_hip_lbtest.so (unikmer_amd/build.py), whose look-back
gives up at once in every tile >= 1 that took its id from blockIdx (UKM_LB_TEST_TIMEOUT in ukm_device.h).  lib.py reads
UKM_LIB_PATH when it is imported, so each library gets ONE child process (tests/lb_retry_driver.py), which runs every case
on a fresh Context and leaves a JSON line per case; every test here asserts on its own line.

Against the seam library every case must be bit-exact with the CPU oracle although its first launch wrote every tile
at base 0, must show "lb_watchdogs" going 0 -> 1 in the call (a case whose injection did not fire FAILS: its shape fell to
one tile or to another route), must repeat exactly on the latched context, and must leave its inputs and the guard words
behind out_cap untouched.  Against the product library the same cases are exact with "lb_watchdogs" 0: the seam is
compiled out.  Not reached by this: a real out-of-order dispatch, a timeout in only some tiles, a timeout in the rank
re-run, and the TABLE pass (no look-back).
"""
import json
import os
import subprocess
import sys
import time

import pytest

import lb_retry_driver as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = {"seam": os.path.join(ROOT, "unikmer_amd", "libunikmer_hip_lbtest.so"),
        "product": os.path.join(ROOT, "unikmer_amd", "libunikmer_hip.so")}
CHILD_TIMEOUT = 300     # seconds; a child takes a few
_stop = []              # why no further child is started (a child ended abnormally)


def _run_child(which, tmp_path_factory):
    if _stop:
        return {"abnormal": "not started: " + _stop[0], "records": {}}
    out = str(tmp_path_factory.mktemp("lb_retry_" + which) / "records.jsonl")
    env = dict(os.environ, UKM_LIB_PATH=LIBS[which])
    env.pop("UKM_FORCE_TICKET", None)
    t0 = time.time()
    abnormal = None
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lb_retry_driver.py"), out], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT)
        if p.returncode != 0:
            abnormal = "the %s child ended with status %d:\n%s" % (which, p.returncode, p.stderr.decode(errors="replace")[-4000:])
    except subprocess.TimeoutExpired as e:
        abnormal = "the %s child did not end within %d s:\n%s" % (which, CHILD_TIMEOUT, (e.stderr or b"").decode(errors="replace")[-4000:])
    records = {}
    if os.path.exists(out):
        with open(out) as fh:
            for line in fh:
                r = json.loads(line)
                records[r["name"]] = r
    if abnormal:
        _stop.append(abnormal)
    print("lb_retry %s child: %.1f s, %d cases, slowest %s" % (
        which, time.time() - t0, len(records), sorted(((r["seconds"], n) for n, r in records.items()), reverse=True)[:3]))
    return {"abnormal": abnormal, "records": records}


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    return _run_child("product", tmp_path_factory)


@pytest.fixture(scope="module")
def seam(tmp_path_factory):
    return _run_child("seam", tmp_path_factory)


def _check(run, name, is_seam):
    assert run["abnormal"] is None, run["abnormal"]
    assert name in run["records"], "the child left no record of this case"
    r = run["records"][name]
    assert r["error"] is None, r["error"]
    assert r["wd"] == D.expected(name, is_seam), "[lb_watchdogs, ticket_latched] at the marks of the case"


@pytest.mark.parametrize("name", D.NAMES)
def test_product_library(product, name):
    """the seam is compiled out: exact, and no watchdog ever fires"""
    _check(product, name, False)


@pytest.mark.parametrize("name", D.NAMES)
def test_seam_library(product, seam, name):
    """exact through the retry; the watchdog fired exactly once, in the first call"""
    _check(seam, name, True)


def test_the_seam_fires_where_a_look_back_runs():
    """what the cases expect of the seam library: a watchdog in every case but the controls"""
    quiet = [n for n in D.NAMES if D.expected(n, True)[-1] == list(D.QUIET)]
    assert quiet == ["unique-in-place", "nthash-unfiltered", "encode_kmers", "sample"]
