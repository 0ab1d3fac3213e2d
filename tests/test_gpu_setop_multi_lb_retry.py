"""The look-back watchdog's retry on the fused set-op kernel (ukm_setop2_multi), by the scheme of test_gpu_lb_retry.py:
ONE child process per library (tests/setop_multi_lb_driver.py with UKM_LIB_PATH set), each under a time limit, and nothing
more is started after a child that ended abnormally.

Seam library (libunikmer_hip_lbtest.so: every tile >= 1 with a blockIdx id gives its look-back up at once): the three-tile
union + inter + diff is bit-exact with the oracle although the first launch placed every tile as if nothing matched in
front of it; "lb_watchdogs" goes 0 -> 1 within the call -- a case whose injection did not fire FAILS --; the call repeats
exactly on the latched context; inputs and the guard words behind every out_cap are untouched.  Product library: the
same case is exact with "lb_watchdogs" 0.
"""
import json
import os
import subprocess
import sys

import pytest

import lb_retry_driver as D
import setop_multi_lb_driver as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = {"seam": os.path.join(ROOT, "unikmer_amd", "libunikmer_hip_lbtest.so"),
        "product": os.path.join(ROOT, "unikmer_amd", "libunikmer_hip.so")}
CHILD_TIMEOUT = 120     # seconds; a child takes a few
_stop = []              # why no further child is started (a child ended abnormally)


def _run_child(which, tmp_path_factory):
    if _stop:
        return {"abnormal": "not started: " + _stop[0], "record": None}
    out = str(tmp_path_factory.mktemp("setop_multi_lb_" + which) / "record.jsonl")
    env = dict(os.environ, UKM_LIB_PATH=LIBS[which])
    env.pop("UKM_FORCE_TICKET", None)
    abnormal = None
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "setop_multi_lb_driver.py"), out], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=CHILD_TIMEOUT)
        if p.returncode != 0:
            abnormal = "the %s child ended with status %d:\n%s" % (which, p.returncode, p.stderr.decode(errors="replace")[-4000:])
    except subprocess.TimeoutExpired as e:
        abnormal = "the %s child did not end within %d s:\n%s" % (which, CHILD_TIMEOUT, (e.stderr or b"").decode(errors="replace")[-4000:])
    record = None
    if os.path.exists(out):
        with open(out) as fh:
            for line in fh:
                record = json.loads(line)
    if abnormal:
        _stop.append(abnormal)
    return {"abnormal": abnormal, "record": record}


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    return _run_child("product", tmp_path_factory)


@pytest.fixture(scope="module")
def seam(tmp_path_factory):
    return _run_child("seam", tmp_path_factory)


def _check(run, marks):
    assert run["abnormal"] is None, run["abnormal"]
    r = run["record"]
    assert r is not None and r["name"] == M.NAME, "the child left no record of the case"
    assert r["error"] is None, r["error"]
    assert r["wd"] == marks, "[lb_watchdogs, ticket_latched] at the marks of the case"


def test_product_library(product):
    """the seam is compiled out: exact, and no watchdog ever fires"""
    _check(product, [list(D.QUIET)] * len(M.MARKS))


def test_seam_library(product, seam):
    """exact through the retry; the watchdog fired exactly once, in the first call"""
    assert M.MARKS == [list(D.QUIET), list(D.FIRED), list(D.FIRED)]
    _check(seam, M.MARKS)
