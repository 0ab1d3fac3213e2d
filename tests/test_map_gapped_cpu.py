"""ukm_map_gapped: what can be checked without a GPU -- the entry point exists in header, binding and library; and the closed
form the kernels implement (runs, chains, groups of X + 1 runs: include/unikmer_hip.h) is the state machine of map.go:298-490
with its per-record reset, on seeded random class streams (tests/map_model.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import map_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from unikmer_amd import build, lib
    build.build()
    return lib


def test_entry_point_declared_listed_exported(built):
    lib = built
    header = open(os.path.join(ROOT, "include", "unikmer_hip.h")).read()
    assert re.search(r"^int ukm_map_gapped\(ukm_ctx \*ctx,", header, re.M)
    assert "ukm_map_gapped" in lib.SYMBOLS
    assert hasattr(ctypes.CDLL(lib.SO_PATH), "ukm_map_gapped")
    assert callable(lib.Context.map_gapped)


def test_null_context_is_invalid(built):
    lib = built
    L = lib.load()
    n = ctypes.c_uint64()
    rc = L.ukm_map_gapped(None, None, None, 0, None, 0, 23, 0, 0, None, 0, 0, 200, 1, 1, None, None, None, 0, ctypes.byref(n))
    assert rc == lib.ERR_INVALID


N_CASES = 24_000


@pytest.fixture(scope="module")
def cases():
    """(circular, cls, lens, k, min_len, x, X) -- 1-3 records, k in {1,3,5}, x in 0..3, X in 0..3, min_len in {1,2,k,k+3,12},
    with and without multiple-mapped windows, linear and circular alternating"""
    rng = np.random.default_rng(20240607)
    return [(bool(i & 1),) + M.random_case(rng, bool(i & 1)) for i in range(N_CASES)]


def test_closed_form_is_the_state_machine(cases):
    regions = with_gaps = multi_run = 0
    for circ, cls, lens, k, min_len, x, X in cases:
        want = M.model_map_gapped(cls, lens, k, circ, min_len, x, X)
        assert M.regions_by_chains(cls, lens, k, circ, min_len, x, X) == want, (circ, cls, lens, k, min_len, x, X)
        regions += len(want)
        with_gaps += x > 0
        multi_run += any("M" in c[s:e - k] for r, s, e in want for c in [M.stream(cls[r], lens[r], k, circ)])
    # the cases are not trivial: regions exist, most calls allow gaps, many regions span a gap
    assert regions > N_CASES and with_gaps > N_CASES // 2 and multi_run > N_CASES // 10


def test_reset_and_drop_change_nothing_on_one_record_with_min_len_at_least_k(cases):
    """the two deviations from the reference are invisible where the reference has nothing to leak and nothing stale passes"""
    n = 0
    for circ, cls, lens, k, min_len, x, X in cases:
        if len(cls) != 1 or min_len < k:
            continue
        n += 1
        assert M.model_map_gapped(cls, lens, k, circ, min_len, x, X) == \
            M.model_map_gapped(cls, lens, k, circ, min_len, x, X, reset_per_record=False, drop_after_break=False)
    assert n > 1000


def test_the_leak_that_matters_and_the_stale_region():
    """the deviations, on the smallest inputs that show them"""
    # record 0 ends inside a tolerated gap (flag stays false): the reference then loses record 1's region
    cls, lens, k = ["GGM", "GGG"], [3, 3], 1
    assert M.model_map_gapped(cls, lens, k, False, 1, 1, 1) == [(0, 0, 2), (1, 0, 3)]
    assert M.model_map_gapped(cls, lens, k, False, 1, 1, 1, reset_per_record=False) == [(0, 0, 2)]
    # circular, min_len < k: behind the `break` the reference prints (start >= L, stale lastmatch + k)
    # (the stream is G M G G G G M G: the run 2..5 is longer than the record and clipped to 2 + L; the run at 7 >= L breaks)
    cls, lens, k = ["GMGGG"], [5], 3
    assert M.model_map_gapped(cls, lens, k, True, 1, 0, 0) == [(0, 0, 3), (0, 2, 7)]
    assert M.model_map_gapped(cls, lens, k, True, 1, 0, 0, drop_after_break=False) == [(0, 0, 3), (0, 2, 7), (0, 7, 8)]
