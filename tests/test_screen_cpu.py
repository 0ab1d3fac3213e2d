"""ukm_screen without a GPU: the argument that lets the kernel keep five integers per record -- the left fold of the pairwise
LCA contract over a record's hit taxids equals the closed form of include/unikmer_hip.h -- on random forests, and the plain
numpy of unikmer_amd/screen.py."""
import numpy as np
import pytest

import screen_model as M


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.mark.parametrize("seed", range(6))
def test_fold_equals_closed_form(O, seed):
    """two trees, depth up to 20, merged ids (also onto absent targets), absent and unknown ids, taxid 0; 60 records a forest"""
    rng = np.random.default_rng(1000 + seed)
    child, parent, m_old, m_new, pool = M.random_forest(rng)
    tax = O.Taxonomy(child, parent, m_old, m_new)
    forest = M.Forest(child, parent, m_old, m_new)
    depth = max(len(forest.path(int(t))) - 1 for t in child)
    assert depth >= 8 and sum(1 for c, p in zip(child, parent) if c == p) == 2
    nodes = [t for t in pool if forest.resolve(t) is not None]
    bad = [t for t in pool if forest.resolve(t) is None]
    seen = set()
    for case in range(60):
        n = int(rng.integers(1, 9))
        kind = case % 6
        if kind == 0:      # valid ids only
            hits = [nodes[int(i)] for i in rng.integers(0, len(nodes), n)]
        elif kind == 1:    # all one id, also an unknown one, a merged one, 0
            hits = [pool[int(rng.integers(0, len(pool)))]] * n
        elif kind == 2:    # one bad id among valid ones, at any place
            hits = [nodes[int(i)] for i in rng.integers(0, len(nodes), n)]
            hits.insert(int(rng.integers(0, n + 1)), bad[int(rng.integers(0, len(bad)))])
        elif kind == 3:    # a merged id and its target, repeated
            j = int(rng.integers(0, len(m_old) - 2))
            hits = [int(m_old[j]), int(m_new[j])] * (1 + n // 2)
            if rng.random() < 0.5:
                hits = hits[::-1]
        elif kind == 4:    # a run of one unknown id, then something else
            hits = [bad[int(rng.integers(0, len(bad)))]] * n + [pool[int(rng.integers(0, len(pool)))]]
        else:              # anything
            hits = [pool[int(i)] for i in rng.integers(0, len(pool), n)]
        got, want = M.fold_lca(tax, hits), M.closed_lca(forest, hits)
        assert got == want, (seed, case, hits, got, want)
        seen.add("zero" if got == 0 else "same" if all(h == hits[0] for h in hits) else "lca")
    assert seen == {"zero", "same", "lca"}


def test_closed_form_by_hand(O):
    #      1            7
    #    2   3          8
    #   4 5
    child, parent = [1, 2, 3, 4, 5, 7, 8], [1, 1, 1, 2, 2, 7, 7]
    f = M.Forest(child, parent, [20, 21], [4, 99])
    tax = O.Taxonomy(np.array(child, dtype=np.uint32), np.array(parent, dtype=np.uint32), np.array([20, 21], dtype=np.uint32),
                     np.array([4, 99], dtype=np.uint32))
    for hits, want in [([4, 5], 2), ([4, 3], 1), ([4, 8], 0), ([20, 20], 20), ([20, 4], 4), ([4, 20], 4), ([20, 5], 2),
                       ([21, 21, 21], 21), ([21, 4], 0), ([55, 55], 55), ([55, 4], 0), ([0, 0], 0), ([4, 0, 4], 0), ([4], 4), ([], 0),
                       ([4, 5, 3, 2], 1), ([8, 8, 7], 7)]:
        assert M.closed_lca(f, hits) == want, hits
        assert M.fold_lca(tax, hits) == want, hits


def test_fraction_and_select():
    from unikmer_amd import screen
    win = np.array([0, 10, 10, 4, 1, 0], dtype=np.uint32)
    hit = np.array([0, 0, 5, 4, 1, 0], dtype=np.uint32)
    fr = screen.fraction(win, hit)
    assert fr.dtype == np.float64 and fr.tolist() == [0.0, 0.0, 0.5, 1.0, 1.0, 0.0]
    assert screen.select(win, hit).tolist() == [False, False, True, True, True, False]
    assert screen.select(win, hit, min_hits=0).tolist() == [False, True, True, True, True, False]   # win == 0 is never kept
    assert screen.select(win, hit, min_frac=0.5).tolist() == [False, False, True, True, True, False]   # equality keeps
    assert screen.select(win, hit, min_frac=0.5000001).tolist() == [False, False, False, True, True, False]
    assert screen.select(win, hit, min_hits=4).tolist() == [False, False, True, True, False, False]    # equality keeps
    assert screen.select(win, hit, min_hits=5).tolist() == [False, False, True, False, False, False]
    assert screen.select(win, hit, min_frac=1.0, min_hits=2).tolist() == [False, False, False, True, False, False]
    assert screen.select([], []).tolist() == [] and screen.fraction([], []).tolist() == []


def test_symbol_is_declared_and_bound():
    import os
    import re
    from unikmer_amd import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "unikmer_hip.h")).read()
    assert re.search(r"\bint\s+ukm_screen\s*\(", hdr)
    assert "ukm_screen" in lib.SYMBOLS and hasattr(lib.load(), "ukm_screen")
    L = lib.load()
    assert L.ukm_screen(None, None, None, 0, 21, 1, 0, 0, None, None, 0, None, None, None) == lib.ERR_INVALID   # NULL ctx
