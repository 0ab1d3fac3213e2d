"""Models of `unikmer map` with -x / -X / --circular for the tests of ukm_map_gapped (a plain helper module).

Everything works on CLASSES: per record a string over G (code in the set, not multiple-mapped), B (in the set, multiple-mapped)
and M (not in the set) -- one letter per window, the L circular windows when circular -- or None for a record shorter than k.

  classes            G / B / M from the CPU oracle's kmer_iter / hash_iter: the three maps of map.go:116-284
  model_map_gapped   the loop of map.go:298-490 statement by statement; with both switches off it is the reference as it stands
  regions_by_chains  the closed form of include/unikmer_hip.h (runs, chains, groups of X + 1 runs), written independently
"""
import re

import numpy as np


def windows(O, bases, off, k, hashed=False, circular=False):
    """per record: the list of canonical window values, or None for a record shorter than k (sketches.ErrShortSeq)"""
    it = O.hash_iter if hashed else O.kmer_iter
    out = []
    for r in range(len(off) - 1):
        seq = bases[int(off[r]):int(off[r + 1])]
        out.append(it(seq, k, True, circular).tolist() if len(seq) >= k else None)
    return out


def classes(wins, genome_of, codes, allow_multi):
    """wins: windows(...) (circular ones when the call is circular: pass 1 counts among exactly these, map.go:222-226);
    genome_of[r] = genome of record r, the same numbering in both passes (tests/test_gpu_map.py)"""
    m = set(codes)
    m2 = {}
    if not allow_multi:
        for r, w in enumerate(wins):
            if w is None:
                continue
            g = m2.setdefault(genome_of[r], {})
            for code in w:
                if code not in g:
                    g[code] = False
                elif not g[code]:
                    g[code] = True
    out = []
    for r, w in enumerate(wins):
        if w is None:
            out.append(None)
            continue
        g = m2.get(genome_of[r], {})
        out.append("".join("M" if c not in m else ("B" if g.get(c, False) else "G") for c in w))
    return out


def stream(cls, L, k, circular):
    """the classes of the windows the second pass iterates over: the record written twice when circular (map.go:338-340)"""
    if not circular:
        assert len(cls) == L - k + 1
        return cls
    assert len(cls) == L
    return (cls + cls)[:2 * L - k + 1]


def model_map_gapped(cls, lens, k, circular, min_len, max_gap_size, max_gap_num, reset_per_record=True, drop_after_break=True):
    """map.go:298-490.  cls[r] / lens[r]: classes and length of record r.  reset_per_record: `flag`, `lastGapNum` and
    `lastmatch` start every record as they start the first; drop_after_break: nothing is emitted behind the circular `break`."""
    out = []
    last_gap_num = lastmatch = 0
    flag = True

    def emit(r, start, lastmatch, length0):
        if circular and lastmatch - start + k > length0:
            lastmatch = length0 - k + start
        out.append((r, start, lastmatch + k))

    for r, c_r in enumerate(cls):
        if c_r is None:
            continue
        length0 = lens[r]
        if reset_per_record:
            last_gap_num = lastmatch = 0
            flag = True
        c, start, gaps, gap_nums = 0, -1, 0, 0
        broke = False
        for i, sym in enumerate(stream(c_r, length0, k, circular)):
            if sym != "M":
                gaps = 0
                if sym == "B":
                    if last_gap_num <= max_gap_num and start >= 0 and lastmatch - start + k >= min_len:
                        emit(r, start, lastmatch, length0)
                    c, start, flag = 0, -1, True
                else:
                    c += 1
                    if c == 1 and flag:
                        start, gap_nums, gaps, last_gap_num = i, 0, 0, 0
                        if circular and start >= length0:
                            broke = True
                            break
                if c >= 1:
                    lastmatch, last_gap_num = i, gap_nums
            else:
                gaps += 1
                if gaps == 1:
                    gap_nums += 1
                if gaps <= max_gap_size and gap_nums <= max_gap_num:
                    c = 0
                    if start >= 0:
                        flag = False
                else:
                    if last_gap_num <= max_gap_num and start >= 0 and lastmatch - start + k >= min_len:
                        emit(r, start, lastmatch, length0)
                    c, start, flag = 0, -1, True
        if broke and drop_after_break:
            continue
        if last_gap_num <= max_gap_num + 1 and start >= 0 and lastmatch - start + k >= min_len:
            emit(r, start, lastmatch, length0)
    return out


def regions_by_chains(cls, lens, k, circular, min_len, max_gap_size, max_gap_num):
    """runs -> chains -> groups of max_gap_num + 1 runs (include/unikmer_hip.h, ukm_map_gapped)"""
    out = []
    group = (max_gap_num if max_gap_size else 0) + 1
    for r, c_r in enumerate(cls):
        if c_r is None:
            continue
        L = lens[r]
        s = stream(c_r, L, k, circular)
        runs = [(m.start(), m.end() - 1) for m in re.finditer("G+", s)]
        chains = []
        for j, (a, b) in enumerate(runs):
            sep = s[runs[j - 1][1] + 1:a] if j else None
            if sep is not None and "B" not in sep and len(sep) <= max_gap_size:
                chains[-1].append((a, b))
            else:
                chains.append([(a, b)])
        for ch in chains:
            for g in range(0, len(ch), group):
                start, last = ch[g][0], ch[min(g + group, len(ch)) - 1][1]
                if last - start + k < min_len:
                    continue
                if not circular:
                    out.append((r, start, last + k))
                elif start < L:
                    out.append((r, start, start + L if last - start + k > L else last + k))
    return out


def random_case(rng, circular):
    """one seeded symbol stream case: 1-3 records; returns (cls, lens, k, min_len, x, X)"""
    k = int(rng.choice([1, 3, 5]))
    x = int(rng.integers(0, 4))
    X = int(rng.integers(1 if x else 0, 4))    # (x > 0 with X = 0 is refused, map.go:112)
    min_len = int(rng.choice([1, 2, k, k + 3, 12]))
    with_b = rng.random() < 0.5
    p = np.array([0.6, 0.1 if with_b else 0.0, 0.3])
    p = p / p.sum()
    cls, lens = [], []
    for _ in range(int(rng.integers(1, 4))):
        nw = int(rng.integers(1, 40))
        L = max(nw, k) if circular else nw + k - 1
        n = L if circular else nw
        if rng.random() < 0.1:                 # a record shorter than k
            cls.append(None)
            lens.append(k - 1)
            continue
        cls.append("".join(rng.choice(list("GBM"), size=n, p=p)))
        lens.append(L)
    return cls, lens, k, min_len, x, X
