"""Model of ukm_screen for its tests (a plain helper module).

  windows       per record the window values from the CPU oracle's kmer_iter / hash_iter, [] for a record shorter than k
  first_taxids  the set as a dict code -> taxid of the code's FIRST copy (what a lower bound finds)
  fold_lca      the definition: the LEFT FOLD of the oracle's pairwise LCA over a record's hit taxids, in window order
  closed_lca    the closed form of include/unikmer_hip.h, written independently of the fold from plain parent / merged dicts
  screen        (win, hit, lca) per record through the fold
"""
import numpy as np


def windows(O, bases, off, k, canonical=True, circular=False, hashed=False):
    it = O.hash_iter if hashed else O.kmer_iter
    out = []
    for r in range(len(off) - 1):
        seq = bases[int(off[r]):int(off[r + 1])]
        out.append(it(seq, k, canonical, circular).tolist() if len(seq) >= k else [])
    return out


def first_taxids(set_keys, set_taxids=None):
    m = {}
    for i, c in enumerate(np.asarray(set_keys).tolist()):
        if c not in m:
            m[c] = 0 if set_taxids is None else int(set_taxids[i])
    return m


def fold_lca(tax, hits):
    """tax: oracle.Taxonomy; hits: the taxids of a record's hit windows in window order"""
    if not hits:
        return 0
    acc = hits[0]
    for t in hits[1:]:
        acc = tax.lca(acc, t)
    return acc


class Forest:
    """parent / merged as plain dicts, for the closed form"""

    def __init__(self, child, parent, merged_old=(), merged_new=()):
        self.parent = {}
        for c, p in zip(child, parent):
            self.parent[int(c)] = int(p)
        for p in list(self.parent.values()):
            self.parent.setdefault(p, p)     # a parent that is nobody's child is a root of its own
        self.merged = {int(o): int(n) for o, n in zip(merged_old, merged_new)}

    def resolve(self, t):
        """the node a taxid stands for, or None (taxid 0, unknown ids, merged ids whose target is unknown)"""
        if t == 0:
            return None
        if t in self.parent:
            return t
        m = self.merged.get(t, 0)
        return m if m in self.parent else None

    def path(self, t):
        """root ... t"""
        p = [t]
        while self.parent[p[-1]] != p[-1]:
            p.append(self.parent[p[-1]])
        return p[::-1]

    def lca_set(self, nodes):
        paths = [self.path(t) for t in nodes]
        last = 0
        for level in zip(*paths):
            if any(x != level[0] for x in level):
                break
            last = level[0]
        return last


def closed_lca(forest, hits):
    if not hits:
        return 0
    if all(t == hits[0] for t in hits):
        return hits[0]
    nodes = [forest.resolve(t) for t in set(hits)]
    if any(n is None for n in nodes):
        return 0
    return forest.lca_set(nodes)


def screen(wins, member, tax=None):
    """wins: windows(...); member: first_taxids(...); tax: oracle.Taxonomy or None.  Returns (win, hit, lca or None)."""
    win = np.array([len(w) for w in wins], dtype=np.uint32)
    hit = np.zeros(len(wins), dtype=np.uint32)
    lca = np.zeros(len(wins), dtype=np.uint32) if tax is not None else None
    for r, w in enumerate(wins):
        hits = [member[c] for c in w if c in member]
        hit[r] = len(hits)
        if tax is not None:
            lca[r] = fold_lca(tax, hits)
    return win, hit, lca


def random_forest(rng, n_nodes=60, max_depth=20):
    """two trees with depth up to max_depth over ids 1 .. n_nodes (some ids left out: absent), merged ids above them (some
    pointing at absent targets).  Returns (child, parent, merged_old, merged_new, pool) with pool = the taxids a test draws
    from: nodes, merged, absent and unknown ids, and 0."""
    ids = rng.permutation(np.arange(1, n_nodes + 1))
    absent = [int(x) for x in ids[: n_nodes // 6]]
    nodes = [int(x) for x in ids[n_nodes // 6:]]
    roots = nodes[:2]
    depth = {roots[0]: 0, roots[1]: 0}
    child, parent = list(roots), list(roots)
    placed = list(roots)
    chain = roots[0]
    for t in nodes[2:]:
        if depth[chain] < max_depth and rng.random() < 0.4:
            p = chain                    # one long chain, so that deep nodes exist
        else:
            cand = [x for x in placed if depth[x] < max_depth]
            p = cand[int(rng.integers(0, len(cand)))]
        depth[t] = depth[p] + 1
        if p == chain:
            chain = t
        child.append(t)
        parent.append(p)
        placed.append(t)
    m_old = list(range(n_nodes + 1, n_nodes + 9))
    m_new = [nodes[int(rng.integers(0, len(nodes)))] for _ in m_old[:-2]] + [absent[0], n_nodes + 50]
    pool = nodes + m_old + absent[:3] + [n_nodes + 100, 0]
    return (np.array(child, dtype=np.uint32), np.array(parent, dtype=np.uint32), np.array(m_old, dtype=np.uint32),
            np.array(m_new, dtype=np.uint32), pool)
