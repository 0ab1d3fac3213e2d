"""Similarity of many k-mer sets from one Context.pair_counts call: pure functions on (counts, sizes), and
`python -m unikmer_amd.similarity [--metric count|jaccard|containment|mash] [--rows R] a.unik b.unik ...`, which prints the
matrix as TSV.

counts[i][j] is the number of distinct codes sets i and j share (i < rows, j < n), sizes[j] the number of distinct codes of
set j; row i of counts belongs to set i, so the first `rows` entries of sizes are the row sets' sizes."""
import argparse
import os
import sys

import numpy as np


def _as_float(counts, sizes):
    c = np.asarray(counts).astype(np.float64)
    s = np.asarray(sizes).astype(np.float64)
    if c.ndim != 2 or s.ndim != 1 or c.shape[1] != len(s) or c.shape[0] > len(s):
        raise ValueError("counts must be (rows, n) and sizes (n,) with rows <= n")
    return c, s


def jaccard(counts, sizes):
    """J[i][j] = c / (s_i + s_j - c).  Two empty sets give 0/0: that is 1.0 on the diagonal (a set and itself) and 0.0
    elsewhere (two different empty sets share nothing)."""
    c, s = _as_float(counts, sizes)
    union = s[: c.shape[0], None] + s[None, :] - c
    out = np.zeros_like(c)
    np.divide(c, union, out=out, where=union > 0)
    r = np.arange(c.shape[0])
    out[r, r] = np.where(union[r, r] > 0, out[r, r], 1.0)
    return out


def containment(counts, sizes):
    """C[i][j] = c / s_i: the share of set i that set j holds.  An empty set i gives 0/0: 1.0 on the diagonal, 0.0 elsewhere,
    as for jaccard."""
    c, s = _as_float(counts, sizes)
    si = np.broadcast_to(s[: c.shape[0], None], c.shape)
    out = np.zeros_like(c)
    np.divide(c, si, out=out, where=si > 0)
    r = np.arange(c.shape[0])
    out[r, r] = np.where(si[r, r] > 0, out[r, r], 1.0)
    return out


def mash_distance(j, k):
    """D = -ln(2 j / (1 + j)) / k for a Jaccard index j (array or number) of k-mers; j == 0 gives 1.0.  Values are clipped
    to [0, 1] as Mash does."""
    j = np.asarray(j, dtype=np.float64)
    out = np.ones_like(j)
    pos = j > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        np.divide(-np.log(np.where(pos, 2.0 * j / (1.0 + j), 1.0)), float(k), out=out, where=pos)
    return np.clip(out, 0.0, 1.0)


METRICS = ("count", "jaccard", "containment", "mash")


def matrix(metric, counts, sizes, k):
    if metric == "count":
        return np.asarray(counts)
    if metric == "jaccard":
        return jaccard(counts, sizes)
    if metric == "containment":
        return containment(counts, sizes)
    if metric == "mash":
        return mash_distance(jaccard(counts, sizes), k)
    raise ValueError("unknown metric %r" % (metric,))


def check_compatible(paths, headers):
    """every file must have the k, the canonical / hashed / scaled flags and the scale of the first; raises ValueError naming
    the two files otherwise"""
    from . import unikfile
    mask = unikfile.CANONICAL | unikfile.HASHED | unikfile.SCALED

    what = ("k", "canonical/hashed/scaled flags", "scale")

    def sig(h):
        return h["k"], h["flag"] & mask, (h["scale"] if h["flag"] & unikfile.SCALED else 0)
    first = sig(headers[0])
    for p, h in zip(paths[1:], headers[1:]):
        for name, x, y in zip(what, first, sig(h)):
            if x != y:
                raise ValueError("%s and %s differ in %s (%s vs %s): their codes cannot be compared" % (paths[0], p, name, x, y))


def format_tsv(names, row_names, m):
    integer = np.issubdtype(np.asarray(m).dtype, np.integer)
    lines = ["\t".join([""] + list(names))]
    for name, row in zip(row_names, m):
        lines.append("\t".join([name] + [str(int(v)) if integer else "%.6g" % v for v in row]))
    return "\n".join(lines) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m unikmer_amd.similarity", description="all-pairs similarity of .unik files as a TSV matrix")
    ap.add_argument("--metric", choices=METRICS, default="count")
    ap.add_argument("--rows", type=int, default=None, help="only the first R files as rows (queries against all files)")
    ap.add_argument("files", nargs="+")
    a = ap.parse_args(argv)
    from . import lib, unikfile
    try:
        headers = [unikfile.read_header(p) for p in a.files]
        check_compatible(a.files, headers)
    except (ValueError, OSError) as e:
        sys.stderr.write("error: %s\n" % e)
        return 1
    ctx = lib.Context(0)
    try:
        keys = [unikfile.load(ctx, p, device=True, ignore_taxid=True)[1] for p in a.files]
        counts, sizes = ctx.pair_counts(keys, rows=a.rows)
    finally:
        ctx.close()
    names = [os.path.basename(p) for p in a.files]
    sys.stdout.write(format_tsv(names, names[: counts.shape[0]], matrix(a.metric, counts, sizes, headers[0]["k"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
