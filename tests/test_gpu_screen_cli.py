"""`python -m unikmer_amd.screen` and screen_file on the GPU: a small set written with unikfile.save (with and without taxids),
FASTA / FASTQ / gzip reads in tmp_path, the TSV compared with tests/screen_model.py."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import screen_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
K = 21


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """sets, reads, the taxonomy directory and the model's rows (index, name, length, win, hit, lca)"""
    from unikmer_amd import lib, unikfile
    from oracle import oracle as O
    d = tmp_path_factory.mktemp("screen")
    rng = np.random.default_rng(5)
    child, parent, m_old, m_new, pool = M.random_forest(rng)
    (d / "nodes.dmp").write_text("".join("%d\t|\t%d\t|\tno rank\t|\n" % (c, p) for c, p in zip(child, parent)))
    (d / "merged.dmp").write_text("".join("%d\t|\t%d\t|\n" % (o, n) for o, n in zip(m_old, m_new)))
    lens = rng.integers(15, 400, 300)
    lens[[3, 50, 299]] = [0, K - 1, K]
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(off[-1]))].copy()
    seqs = [bases[int(off[r]):int(off[r + 1])].tobytes().decode() for r in range(len(lens))]
    names = ["read%d" % r for r in range(len(lens))]
    fa = "".join(">%s some description\n%s" % (n, "".join(s[i:i + 60] + "\n" for i in range(0, len(s), 60)) or "\n") for n, s in zip(names, seqs))
    fq = "".join("@%s\tx\n%s\n+\n%s\n" % (n, s, "I" * len(s)) for n, s in zip(names, seqs))
    (d / "reads.fa").write_text(fa)
    (d / "reads.fq").write_text(fq)
    with gzip.open(d / "reads.fa.gz", "wb") as f:
        f.write(fa.encode())
    wins = M.windows(O, bases, off, K)
    allc = np.unique(np.array([c for w in wins for c in w], dtype=np.uint64))
    keys = allc[rng.random(len(allc)) < 0.3]
    tx = np.array([pool[int(i)] for i in rng.integers(0, len(pool), len(keys))], dtype=np.uint32)
    ctx = lib.Context(0)
    try:
        flag = unikfile.CANONICAL | unikfile.SORTED | unikfile.COMPACT
        unikfile.save(ctx, str(d / "plain.unik"), {"k": K, "flag": flag}, keys)
        unikfile.save(ctx, str(d / "taxed.unik"), {"k": K, "flag": flag | unikfile.INCLUDE_TAXID}, keys, tx)
    finally:
        ctx.close()
    tax = O.Taxonomy(child, parent, m_old, m_new)
    win, hit, lca = M.screen(wins, M.first_taxids(keys, tx), tax)
    rows = [(r, names[r], int(lens[r]), int(win[r]), int(hit[r]), int(lca[r])) for r in range(len(lens))]
    return d, rows


def _tsv(rows, with_lca, keep=lambda r: True):
    head = ["index", "name", "length", "windows", "hits", "fraction"] + (["lca"] if with_lca else [])
    out = ["\t".join(head)]
    for r in rows:
        if keep(r):
            cols = [str(r[0]), r[1], str(r[2]), str(r[3]), str(r[4]), "%.6g" % (r[4] / r[3] if r[3] else 0.0)]
            out.append("\t".join(cols + ([str(r[5])] if with_lca else [])))
    return "\n".join(out) + "\n"


def _cli(*args):
    p = subprocess.run([sys.executable, "-m", "unikmer_amd.screen"] + [str(a) for a in args], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return p.stdout


def _main(capsys, *args):
    """the same entry point inside this process (a child process costs seconds of start-up: two tests below pay for one each)"""
    from unikmer_amd import screen
    assert screen.main([str(a) for a in args]) == 0
    return capsys.readouterr().out


def test_cli_plain_set(files, capsys):
    d, rows = files
    assert _cli(d / "plain.unik", d / "reads.fa.gz") == _tsv(rows, False)
    assert _main(capsys, d / "plain.unik", d / "reads.fa") == _tsv(rows, False)
    assert _main(capsys, "-n", 5, d / "plain.unik", d / "reads.fq") == _tsv(rows, False, lambda r: r[3] > 0 and r[4] >= 5)


def test_cli_taxed_set_and_filters(files, capsys):
    d, rows = files
    got = _cli("--data-dir", d, "-f", 0.25, "-n", 3, d / "taxed.unik", d / "reads.fq")
    assert got == _tsv(rows, True, lambda r: r[3] > 0 and r[4] >= 3 and r[4] / r[3] >= 0.25)
    assert 1 < got.count("\n") < len(rows)
    assert _main(capsys, "--data-dir", d, d / "taxed.unik", d / "reads.fa.gz") == _tsv(rows, True)
    assert _main(capsys, "--data-dir", d, "-f", 0, d / "taxed.unik", d / "reads.fa") == _tsv(rows, True, lambda r: r[3] > 0 and r[4] >= 1)


def test_screen_file_chunks(files):
    from unikmer_amd import lib, screen
    d, rows = files
    ctx = lib.Context(0)
    try:
        screen.load_taxdump(ctx, str(d))
        for name in ("reads.fa", "reads.fq", "reads.fa.gz"):
            whole = list(screen.screen_file(ctx, str(d / "taxed.unik"), str(d / name)))
            small = list(screen.screen_file(ctx, str(d / "taxed.unik"), str(d / name), chunk_bytes=1024))
            assert whole == rows and small == rows, name
        plain = list(screen.screen_file(ctx, str(d / "plain.unik"), str(d / "reads.fa"), chunk_bytes=1024))
        assert plain == [r[:5] + (None,) for r in rows]
        (d / "bad.fa").write_text(">a\nACGT\n>b\nACGT\n")
        with open(d / "bad.fa", "r+b") as f:
            f.write(b"xx")            # a line in front of the first header
        with pytest.raises(ValueError, match="byte 0"):
            list(screen.screen_file(ctx, str(d / "plain.unik"), str(d / "bad.fa")))
    finally:
        ctx.close()
