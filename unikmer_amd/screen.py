"""Which records belong to a k-mer set: pure functions on the (win, hit) arrays of one Context.screen call, a reader that
screens a FASTA/Q file chunk by chunk against a `.unik` file, and
`python -m unikmer_amd.screen [-f MIN_FRAC] [-n MIN_HITS] [--data-dir DIR] set.unik reads.fa`, which prints one TSV row per
record: index, name, length, windows, hits, fraction and -- when the set carries taxids -- the LCA of the hits' taxids
(the taxonomy: DIR/nodes.dmp and, when present, DIR/merged.dmp).  With -f or -n only the kept records are printed.

win[r] is the number of windows (k-mers) of record r, hit[r] the number of them whose value is in the set."""
import argparse
import gzip
import os
import sys

import numpy as np


def fraction(win, hit):
    """hit / win as float64; 0 where a record has no window"""
    w = np.asarray(win).astype(np.float64)
    h = np.asarray(hit).astype(np.float64)
    out = np.zeros_like(w)
    np.divide(h, w, out=out, where=w > 0)
    return out


def select(win, hit, min_frac=0.0, min_hits=1):
    """boolean keep mask: at least min_hits hits and a fraction of at least min_frac; a record without windows is never kept"""
    w = np.asarray(win).astype(np.int64)
    h = np.asarray(hit).astype(np.int64)
    # (compared on the float64 quotient fraction() returns: a threshold equal to a record's fraction keeps it)
    return (w > 0) & (h >= int(min_hits)) & (fraction(w, h) >= float(min_frac))


def load_taxdump(ctx, data_dir):
    """loads <data_dir>/nodes.dmp (and merged.dmp when it is there) into the context: the first two `|`-separated columns"""
    def pairs(path):
        a, b = [], []
        with open(path) as f:
            for line in f:
                cols = line.split("|")
                if len(cols) >= 2 and cols[0].strip():
                    a.append(int(cols[0]))
                    b.append(int(cols[1]))
        return np.array(a, dtype=np.uint32), np.array(b, dtype=np.uint32)
    child, parent = pairs(os.path.join(data_dir, "nodes.dmp"))
    merged = os.path.join(data_dir, "merged.dmp")
    old, new = pairs(merged) if os.path.exists(merged) else (None, None)
    if old is not None and len(old) == 0:
        old, new = None, None
    ctx.taxonomy_load(child, parent, old, new)


def _open(path):
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    return gzip.open(path, "rb") if gz else open(path, "rb")


def _name(text, at):
    """the first word behind the '>' / '@' at text[at]"""
    end = at + 1
    n = len(text)
    while end < n and text[end] not in b" \t\r\n":
        end += 1
    return bytes(text[at + 1:end]).decode("latin-1")


def screen_file(ctx, set_path, fastx_path, chunk_bytes=1 << 28):
    """yields (index, name, length, win, hit, lca) per record of a FASTA/Q file (plain or gzip), screened against the set of a
    `.unik` file: k and the canonical / hashed flags come from its header, and the taxids if its records carry them (lca is
    None otherwise; with taxids the context needs a loaded taxonomy).  The text is read in chunks of chunk_bytes, parsed by
    Context.fastx, and the incomplete record at a chunk's end is carried into the next one.  Text outside the device's
    grammar raises ValueError with the byte offset."""
    from . import lib, unikfile
    h, keys, taxids = unikfile.load(ctx, set_path, device=True)
    k = h["k"]
    canonical = bool(h["flag"] & unikfile.CANONICAL)
    hashed = bool(h["flag"] & unikfile.HASHED)
    if not h["flag"] & unikfile.SORTED:
        if taxids is not None:
            keys, taxids = ctx.sort_pairs(keys, taxids)
        else:
            keys = ctx.sort_u64(keys)
    import torch
    index = 0
    done = 0           # bytes of the file in front of `tail`
    tail = b""
    fastq = None
    with _open(fastx_path) as f:
        eof = False
        while not eof:
            more = f.read(int(chunk_bytes))
            eof = len(more) < int(chunk_bytes)
            if not eof:   # (a file that ends exactly on a chunk: the next read says so)
                peek = f.read(1)
                eof = peek == b""
                more += peek
            text = tail + more
            if fastq is None:
                if not text:
                    return
                first = text.split(b"\n", 1)[0]
                fastq = first[:1] == b"@"
            if not text:
                break
            t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
            bases, rec_off, hdr_off, consumed, stop = ctx.fastx(t, fastq=fastq, last=eof)
            if stop == lib.FASTX_STOP_GRAMMAR or (eof and stop != lib.FASTX_STOP_NONE):
                raise ValueError("%s: text outside the FASTA/Q grammar at byte %d" % (fastx_path, done + consumed))
            if consumed == 0 and not eof and len(more) == 0:
                raise ValueError("%s: no progress at byte %d" % (fastx_path, done))
            n_rec = int(hdr_off.numel())
            if n_rec:
                win, hit, lca = ctx.screen(bases, rec_off, k, keys, set_taxids=taxids, canonical=canonical, hashed=hashed)
                off = rec_off.cpu().numpy().astype(np.int64)
                hdr = hdr_off.cpu().numpy().astype(np.int64)
                win, hit = win.cpu().numpy().astype(np.uint32), hit.cpu().numpy().astype(np.uint32)
                lca = None if lca is None else lca.cpu().numpy().astype(np.uint32)
                for r in range(n_rec):
                    yield (index, _name(text, int(hdr[r])), int(off[r + 1] - off[r]), int(win[r]), int(hit[r]),
                           None if lca is None else int(lca[r]))
                    index += 1
            tail = text[consumed:]
            done += consumed


def format_row(row, with_lca):
    index, name, length, win, hit, lca = row
    cols = [str(index), name, str(length), str(win), str(hit), "%.6g" % (hit / win if win else 0.0)]
    if with_lca:
        cols.append(str(lca))
    return "\t".join(cols)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m unikmer_amd.screen",
                                 description="per-record k-mer hits (and taxid LCA) of a FASTA/Q file against a .unik set, as TSV")
    ap.add_argument("-f", "--min-frac", type=float, default=None, help="keep records with at least this fraction of windows in the set")
    ap.add_argument("-n", "--min-hits", type=int, default=None, help="keep records with at least this many windows in the set")
    ap.add_argument("--data-dir", default=os.path.join(os.path.expanduser("~"), ".unikmer"),
                    help="directory with nodes.dmp (and merged.dmp): read when the set carries taxids")
    ap.add_argument("set")
    ap.add_argument("fastx")
    a = ap.parse_args(argv)
    from . import lib, unikfile
    try:
        h = unikfile.read_header(a.set)
    except (ValueError, OSError) as e:
        sys.stderr.write("error: %s\n" % e)
        return 1
    with_lca = bool(h["flag"] & unikfile.INCLUDE_TAXID)
    filt = a.min_frac is not None or a.min_hits is not None
    min_frac = 0.0 if a.min_frac is None else a.min_frac
    min_hits = 1 if a.min_hits is None else a.min_hits
    ctx = lib.Context(0)
    try:
        if with_lca:
            load_taxdump(ctx, a.data_dir)
        cols = ["index", "name", "length", "windows", "hits", "fraction"] + (["lca"] if with_lca else [])
        sys.stdout.write("\t".join(cols) + "\n")
        for row in screen_file(ctx, a.set, a.fastx):
            if filt and not bool(select([row[3]], [row[4]], min_frac, min_hits)[0]):
                continue
            sys.stdout.write(format_row(row, with_lca) + "\n")
    except (ValueError, OSError, lib.UkmError) as e:
        sys.stderr.write("error: %s\n" % e)
        return 1
    finally:
        ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
