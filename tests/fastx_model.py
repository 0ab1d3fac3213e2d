"""A Python restatement of the FASTA/Q reader (unikmer_amd/host/seqtext.hpp: parse_fastx) and of the prefix grammar of
ukm_fastx (include/unikmer_hip.h), written with bytes.split / translate: megabytes take well under a second.

parse(text, fastq)        -> (bases, rec_off, names) as the host parser's sink sees them; HostError with the host's message
                             (without the file name) where the host dies.  fastq=None: the first line decides, as the host does.
device(text, fastq, last) -> (bases, rec_off, hdr_off, consumed, stop) as ukm_fastx leaves them.
CORPUS_FASTA / CORPUS_FASTQ / FASTQ_DEVIATIONS: the small explicit texts the CPU and the GPU tests share."""
import gzip
import os

import numpy as np

STOP_NONE, STOP_TAIL, STOP_GRAMMAR = 0, 1, 2
BLANKS = b" \t"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class HostError(Exception):
    pass


def is_fastq(text):
    """parse_fastx's rule: FASTQ iff the first line of the file is non-empty and begins with '@'"""
    first = text.split(b"\n", 1)[0]
    if b"\n" in text and first.endswith(b"\r"):
        first = first[:-1]
    return first[:1] == b"@"


def host_lines(text):
    """the lines the host handles: a CR in front of an LF is dropped; the rest behind the last LF is a line if it holds a byte"""
    parts = text.split(b"\n")
    lines = [p[:-1] if p.endswith(b"\r") else p for p in parts[:-1]]
    if parts[-1]:
        lines.append(parts[-1])
    return lines


def parse(text, fastq=None):
    if fastq is None:
        fastq = is_fastq(text)
    names, seqs = [], []
    if fastq:
        state, seq_len, qual_len = 0, 0, 0
        for l in host_lines(text):
            if state == 0:
                if not l:
                    continue
                if l[:1] != b"@":
                    raise HostError("invalid FASTQ record in")
                names.append(l[1:])
                seqs.append([])
                seq_len = qual_len = 0
                state = 1
            elif state == 1:
                if l[:1] == b"+":
                    state = 3
                else:
                    s = l.translate(None, BLANKS)
                    seqs[-1].append(s)
                    seq_len += len(s)
            else:
                qual_len += len(l)
                if qual_len >= seq_len:
                    state = 0
    else:
        for l in host_lines(text):
            if l[:1] == b">":
                names.append(l[1:])
                seqs.append([])
            elif not names:
                if l:
                    raise HostError("invalid FASTA/Q format:")
            else:
                seqs[-1].append(l.translate(None, BLANKS))
    recs = [b"".join(s) for s in seqs]
    rec_off = np.zeros(len(recs) + 1, dtype=np.uint64)
    if recs:
        rec_off[1:] = np.cumsum([len(r) for r in recs], dtype=np.uint64)
    return b"".join(recs), rec_off, names


def _pieces(text):
    """(start, raw bytes, ends in an LF) of every line that holds a byte or an LF"""
    parts = text.split(b"\n")
    out, at = [], 0
    for i, p in enumerate(parts):
        lf = i + 1 < len(parts)
        if lf or p:
            out.append((at, p, lf))
        at += len(p) + 1
    return out


def _result(text, consumed, fastq, stop, hdr):
    bases, rec_off, names = parse(text[:consumed], fastq)
    assert len(names) == len(hdr)
    return bases, rec_off, np.array(hdr, dtype=np.uint64), consumed, stop


def device(text, fastq, last):
    n = len(text)
    if n == 0:
        return b"", np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint64), 0, STOP_NONE
    pieces = _pieces(text)
    if not fastq:
        hdr = [at for at, p, lf in pieces if p[:1] == b">"]
        for at, p, lf in pieces:
            if p[:1] == b">":
                break
            # in front of the first header: an empty line passes; a CR that ends a text with more behind it is undecided
            if (p == b"" and lf) or (p == b"\r" and (lf or not last)):
                continue
            return _result(text, 0, False, STOP_GRAMMAR, [])[:3] + (at, STOP_GRAMMAR)
        if last:
            return _result(text, n, False, STOP_NONE, hdr)
        if not hdr:
            return _result(text, 0, False, STOP_TAIL, [])
        return _result(text, hdr[-1], False, STOP_TAIL, hdr[:-1])
    # FASTQ: groups of four lines; without LAST a line counts only with its LF
    lines = [x for x in pieces if x[2] or last]
    hdr, consumed, bad = [], 0, False
    for g in range(len(lines) // 4):
        (a0, a, _), (_, b, _), (_, c, _), (d0, d, dlf) = lines[4 * g: 4 * g + 4]
        bs = b[:-1] if b.endswith(b"\r") else b
        ds = d[:-1] if dlf and d.endswith(b"\r") else d
        ok = (a[:1] == b"@" and b[:1] != b"+" and b" " not in b and b"\t" not in b and c[:1] == b"+" and len(ds) >= len(bs))
        if not ok:
            bad = True
            break
        hdr.append(a0)
        consumed = min(d0 + len(d) + 1, n)
    stop = STOP_GRAMMAR if bad else STOP_NONE if consumed == n else STOP_GRAMMAR if last else STOP_TAIL
    return _result(text, consumed, True, stop, hdr)


def golden_texts():
    out = {}
    for f in sorted(os.listdir(GOLDEN)):
        if f.endswith(".fasta.gz"):
            with gzip.open(os.path.join(GOLDEN, f), "rb") as fh:
                out[f] = fh.read()
    return out


CORPUS_FASTA = {
    "lf": b">r1 first\nACGTACGT\nACGT\n>r2\nTTGGCCAA\n",
    "crlf": b">r1 first\r\nACGTACGT\r\nACGT\r\n>r2\r\nTTGGCCAA\r\n",
    "cr_inside": b">r1\nAC\rGT\nA\r\r\nCC\n",
    "cr_last_byte": b">r1\nACGT\n>r2\nGG\r",
    "no_final_lf": b">r1\nACGT\n>r2\nGGTT",
    "leading_empty": b"\n\r\n\n>r1\nACGT\n",
    "garbage_first": b"ACGT\n>r1\nACGT\n",
    "garbage_after_empty": b"\n\nxyz\n>r1\nACGT\n",
    "blank_line_first": b" \n>r1\nACGT\n",
    "cr_only_first": b"\r>r1\nACGT\n",
    "gt_alone": b">",
    "gt_alone_lf": b">\n",
    "gt_after_gt": b">\n>\n>a\n>b\nAC\n>\n",
    "blanks_in_seq": b">r1\nAC GT\tAC\n \t \nGG \n>r2\n\tT\n",
    "empty_lines_inside": b">r1\nAC\n\n\r\nGT\n\n>r2\n\n",
    "gt_inside_seq": b">r1\nAC>GT\nA>\n",
    "empty_then_at": b"\n@r1\nACGT\n",
    "one_line_record": b">r1\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n",
    "only_empty_lines": b"\n\n\r\n",
    "header_only_no_lf": b">r1 name without end",
}

CORPUS_FASTQ = {
    "well_formed": b"@r1\nACGT\n+\nIIII\n@r2 x\nGGCC\n+r2\nJJJJ\n",
    "qual_begins_at": b"@r1\nACGT\n+\n@III\n@r2\nGG\n+\n@@\n",
    "qual_begins_plus": b"@r1\nACGT\n+\n+III\n@r2\nGG\n+\n++\n",
    "empty_seq": b"@r1\n\n+\n\n@r2\nAC\n+\nII\n",
    "qual_longer": b"@r1\nAC\n+\nIIIII\n@r2\nAC\n+\nII\n",
    "no_final_lf": b"@r1\nACGT\n+\nIIII\n@r2\nGGCC\n+\nJJJJ",
    "crlf": b"@r1\r\nACGT\r\n+\r\nIIII\r\n@r2\r\nGG\r\n+\r\nJJ\r\n",
    "cr_last_byte": b"@r1\nACGT\n+\nIII\r",
    "at_alone": b"@\nAC\n+\nII\n",
}

FASTQ_DEVIATIONS = {
    "two_line_seq": b"@r1\nACGT\n+\nIIII\n@r2\nAC\nGT\n+\nIIII\n@r3\nAC\n+\nII\n",
    "two_line_qual": b"@r1\nACGT\n+\nIIII\n@r2\nACGT\n+\nII\nII\n@r3\nAC\n+\nII\n",
    "short_qual": b"@r1\nACGT\n+\nIII\n@r2\nAC\n+\nII\n",
    "blank_in_seq": b"@r1\nAC GT\n+\nIIII\n@r2\nAC\n+\nII\n",
    "empty_between": b"@r1\nACGT\n+\nIIII\n\n@r2\nAC\n+\nII\n",
    "trailing_empty": b"@r1\nACGT\n+\nIIII\n\n",
    "header_without_at": b"@r1\nACGT\n+\nIIII\nr2\nAC\n+\nII\n",
}
