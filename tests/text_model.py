"""A model of the k-mer text of `unikmer view` and `unikmer dump`, in plain Python: the seven line formats of view.go:163-218
(render) and the strict grammar ukm_dump accepts (parse: the records, or the offset of the first bad line).
tests/test_text_cpu.py pins both to the host loops of unikmer_amd/host/cmd_cpu.hpp; tests/test_gpu_text.py holds ukm_view and
ukm_dump to them byte for byte."""
import collections

KMER, KMER_CODE, CODE, KMER_TAXID, TAXID, FASTA, FASTQ = range(7)
WITH_TAXID = 16
FORMATS = (KMER, KMER_CODE, CODE, KMER_TAXID, TAXID, FASTA, FASTQ, FASTA | WITH_TAXID, FASTQ | WITH_TAXID)
D_TAXID, D_DECIMAL, D_CANONICAL, D_CANONICAL_ONLY = 1, 2, 4, 8
MAX_LINE = 32 + 1 + 10 + 1 + 1     # the longest legal line of dump: k-mer, TAB, taxid, CR, LF

BASE2BIT = {}
for _letters, _bit in (("ANMVHRDW", 0), ("CSBY", 1), ("GK", 2), ("TU", 3)):
    for _c in _letters:
        BASE2BIT[ord(_c)] = BASE2BIT[ord(_c.lower())] = _bit


def kmer_text(code, k):
    return "".join("ACGT"[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def line(code, taxid, k, hashed, fmt):
    """one record as view prints it"""
    C, T = str(code), str(taxid)
    K = C if hashed else kmer_text(code, k)
    base = fmt & 15
    head = C + (" " + T if fmt & WITH_TAXID else "")
    return {KMER: K + "\n", KMER_CODE: K + "\t" + C + "\n", CODE: C + "\n", KMER_TAXID: K + "\t" + T + "\n", TAXID: T + "\n",
            FASTA: ">" + head + "\n" + K + "\n", FASTQ: "@" + head + "\n" + K + "\n+\n" + "g" * k + "\n"}[base]


def render(codes, taxids, file_taxid, k, hashed, fmt):
    """the text of the records; taxids None: every record carries file_taxid"""
    return "".join(line(int(c), int(file_taxid if taxids is None else taxids[i]), k, hashed, fmt) for i, c in enumerate(codes)).encode()


def bound(n, k, hashed, fmt):
    """what ukm_view_bound promises: exact for KMER of plain codes, else codes of 20 and taxids of 10 digits"""
    return n * len(line((1 << 64) - 1, (1 << 32) - 1, k, hashed, fmt))


def revcomp(code, k):
    c, r = ~code, 0
    for _ in range(k):
        r = (r << 2) | (c & 3)
        c >>= 2
    return r


Parsed = collections.namedtuple("Parsed", "codes taxids bad_off")   # bad_off None: the text is legal


def _decimal(field, most_digits, top):
    if not 1 <= len(field) <= most_digits or not all(48 <= b <= 57 for b in field):
        return None
    v = int(field)
    return v if v <= top else None


def parse(text, k, flags):
    """the strict grammar: lines between LF (the last may lack it), one trailing CR dropped, empty lines skipped, every
    other line field1 or -- with D_TAXID -- field1 TAB field2 and nothing else"""
    codes, taxids = [], []
    off = 0
    while off < len(text):
        end = text.find(b"\n", off)
        nxt = len(text) if end < 0 else end + 1
        ln = text[off:len(text) if end < 0 else end]
        start, off = off, nxt
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        if not ln:
            continue
        fields = ln.split(b"\t")
        if len(fields) != (2 if flags & D_TAXID else 1):
            return Parsed(None, None, start)
        if flags & D_DECIMAL:
            code = _decimal(fields[0], 20, (1 << 64) - 1)
        elif len(fields[0]) == k and all(b in BASE2BIT for b in fields[0]):
            code = 0
            for b in fields[0]:
                code = (code << 2) | BASE2BIT[b]
        else:
            code = None
        taxid = _decimal(fields[1], 10, (1 << 32) - 1) if flags & D_TAXID else 0
        if code is None or taxid is None:
            return Parsed(None, None, start)
        if flags & D_CANONICAL_ONLY:
            if revcomp(code, k) < code:
                continue
        elif flags & D_CANONICAL:
            code = min(code, revcomp(code, k))
        codes.append(code)
        taxids.append(taxid)
    return Parsed(codes, taxids if flags & D_TAXID else None, None)
