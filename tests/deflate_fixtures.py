"""What the deflate tests share (tests/test_deflate_cpu.py, tests/test_gpu_deflate.py): the chunk size read from the
kernels' source, real sorted .unik bodies from the golden genome, and the coder the device is measured against."""
import functools
import os
import re
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import unik_model as M  # noqa: E402

SOURCE = os.path.join(ROOT, "unikmer_amd", "csrc", "ukm_deflate.hip")


def source_constant(name):
    m = re.search(r"constexpr int %s = (\d+);" % name, open(SOURCE).read())
    assert m, "%s not found in %s" % (name, SOURCE)
    return int(m.group(1))


CH = source_constant("DFL_CHUNK")      # source bytes per chunk
STORED = source_constant("DFL_STORED")  # bytes a stored block adds
BODY_RECORDS = 34000                    # about 200 KB as a sorted body


def fibonacci_chunk():
    """frequencies 1, 1, 2, 3 ... 10946 over 21 byte values: 28656 bytes"""
    f = [1, 1]
    while len(f) < 21:
        f.append(f[-1] + f[-2])
    return np.concatenate([np.full(c, 37 + 5 * i, dtype=np.uint8) for i, c in enumerate(f)])


def fibonacci_chain():
    """1, 2, 3, 5 ... 2584 over 17 byte values: with end-of-block the unlimited Huffman tree is one chain 17 deep, so the
    limit of 15 acts"""
    f = [1, 2]
    while len(f) < 17:
        f.append(f[-1] + f[-2])
    return np.concatenate([np.full(c, 250 - 9 * i, dtype=np.uint8) for i, c in enumerate(f)])


@functools.lru_cache(maxsize=None)
def sorted_bodies():
    """(body, body with 4-byte taxids): BODY_RECORDS consecutive distinct canonical 31-mers from the middle of E. coli
    MG1655's sorted set, as unik::Writer lays them out (tests/unik_model.py)"""
    from conftest import MG1655, read_fasta_gz, splitmix64
    from oracle import oracle as O
    bases, off = read_fasta_gz(MG1655)
    codes = O.unique(O.sort_u64(O.count_windows(bases, off, 31, hashed=False, canonical=True)), mode=O.UNIQUE)
    codes = codes[len(codes) // 2: len(codes) // 2 + BODY_RECORDS]
    tax = (splitmix64(codes) % np.uint64(3000) + np.uint64(1)).astype(np.uint32)
    cl, tl = [int(c) for c in codes], [int(t) for t in tax]
    plain = M.encode(cl, None, 31, M.SORTED, 0)
    taxed = M.encode(cl, tl, 31, M.SORTED | M.INCLUDE_TAXID, 4)
    return np.frombuffer(plain, dtype=np.uint8), np.frombuffer(taxed, dtype=np.uint8)


def chunks_of(data):
    b = bytes(data)
    return [b[i: i + CH] for i in range(0, len(b), CH)]


def huffman_only(data):
    """zlib with Z_HUFFMAN_ONLY on the same chunks, a full flush behind each: the same coding decision per chunk, so what
    is left between this and the device is the block headers and the length-limiting rule"""
    z = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
    return b"".join(z.compress(c) + z.flush(zlib.Z_FULL_FLUSH) for c in chunks_of(data))
