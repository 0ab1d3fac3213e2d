"""`.unik` files for the Python user: the header is read and written here, the body goes through the device codec
(Context.unik_decode / unik_encode).  gzip inflate is the `gzip` module's, one host thread, unless load() is told
inflate="device" (Context.inflate: files written by save(deflate="device") or by the driver under UNIKMER_DEVICE_GZIP);
deflate is the `gzip` module's unless save() is told deflate="device" (Context.deflate).

The header layout is the one unikmer_amd/host/unik.hpp states (unik::Reader::read_header, unik::Writer::write_header),
big-endian throughout:
    magic ".unikmer" (8) | main = 5, minor = 0, K, 0 (4 x u8) | flag u32 | number u64 | global taxid u32
    | taxid bytes u8, 3 x 0 | description length u32 | description | scale u32 | max hash u64 | 52 reserved zero bytes
"""
import gzip
import io
import struct
import zlib

import numpy as np

from . import lib

MAGIC = b".unikmer"
COMPACT, CANONICAL, SORTED, INCLUDE_TAXID, HASHED, SCALED = 1, 2, 4, 8, 16, 32
UNKNOWN_NUMBER = 0xFFFFFFFFFFFFFFFF


def _open(path):
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    return gzip.open(path, "rb") if gz else open(path, "rb")


def _must(f, n, path):
    b = f.read(n)
    if len(b) != n:
        raise ValueError("unexpected EOF: %s" % path)
    return b


def _read_header(f, path):
    if f.read(8) != MAGIC:
        raise ValueError("invalid binary format: %s" % path)
    main, minor, k, _ = struct.unpack(">4B", _must(f, 4, path))
    if main != 5:
        raise ValueError("version mismatch (need v5.x): %s" % path)
    flag, number, global_taxid, tb = struct.unpack(">IQIB3x", _must(f, 20, path))
    if not 1 <= tb <= 4:
        raise ValueError("bad taxid byte length: %s" % path)
    (dl,) = struct.unpack(">I", _must(f, 4, path))
    if dl > 1024:
        raise ValueError("description too long: %s" % path)
    desc = _must(f, dl, path)
    scale, max_hash = struct.unpack(">IQ", _must(f, 12, path))
    _must(f, 52, path)
    return {"main_version": main, "minor_version": minor, "k": k, "flag": flag, "number": number, "global_taxid": global_taxid,
            "taxid_bytes": tb, "description": desc.decode("latin-1"), "scale": scale, "max_hash": max_hash}


def read_header(path):
    """the fields of unik::Header, as a dict"""
    with _open(path) as f:
        return _read_header(f, path)


def header_bytes(h):
    desc = h.get("description", "").encode("latin-1")
    return (MAGIC + struct.pack(">4B", h.get("main_version", 5), h.get("minor_version", 0), h["k"], 0)
            + struct.pack(">IQIB3x", h["flag"], h.get("number", UNKNOWN_NUMBER), h.get("global_taxid", 0), h.get("taxid_bytes", 4))
            + struct.pack(">I", len(desc)) + desc + struct.pack(">IQ", h.get("scale", 1), h.get("max_hash", UNKNOWN_NUMBER)) + bytes(52))


MARKER = b"\x00\x00\xff\xff"   # an empty stored block behind its 3 header bits and padding: where a sync flush ends


def _device_gunzip(ctx, path, device):
    """(header, body) of a gzip file whose body Context.inflate takes, the body where `device` says; None: the file is for
    the host path (which then also words whatever is wrong with it)"""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 18 or raw[:4] != b"\x1f\x8b\x08\x00":    # one member, deflate, FLG == 0
        return None
    src = raw[10:-8]
    trailer_crc, isize = struct.unpack("<II", raw[-8:])
    # zlib reads the .unik header, byte by byte, to the marker behind it (what save(deflate="device") and the driver write)
    d, hb, at, need = zlib.decompressobj(-15), b"", 0, None
    while True:
        if at >= len(src) or d.eof:
            return None
        try:
            hb += d.decompress(src[at: at + 1])
        except zlib.error:
            return None
        at += 1
        if need is None and len(hb) >= 36:
            need = 36 + struct.unpack(">I", hb[32:36])[0] + 64
        if len(hb) > (need if need is not None else 36 + 1024 + 64):
            return None                                    # the header does not end at a block boundary
        if len(hb) == need and src[at - 4: at] == MARKER:
            break
    try:
        h = _read_header(io.BytesIO(hb), path)
    except ValueError:
        return None
    frag = np.frombuffer(src, dtype=np.uint8)[at:]
    n = len(frag)
    # the body's size from ISIZE, the total modulo 2^32: the smallest that the fragment can inflate to (stored framing takes
    # less than a byte per 4096), and not above 8 bytes per byte
    total = (isize - len(hb)) % (1 << 32)
    while total < n - n // 4096 - 64:
        total += 1 << 32
    if total > lib.inflate_bound(n):
        return None
    if device:
        import torch
        frag = torch.from_numpy(frag.copy()).cuda()
    try:
        body, consumed, crc = ctx.inflate(frag, crc=zlib.crc32(hb), out=lib._empty_like_kind(frag, total, np.uint8))
    except lib.CapacityError as e:
        body, consumed, crc = ctx.inflate(frag, crc=zlib.crc32(hb), out=lib._empty_like_kind(frag, e.needed, np.uint8))
    if consumed == 0:
        return None
    nb = int(body.numel()) if lib._is_torch(body) else len(body)
    last = body[max(0, nb - 32768):]
    last = (last.cpu().numpy() if lib._is_torch(last) else last).tobytes()
    zdict = (hb + last)[-32768:]
    try:
        d = zlib.decompressobj(-15, zdict=zdict)
        tail = d.decompress(src[at + consumed:])
    except zlib.error:
        return None
    if not d.eof or d.unused_data:                         # a second member, or a stream that does not end
        return None
    if zlib.crc32(tail, crc) != trailer_crc or (len(hb) + nb + len(tail)) & 0xFFFFFFFF != isize:
        return None
    body = body[:nb]
    if tail:
        t = np.frombuffer(tail, dtype=np.uint8)
        if lib._is_torch(body):
            import torch
            body = torch.cat([body, torch.from_numpy(t.copy()).to(body.device)])
        else:
            body = np.concatenate([body, t])
    return h, body


def load(ctx, path, device=True, ignore_taxid=False, inflate="host"):
    """(header, keys, taxids): the records of a file, decoded on the device.  device=True: torch tensors on the GPU (the
    body is uploaded, 3-6 bytes a record for a sorted file), else numpy arrays.  taxids is None when the records carry none
    (a global taxid is in the header) or with ignore_taxid.  inflate="device": a gzip file written by
    save(deflate="device") or by the driver's device gzip is inflated by Context.inflate -- with device=True the compressed
    bytes are uploaded and the inflated body never crosses to the host; zlib reads the header, finishes the stream behind the
    body and the trailer's CRC-32 and size are checked.  Any other file goes the host's way, as without it."""
    if inflate not in ("host", "device"):
        raise ValueError("inflate must be 'host' or 'device'")
    got = _device_gunzip(ctx, path, device) if inflate == "device" else None
    if got is not None:
        h, body = got
        keys, taxids = ctx.unik_decode(body, h["k"], h["flag"], h["taxid_bytes"], with_taxids=not ignore_taxid)
        return h, keys, taxids
    with _open(path) as f:
        h = _read_header(f, path)
        body = np.frombuffer(f.read(), dtype=np.uint8)
    if device:
        import torch
        body = torch.from_numpy(body.copy()).cuda()
    keys, taxids = ctx.unik_decode(body, h["k"], h["flag"], h["taxid_bytes"], with_taxids=not ignore_taxid)
    return h, keys, taxids


GZIP_HEADER = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255])


def save(ctx, path, header, keys, taxids=None, compress=True, deflate="host"):
    """writes header and records; header["flag"] decides the layout (SORTED: keys must ascend pair by pair).  `number` is
    set to the record count.  deflate="device" (with compress): the body is deflated where it was encoded
    (Context.deflate: Huffman coding in independent chunks) and only the compressed bytes come to the host; the file is one
    gzip member that inflates to the same bytes."""
    if deflate not in ("host", "device"):
        raise ValueError("deflate must be 'host' or 'device'")
    h = dict(header)
    n = int(keys.numel()) if lib._is_torch(keys) else len(keys)
    h["number"] = n
    if taxids is None:
        h["flag"] &= ~INCLUDE_TAXID
    body = ctx.unik_encode(keys, h["k"], h["flag"], taxids=taxids, taxid_bytes=h.get("taxid_bytes", 4))
    if compress and deflate == "device":
        hb = header_bytes(h)
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        head = z.compress(hb) + z.flush(zlib.Z_SYNC_FLUSH)   # ends on a byte boundary, no final block
        frag, crc = ctx.deflate(body, crc=zlib.crc32(hb), final=True)
        nbody = int(body.numel()) if lib._is_torch(body) else len(body)
        if lib._is_torch(frag):
            frag = frag.cpu().numpy()
        with open(path, "wb") as f:
            f.write(GZIP_HEADER)
            f.write(head)
            f.write(frag.tobytes())
            f.write(struct.pack("<II", crc, (len(hb) + nbody) & 0xFFFFFFFF))
        return
    if lib._is_torch(body):
        body = body.cpu().numpy()
    with (gzip.open(path, "wb", compresslevel=6) if compress else open(path, "wb")) as f:
        f.write(header_bytes(h))
        f.write(body.tobytes())
