"""A pure-Python model of ukm_inflate's contract (include/unikmer_hip.h): the longest prefix of a raw RFC 1951 fragment
that is non-final blocks of literals, and where it stops.  inflate_prefix(src) -> (consumed, out).

It states the contract a second time, independently of the kernels: candidates behind every 00 00 FF FF, a segment parser,
and the chain from offset 0.  The GPU tests compare against it wherever zlib alone cannot say where the device must stop."""

MARKER = b"\x00\x00\xff\xff"
SEG_LIMIT = 1 << 31
LITERAL_LIMIT = 1 << 20      # literals of Huffman blocks in one segment: what one lane may be asked to decode
BLOCK_LIMIT = 1 << 20        # blocks in one segment
PERM = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


class Stop(Exception):
    """the block at hand is one the device does not take"""


class Bits:
    def __init__(self, src, bit):
        self.src, self.pos, self.end = src, bit, 8 * len(src)

    def peek(self, n):
        """n <= 24 bits at pos, zeros behind the end"""
        b = self.pos >> 3
        return (int.from_bytes(self.src[b: b + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def take(self, n):
        if self.pos + n > self.end:
            raise Stop("runs past n_bytes")
        v = self.peek(n)
        self.pos += n
        return v


def kraft(lens):
    """(left in units of 2^-15, longest length)"""
    left = 1 << 15
    for l in lens:
        if l:
            left -= 1 << (15 - l)
    return left, max(lens) if lens else 0


def accepted(lens, code_lengths):
    """zlib's inflate_table: over-subscribed never; incomplete only as ONE code of one bit, and not for the code-length
    code; no code at all only for distances"""
    left, mx = kraft(lens)
    if left < 0:
        return False
    if mx == 0:
        return not code_lengths
    return left == 0 or (not code_lengths and mx == 1)


def decoder(lens):
    """(table, width): table[the next `width` bits] = (symbol, length) or None; canonical codes, RFC 1951 3.2.2"""
    width = max(lens)
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = [None] * (1 << width)
    for s, l in enumerate(lens):
        if not l:
            continue
        c = nxt[l]
        nxt[l] += 1
        r = int(format(c, "0%db" % l)[::-1], 2)        # packed from the most significant bit
        for hi in range(1 << (width - l)):
            table[r | (hi << l)] = (s, l)
    return table, width


def symbol(br, dec):
    table, width = dec
    e = table[br.peek(width)]
    if e is None:
        raise Stop("no code")
    if br.pos + e[1] > br.end:
        raise Stop("runs past n_bytes")
    br.pos += e[1]
    return e[0]


FIXED = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def dynamic_lengths(br):
    nlen, ndist, ncode = 257 + br.take(5), 1 + br.take(5), 4 + br.take(4)
    if nlen > 286 or ndist > 30:
        raise Stop("too many symbols")
    cl = [0] * 19
    for i in range(ncode):
        cl[PERM[i]] = br.take(3)
    if max(cl) == 0 or not accepted(cl, True):
        raise Stop("code-length code")
    dec = decoder(cl)
    lens = []
    while len(lens) < nlen + ndist:
        s = symbol(br, dec)
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise Stop("repeat of nothing")
            val, rep = lens[-1], 3 + br.take(2)
        elif s == 17:
            val, rep = 0, 3 + br.take(3)
        else:
            val, rep = 0, 11 + br.take(7)
        if len(lens) + rep > nlen + ndist:
            raise Stop("repeat too long")
        lens += [val] * rep
    if lens[256] == 0:
        raise Stop("no end-of-block")
    if not accepted(lens[nlen:], False) or not accepted(lens[:nlen], False):
        raise Stop("code")
    return lens[:nlen]


def parse_segment(src, start, seen=None):
    """(end, out, early): the segment that starts at byte `start`.  It ends behind an empty stored block; early: it stopped
    in front of a block the device does not take, and end / out are the last safe point: the start, or the byte behind a
    stored block whose header began on a byte boundary.  seen: a set that collects what it met."""
    br = Bits(src, 8 * start)
    out = bytearray()
    safe = (start, 0)
    seen = seen if seen is not None else set()
    literals = blocks = 0
    try:
        while True:
            hdr = br.pos
            blocks += 1
            if blocks > BLOCK_LIMIT:
                raise Stop("block limit")
            if br.take(1):
                raise Stop("final")
            btype = br.take(2)
            if btype == 3:
                raise Stop("BTYPE 11")
            if btype == 0:
                br.pos = (br.pos + 7) & ~7
                ln, nln = br.take(16), br.take(16)
                if ln ^ 0xFFFF != nln:
                    raise Stop("LEN != ~NLEN")
                p = br.pos >> 3
                if p + ln > len(src):
                    raise Stop("runs past n_bytes")
                if len(out) + ln >= SEG_LIMIT:
                    raise Stop("segment limit")
                out += src[p: p + ln]
                br.pos += 8 * ln
                if ln == 0:
                    seen.add("marker")
                    return p, bytes(out), False
                seen.add("stored")
                if hdr & 7:
                    seen.add("stored unaligned")
                else:
                    safe = (p + ln, len(out))
                continue
            dec = decoder(FIXED if btype == 1 else dynamic_lengths(br))
            blk = bytearray()
            while True:
                s = symbol(br, dec)
                if s == 256:
                    break
                if s > 256:
                    raise Stop("length symbol")
                blk.append(s)
                if len(out) + len(blk) >= SEG_LIMIT or literals + len(blk) > LITERAL_LIMIT:
                    raise Stop("segment limit")
            out += blk
            literals += len(blk)
            seen.add("fixed" if btype == 1 else "dynamic")
    except Stop:
        return safe[0], bytes(out[: safe[1]]), True


def candidates(src):
    c, p = [0], src.find(MARKER)
    while p >= 0:
        c.append(p + 4)
        p = src.find(MARKER, p + 1)
    return c


def inflate_prefix(src, seen=None):
    """(consumed, out): segment ends chained from offset 0; only segments on the chain count, and the chain ends at the first
    one that stopped early, whose byte-aligned prefix still counts"""
    src = bytes(src)
    cand = set(candidates(src))
    at, out = 0, bytearray()
    while at < len(src):
        end, o, early = parse_segment(src, at, seen)
        out += o
        at = end
        if early or end not in cand:
            break
    return at, bytes(out)
