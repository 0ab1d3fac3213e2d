// ukm_inflate.h — the block parser of ukm_inflate.hip, compiled for host and device alike (and, with a plain C++ compiler,
// into tests/inflate_units.cpp): a bit reader that never leaves src[0, n_bytes), the canonical decode table of a fixed or
// dynamic block under zlib's rules of acceptance, and the walk over one segment of a raw RFC 1951 fragment.
//
// A segment starts at a block boundary on a byte boundary and holds NON-FINAL blocks of literals: stored, fixed, dynamic.
// It ENDS behind an empty stored block (the marker 00 00 FF FF: a sync or full flush), and it STOPS EARLY in front of the
// first block that is final, has BTYPE 11, holds a symbol above end-of-block, has LEN != ~NLEN, a code zlib refuses,
// runs past n_bytes, or takes the segment beyond one of its limits (below).  A segment that stops early reports the last SAFE point it passed: its own start, or the byte behind a
// stored block whose header began on a byte boundary.  Nothing here judges the stream: whatever stops the walk is left for
// zlib to meet and name.
#pragma once
#include <stdint.h>

#include "ukm_huff.h"

namespace ukm_puff {

constexpr int LL_SYMS = 288;         // what a fixed block's literal / length code covers (a dynamic one: at most 286)
constexpr int LENS = 320;            // code lengths a dynamic header carries at most: 286 + 30, rounded up
constexpr uint32_t CP_BYTES = 1024;  // output bytes between two checkpoints
constexpr int LUT_BITS = 9;          // codes up to this length are decoded by ONE lookup where the caller has room for the table
constexpr int LUT_SIZE = 1 << LUT_BITS;  // entries of uint16_t: symbol | length << 9; 0: a longer code, or none
constexpr uint64_t SEG_LIMIT = 1ull << 31;  // a segment's output stays below this: its size is summed in 32 bits
// What ONE lane may be asked to do, on the chain or off it: a segment is walked serially, and a file made for the purpose (a
// stored payload full of markers, each in front of long valid data; a Huffman-only stream that never flushes) must not hold a
// lane for minutes.  A segment stops early in front of the block that takes it beyond either.  ukm_deflate's segments are one
// block of 32768 literals; zlib's flushed per chunk a few hundred blocks.
constexpr uint64_t LITERAL_LIMIT = 1ull << 20;  // literals of Huffman blocks in one segment
constexpr uint64_t BLOCK_LIMIT = 1ull << 20;    // blocks in one segment
constexpr uint64_t STORED_CP = ~0ull;       // Checkpoint::hdr of a piece of a stored block

struct Table {  // canonical decode: symbols by (length, symbol), and how many have each length
    uint16_t count[16];
    uint16_t sym[LL_SYMS];
};

// Where the write pass resumes: `n` <= CP_BYTES output bytes that land at out[out, out + n).  hdr: the bit position of the
// header (BFINAL) of the block they belong to, bit: that of their first symbol.  A piece of a stored block: hdr = STORED_CP,
// bit = 8 * the source offset of its first byte.
struct Checkpoint {
    uint64_t bit, hdr, out;
    uint32_t n, pad;
};

struct BitReader {
    const uint8_t *src;
    uint64_t n_bytes, next;  // next: the first byte not in buf
    uint64_t buf;
    uint32_t cnt;  // valid bits in buf, from bit 0
    UKM_HD void seek(uint64_t bit) {
        next = bit >> 3;
        buf = 0;
        cnt = 0;
        if (bit & 7) {
            refill();
            const uint32_t d = (uint32_t)(bit & 7);
            if (cnt >= d) {
                buf >>= d;
                cnt -= d;
            } else {
                cnt = 0;
            }
        }
    }
    UKM_HD uint64_t pos() const { return next * 8 - cnt; }
    // up to 57..64 bits where the source has them: an aligned 4-byte word wholly inside src, or single bytes
    UKM_HD void refill() {
        while (cnt <= 56 && next < n_bytes) {
            if (cnt <= 32 && next + 4 <= n_bytes && (((uintptr_t)(src + next)) & 3) == 0) {
                buf |= (uint64_t)(*(const uint32_t *)(src + next)) << cnt;
                next += 4;
                cnt += 32;
            } else {
                buf |= (uint64_t)src[next] << cnt;
                next += 1;
                cnt += 8;
            }
        }
    }
    // n <= 32 bits; false: the source ends first
    UKM_HD bool take(uint32_t n, uint32_t *v) {
        if (cnt < n) {
            refill();
            if (cnt < n) return false;
        }
        *v = (uint32_t)(buf & ((1ull << n) - 1ull));
        buf >>= n;
        cnt -= n;
        return true;
    }
    UKM_HD void align() {
        const uint32_t d = cnt & 7;  // next * 8 is a byte boundary, so cnt mod 8 bits remain of the current byte
        buf >>= d;
        cnt -= d;
    }
};

// One symbol: 0 .. LL_SYMS - 1, or -1 where the source ends inside the code or the bits are no code of the table (an
// incomplete code's unused pattern).  Bit by bit, as RFC 1951 3.2.2 numbers the codes; every index is below LL_SYMS whatever
// the table holds.  lut (fill_lut): the short codes by one lookup first; what it does not hold goes bit by bit.
UKM_HD int decode_symbol(BitReader *br, const Table *t, const uint16_t *lut = nullptr) {
    if (br->cnt < 15) br->refill();
    if (lut) {
        const uint32_t e = lut[br->buf & (uint64_t)(LUT_SIZE - 1)], len = e >> 9;  // (bits behind the source's end read as zeros)
        if (e && len <= br->cnt) {
            br->buf >>= len;
            br->cnt -= len;
            return (int)(e & 511u);
        }
    }
    uint64_t bits = br->buf;
    const uint32_t avail = br->cnt < 15 ? br->cnt : 15;
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len <= avail; len++) {
        code |= (uint32_t)(bits & 1u);
        bits >>= 1;
        const uint32_t count = t->count[len];
        if (code - first < count) {
            br->buf >>= len;
            br->cnt -= len;
            const uint32_t i = index + (code - first);
            return t->sym[i < (uint32_t)LL_SYMS ? i : LL_SYMS - 1];
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return -1;
}

// count[] and sym[] from lens[0, n), n <= LL_SYMS.  Returns the Kraft remainder `left` in units of 2^-15 (0: complete;
// below 0: over-subscribed) and *max_len, the longest length in use (0: no code at all).
UKM_HD int fill_table(const uint8_t *lens, int n, Table *t, int *max_len) {
    uint16_t offs[16];
    for (int b = 0; b < 16; b++) t->count[b] = 0;
    for (int s = 0; s < n; s++) t->count[lens[s] & 15]++;
    t->count[0] = 0;
    int left = 1 << 15, mx = 0;
    for (int b = 1; b < 16; b++) {
        left -= (int)t->count[b] << (15 - b);
        if (t->count[b]) mx = b;
    }
    *max_len = mx;
    if (left < 0) return left;
    offs[1] = 0;
    for (int b = 1; b < 15; b++) offs[b + 1] = (uint16_t)(offs[b] + t->count[b]);
    for (int s = 0; s < n; s++) {
        const int l = lens[s] & 15;
        if (l) {
            const uint32_t i = offs[l]++;
            if (i < (uint32_t)LL_SYMS) t->sym[i] = (uint16_t)s;
        }
    }
    return left;
}
// lut[LUT_SIZE] for a table that is not over-subscribed: every code of at most LUT_BITS bits, at all the indexes whose low bits
// are the code as it stands in the stream (most significant code bit first)
UKM_HD void fill_lut(const Table *t, uint16_t *lut) {
    for (int i = 0; i < LUT_SIZE; i++) lut[i] = 0;
    uint32_t first = 0, index = 0;
    for (uint32_t len = 1; len <= (uint32_t)LUT_BITS; len++) {
        const uint32_t count = t->count[len];
        for (uint32_t j = 0; j < count && first + j < (1u << len) && index + j < (uint32_t)LL_SYMS; j++) {
            const uint32_t rev = ukm_huff::bit_reverse(first + j, (int)len);
            const uint16_t e = (uint16_t)((t->sym[index + j] & 511u) | (len << 9));
            for (uint32_t at = rev; at < (uint32_t)LUT_SIZE; at += 1u << len) lut[at] = e;
        }
        index += count;
        first = (first + count) << 1;
    }
}

// zlib's inflate_table: an over-subscribed code is refused; an incomplete one too, unless it is a literal / length or a
// distance code whose longest length is 1 (one code of one bit); a distance code with no code at all passes
UKM_HD bool code_accepted(int left, int max_len, bool code_lengths) {
    if (left < 0) return false;
    if (max_len == 0) return !code_lengths;
    return left == 0 || (!code_lengths && max_len == 1);
}

// The table of the block whose 3 header bits br has just passed: btype 1 (fixed) or 2 (dynamic, header read from br).
// lens: LENS bytes of scratch; lut: LUT_SIZE entries for decode_symbol, or nullptr.  false: zlib would refuse the header, or
// the source ends inside it.
UKM_HD bool build_table(BitReader *br, int btype, Table *t, uint8_t *lens, uint16_t *lut = nullptr) {
    int mx;
    if (btype == 1) {
        for (int s = 0; s < LL_SYMS; s++) lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
        (void)fill_table(lens, LL_SYMS, t, &mx);
        if (lut) fill_lut(t, lut);
        return true;
    }
    uint32_t v;
    if (!br->take(14, &v)) return false;
    const int nlen = 257 + (int)(v & 31), ndist = 1 + (int)((v >> 5) & 31), ncode = 4 + (int)(v >> 10);
    if (nlen > 286 || ndist > 30) return false;
    const uint8_t perm[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < 19; i++) lens[i] = 0;
    for (int i = 0; i < ncode; i++) {
        if (!br->take(3, &v)) return false;
        lens[perm[i]] = (uint8_t)v;
    }
    int left = fill_table(lens, 19, t, &mx);
    if (mx == 0 || !code_accepted(left, mx, true)) return false;
    // the code-length code sits in t while the lengths are read: it is replaced below
    int have = 0;
    while (have < nlen + ndist) {
        const int s = decode_symbol(br, t);
        if (s < 0 || s > 18) return false;
        if (s < 16) {
            lens[have++] = (uint8_t)s;
            continue;
        }
        int rep, val = 0;
        if (s == 16) {
            if (have == 0 || !br->take(2, &v)) return false;
            val = lens[have - 1];
            rep = 3 + (int)v;
        } else if (s == 17) {
            if (!br->take(3, &v)) return false;
            rep = 3 + (int)v;
        } else {
            if (!br->take(7, &v)) return false;
            rep = 11 + (int)v;
        }
        if (have + rep > nlen + ndist) return false;
        while (rep--) lens[have++] = (uint8_t)val;
    }
    if (lens[256] == 0) return false;  // no end-of-block
    // the distance code first: its table is only judged, never used
    left = fill_table(lens + nlen, ndist, t, &mx);
    if (!code_accepted(left, mx, false)) return false;
    left = fill_table(lens, nlen, t, &mx);
    if (!code_accepted(left, mx, false)) return false;
    if (lut) fill_lut(t, lut);
    return true;
}

struct SegResult {
    uint64_t end;  // the byte behind the marker, or the last safe point of a segment that stopped early
    uint64_t out;  // output bytes of src[start, end)
    uint64_t ncp;  // checkpoints of src[start, end)
    bool early;
};

// Walks the segment that starts at byte `start`; emit(bit, hdr, out, n) is called for every checkpoint, `out` counted from
// the segment's start.  limit: a safe point at which the walk returns as if the segment ended there (the write side passes
// the end the size side reported, and so sees exactly the checkpoints counted); ~0: none.
template <class Emit>
UKM_HD SegResult walk_segment(const uint8_t *src, uint64_t n_bytes, uint64_t start, uint64_t limit, Table *t, uint8_t *lens, uint16_t *lut,
                              Emit &&emit) {
    BitReader br;
    br.src = src;
    br.n_bytes = n_bytes;
    br.seek(start * 8);
    SegResult safe = {start, 0, 0, true};
    uint64_t out = 0, ncp = 0, literals = 0, blocks = 0;
    for (;;) {
        const uint64_t hdr = br.pos();
        const bool aligned = (hdr & 7) == 0;
        if (aligned && (hdr >> 3) == limit) {
            SegResult r = {limit, out, ncp, false};
            return r;
        }
        uint32_t h;
        if (++blocks > BLOCK_LIMIT) break;
        if (!br.take(3, &h)) break;
        if (h & 1u) break;
        const int btype = (int)(h >> 1);
        if (btype == 3) break;
        if (btype == 0) {
            br.align();
            uint32_t len, nlen;
            if (!br.take(16, &len) || !br.take(16, &nlen)) break;
            if ((len ^ 0xFFFFu) != nlen) break;
            const uint64_t payload = br.pos() >> 3;
            if (payload + len > n_bytes || out + len >= SEG_LIMIT) break;
            for (uint32_t o = 0; o < len; o += CP_BYTES) {
                emit((payload + o) * 8, STORED_CP, out + o, len - o < CP_BYTES ? len - o : CP_BYTES);
                ncp++;
            }
            out += len;
            br.seek((payload + len) * 8);
            if (len == 0) {
                SegResult r = {payload, out, ncp, false};
                return r;
            }
            if (aligned) {
                safe.end = payload + len;
                safe.out = out;
                safe.ncp = ncp;
            }
            continue;
        }
        if (!build_table(&br, btype, t, lens, lut)) break;
        uint64_t blk = 0, cp_bit = br.pos();
        uint32_t cp_n = 0;
        bool bad = false;
        for (;;) {
            const int s = decode_symbol(&br, t, lut);
            if (s < 0 || s > 256) {
                bad = true;
                break;
            }
            if (s == 256) break;
            blk++;
            if (out + blk >= SEG_LIMIT || literals + blk > LITERAL_LIMIT) {
                bad = true;
                break;
            }
            if (++cp_n == CP_BYTES) {
                emit(cp_bit, hdr, out + blk - CP_BYTES, CP_BYTES);
                ncp++;
                cp_n = 0;
                cp_bit = br.pos();
            }
        }
        if (bad) break;
        if (cp_n) {
            emit(cp_bit, hdr, out + blk - cp_n, cp_n);
            ncp++;
        }
        out += blk;
        literals += blk;
    }
    return safe;
}

}  // namespace ukm_puff
