// ukm_huff.h — what ukm_deflate.hip's kernels and its host code share, compiled for host and device alike (and, with a
// plain C++ compiler, into tests/deflate_units.cpp): length-limited Huffman code lengths, canonical deflate codes, the
// header of a dynamic block of literals, and the arithmetic of CRC-32 (RFC 1951 3.2.2, 3.2.7; RFC 1952 8).  The CRC part,
// with the workgroup's slice routine, is ukm_inflate.hip's too.
//
// Code lengths: Huffman, then repair -- what zlib's gen_bitlen does.  The used symbols are sorted by (frequency, symbol);
// the two-queue merge (sorted leaves, internal nodes in creation order) builds the tree in O(n); the depths of the leaves
// are COUNTED per length, depths beyond the limit are cut to the limit, and for every two nodes so cut one leaf of the
// deepest level above the limit is pushed one level down, which brings the Kraft sum back to exactly 1.  The lengths are then
// dealt out afresh, the longest to the least frequent symbol: only the counts per length matter.  Everything is integer
// arithmetic on the histogram: the lengths are a pure function of it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define UKM_HD __host__ __device__ inline
#else
#define UKM_HD inline
#endif

namespace ukm_huff {

constexpr int MAX_SYMS = 286;   // the literal / length alphabet; the code-length alphabet (19) goes through the same routine
constexpr int LIT_SYMS = 257;   // literals and end-of-block: all a block of ukm_deflate uses
constexpr int EOB = 256;
constexpr int CL_SYMS = 19;
constexpr int LIT_LIMIT = 15, CL_LIMIT = 7;
constexpr int SEQ_LEN = LIT_SYMS + 1;  // the lengths a header carries: 257 literal / length codes, 1 distance code

struct Scratch {  // working memory of the length routine (LDS on the device)
    uint32_t weight[2 * MAX_SYMS];
    uint16_t parent[2 * MAX_SYMS];
    uint16_t depth[2 * MAX_SYMS];
    uint16_t order[MAX_SYMS];  // the used symbols by (frequency, symbol) ascending
    uint16_t count[16];        // leaves per length
};

// order[0, m) = the symbols with freq > 0 by (freq, symbol) ascending; returns m.  (The kernels rank in parallel instead.)
UKM_HD int sort_symbols(const uint32_t *freq, int n, uint16_t *order) {
    int m = 0;
    for (int s = 0; s < n; s++) {
        if (!freq[s]) continue;
        int i = m++;
        while (i > 0 && freq[order[i - 1]] > freq[s]) {
            order[i] = order[i - 1];
            i--;
        }
        order[i] = (uint16_t)s;
    }
    return m;
}

// len[0, n): 0 for a symbol that does not occur, else 1..limit, Kraft sum exactly 1.  S->order[0, m) as sort_symbols leaves
// it, m >= 1, m <= 2^limit.  One symbol alone gets one bit and a partner that never occurs the other: inflate refuses an
// incomplete code.
UKM_HD void lengths_from_sorted(const uint32_t *freq, int n, int m, int limit, Scratch *S, uint8_t *len) {
    for (int s = 0; s < n; s++) len[s] = 0;
    if (m <= 0) return;
    if (m == 1) {
        const int s = S->order[0];
        len[s] = 1;
        len[s == 0 ? 1 : 0] = 1;
        return;
    }
    // nodes [0, m): the leaves in order; [m, 2m - 1): internal nodes as they are made, weights ascending
    for (int i = 0; i < m; i++) S->weight[i] = freq[S->order[i]];
    int leaf = 0, inner = m, next = m;
    while (next < 2 * m - 1) {
        int pick[2];
        for (int j = 0; j < 2; j++) {  // the lighter head of the two queues; a leaf on a tie
            if (leaf < m && (inner >= next || S->weight[leaf] <= S->weight[inner])) pick[j] = leaf++;
            else pick[j] = inner++;
        }
        S->weight[next] = S->weight[pick[0]] + S->weight[pick[1]];
        S->parent[pick[0]] = S->parent[pick[1]] = (uint16_t)next;
        next++;
    }
    const int root = 2 * m - 2;
    // depths top down, cut at the limit; every NODE cut, leaf or not, counts as overflow (gen_bitlen's accounting: the tree
    // with all of them at the limit is over-subscribed by half that many codes of the limit's length)
    for (int b = 0; b < 16; b++) S->count[b] = 0;
    int overflow = 0;
    S->depth[root] = 0;
    for (int i = root - 1; i >= 0; i--) {
        int d = S->depth[S->parent[i]] + 1;
        if (d > limit) {
            d = limit;
            overflow++;
        }
        if (i >= m) S->depth[i] = (uint16_t)d;
        else S->count[d]++;
    }
    while (overflow > 0) {
        int bits = limit - 1;
        while (S->count[bits] == 0) bits--;
        S->count[bits]--;         // one leaf down a level ...
        S->count[bits + 1] += 2;  // ... beside one of the overflowing leaves
        S->count[limit]--;        // which takes a second of them off the limit's level
        overflow -= 2;
    }
    int i = 0;
    for (int bits = limit; bits >= 1; bits--)
        for (int c = S->count[bits]; c > 0; c--) len[S->order[i++]] = (uint8_t)bits;
}

UKM_HD void build_lengths(const uint32_t *freq, int n, int limit, Scratch *S, uint8_t *len) {
    const int m = sort_symbols(freq, n, S->order);
    lengths_from_sorted(freq, n, m, limit, S, len);
}

UKM_HD uint32_t bit_reverse(uint32_t v, int nbits) {
    uint32_t r = 0;
    for (int i = 0; i < nbits; i++) {
        r = (r << 1) | (v & 1u);
        v >>= 1;
    }
    return r;
}

// first[b] = the first canonical code of length b (RFC 1951 3.2.2), b = 1..15; first[0] unused
UKM_HD void first_codes(const uint8_t *len, int n, uint16_t *first) {
    uint16_t count[16];
    for (int b = 0; b < 16; b++) count[b] = 0;
    for (int s = 0; s < n; s++) count[len[s]]++;
    count[0] = 0;
    uint32_t code = 0;
    first[0] = 0;
    for (int b = 1; b < 16; b++) {
        code = (code + count[b - 1]) << 1;
        first[b] = (uint16_t)code;
    }
}

// code[s] = symbol s's canonical code, bit-reversed: deflate packs Huffman codes from their most significant bit, into bytes
// that fill from the least significant
UKM_HD void assign_codes(const uint8_t *len, int n, uint16_t *code) {
    uint16_t next[16];
    first_codes(len, n, next);
    for (int s = 0; s < n; s++) code[s] = len[s] ? (uint16_t)bit_reverse(next[len[s]]++, len[s]) : (uint16_t)0;
}

// Bits into a zeroed byte buffer, least significant first.  buf == nullptr: the bits are only counted.
struct BitWriter {
    uint8_t *buf;
    uint64_t pos;  // bits behind buf[0]'s bit 0
    UKM_HD void put(uint32_t v, int nbits) {
        if (buf) {
            uint64_t w = (uint64_t)v << (pos & 7);
            uint64_t b = pos >> 3;
            for (int left = nbits + (int)(pos & 7); left > 0; left -= 8, b++, w >>= 8) buf[b] |= (uint8_t)w;
        }
        pos += (uint64_t)nbits;
    }
};

struct HeaderScratch {  // working memory of block_header
    Scratch lengths;
    uint32_t cl_freq[CL_SYMS];
    uint16_t cl_code[CL_SYMS];
    uint16_t token[SEQ_LEN];  // code-length symbol | extra bits << 8
    uint8_t cl_len[CL_SYMS];
    uint8_t seq[SEQ_LEN];
};

// The header of one dynamic block of literals: BFINAL = 0, BTYPE = 10, HLIT = 257 codes (end-of-block always occurs, so
// none can be cut), HDIST = 1 code of one bit that is never used -- RFC 1951 3.2.7's form for "only one distance code" --,
// HCLEN, the code-length code in its permuted order, the 258 lengths with the run symbols 16 / 17 / 18.
UKM_HD void block_header(const uint8_t *litlen, HeaderScratch *H, BitWriter *w) {
    const uint8_t perm[CL_SYMS] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int s = 0; s < LIT_SYMS; s++) H->seq[s] = litlen[s];
    H->seq[LIT_SYMS] = 1;
    for (int s = 0; s < CL_SYMS; s++) H->cl_freq[s] = 0;
    int nt = 0;
    for (int i = 0; i < SEQ_LEN;) {
        const int v = H->seq[i];
        int run = 1;
        while (i + run < SEQ_LEN && H->seq[i + run] == v) run++;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const int r = run < 138 ? run : 138;
                H->token[nt++] = (uint16_t)(18 | ((r - 11) << 8));
                run -= r;
            }
            if (run >= 3) {
                H->token[nt++] = (uint16_t)(17 | ((run - 3) << 8));
                run = 0;
            }
        } else {
            H->token[nt++] = (uint16_t)v;
            run--;
            while (run >= 3) {
                const int r = run < 6 ? run : 6;
                H->token[nt++] = (uint16_t)(16 | ((r - 3) << 8));
                run -= r;
            }
        }
        for (; run > 0; run--) H->token[nt++] = (uint16_t)v;
    }
    for (int t = 0; t < nt; t++) H->cl_freq[H->token[t] & 255]++;
    build_lengths(H->cl_freq, CL_SYMS, CL_LIMIT, &H->lengths, H->cl_len);
    assign_codes(H->cl_len, CL_SYMS, H->cl_code);
    int hclen = CL_SYMS;
    while (hclen > 4 && H->cl_len[perm[hclen - 1]] == 0) hclen--;
    w->put(0, 1);  // BFINAL
    w->put(2, 2);  // BTYPE = 10
    w->put(LIT_SYMS - 257, 5);
    w->put(0, 5);  // HDIST - 1
    w->put((uint32_t)(hclen - 4), 4);
    for (int i = 0; i < hclen; i++) w->put(H->cl_len[perm[i]], 3);
    for (int t = 0; t < nt; t++) {
        const int sym = H->token[t] & 255, extra = H->token[t] >> 8;
        w->put(H->cl_code[sym], H->cl_len[sym]);
        if (sym == 16) w->put((uint32_t)extra, 2);
        else if (sym == 17) w->put((uint32_t)extra, 3);
        else if (sym == 18) w->put((uint32_t)extra, 7);
    }
}

// A chunk's dynamic form in bytes: header, the literals' bits, end-of-block, then the empty stored block that restores byte
// alignment (3 header bits, padding, 00 00 FF FF).
UKM_HD uint32_t dynamic_bytes(uint64_t header_bits, uint64_t literal_bits, int eob_len) {
    return (uint32_t)((header_bits + literal_bits + (uint64_t)eob_len + 3 + 7) / 8 + 4);
}

// ---- CRC-32 (reflected, polynomial EDB88320): polynomials over GF(2) with x^0 in bit 31 -------------------------------------
constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr uint32_t CRC_X0 = 0x80000000u, CRC_X8 = 0x00800000u;  // x^0, x^8

// a * b mod the polynomial
UKM_HD uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
// x^(8 n) mod the polynomial: what n more bytes multiply a CRC register by
UKM_HD uint32_t crc_x8n(uint64_t n) {
    uint32_t p = CRC_X0, sq = CRC_X8;
    for (; n; n >>= 1) {
        if (n & 1) p = crc_mul(p, sq);
        sq = crc_mul(sq, sq);
    }
    return p;
}
// entry b of the byte table: the register after byte b from a zero register
UKM_HD uint32_t crc_table_entry(uint32_t b) {
    for (int i = 0; i < 8; i++) b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    return b;
}
#if defined(__HIPCC__)
// A workgroup's raw CRC (zero register, no inversion) of len < 65536 bytes in LDS, from per-thread slices (ukm_deflate.hip: a
// chunk of the source; ukm_inflate.hip: a tile of the output).  tab[256], pow[16]: LDS, filled by 256 threads in front of a
// barrier; crc_slice: the raw CRC of B[lo, hi) times x^(8 * the bytes behind it): the XOR over all slices is the CRC of B.
__device__ inline void crc_lds_tables(uint32_t *tab, uint32_t *pow, int tid) {
    tab[tid] = crc_table_entry((uint32_t)tid);
    if (tid < 16) {  // x^(8 * 2^tid): what 2^tid more bytes multiply a CRC by
        uint32_t p = CRC_X8;
        for (int i = 0; i < tid; i++) p = crc_mul(p, p);
        pow[tid] = p;
    }
}
__device__ inline uint32_t crc_slice(const uint8_t *B, uint32_t lo, uint32_t hi, uint32_t len, const uint32_t *tab, const uint32_t *pow) {
    uint32_t c = 0;
    for (uint32_t p = lo; p < hi; p++) c = tab[(c ^ B[p]) & 255u] ^ (c >> 8);
    const uint32_t behind = len - hi;
    for (int k = 0; k < 16; k++)
        if ((behind >> k) & 1u) c = crc_mul(c, pow[k]);
    return c;
}
#endif

// The CRC-32 (as zlib's crc32 returns it) of A followed by B, from crc(A), the RAW CRC of B -- zero initial register, no final
// inversion -- and B's length: the register is linear in (register, data).
UKM_HD uint32_t crc_append_raw(uint32_t crc_a, uint32_t raw_b, uint64_t len_b) {
    return (crc_mul(crc_a ^ 0xFFFFFFFFu, crc_x8n(len_b)) ^ raw_b) ^ 0xFFFFFFFFu;
}
// the same from crc(B): zlib's crc32_combine
UKM_HD uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return crc_mul(crc_a, crc_x8n(len_b)) ^ crc_b; }

}  // namespace ukm_huff
