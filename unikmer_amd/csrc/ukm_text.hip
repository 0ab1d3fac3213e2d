// ukm_text.hip — ukm_view / ukm_dump: records to the text `unikmer view` prints, and the text `unikmer dump` reads back to
// records.  The byte-image machinery and the size-then-write protocol both calls follow are ukm_bytes.h's (shared with
// ukm_unik.hip and ukm_deflate.hip); neither call needs a look-back.
//
// view.  The one fixed-width case (UKM_VIEW_KMER of codes that are not hashed: k + 1 bytes a line) is one kernel, a tile of
// FIXV_RECS lines built in an LDS image and flushed as aligned 16-byte words.  Every other format has lines whose length
// depends on the data (decimal codes of 1..20 digits, decimal taxids of 1..10), size-then-write (ukm_bytes.h: SizeScan):
//   size:  view_sum_kernel, the bytes of a tile of VIEW_RECS records (digit counts from comparisons against the powers of ten),
//   write: view_write_kernel scans the lengths of its records in LDS, builds the lines in the image, flushes it.
// Both take a thread's records and their bytes from view_load: the offsets of the second pass are the sizes of the first.
// The image is sized by the longest line the format can give (VIEW_RECS x 32, 64 or 121 bytes: three instantiations), so
// the short formats do not pay the LDS of FASTQ.
//
// dump.  Tiles of DUMP_TILE text bytes, one byte in front (does position 0 start a line?) and DUMP_TAIL bytes behind (a
// line belongs to the tile it starts in, and a legal line is at most DUMP_LINE bytes with its LF).  Line starts are locally
// decidable -- the byte in front is an LF, or it is offset 0 -- so every thread looks at DUMP_VT consecutive positions, the
// starts found are compacted in LDS (one scan), and thread i parses line i: a wave parses 64 lines at once, where parsing at
// the positions themselves would run the parser once for every position a lane holds, each time for the few lanes at a start.
//   size:  dump_count_kernel, records per tile; the lowest start of a line outside the grammar by a 64-bit atomicMin into
//          the protocol's flag word,
//   write: dump_write_kernel parses again, ranks the tile's records in LDS (line order), stores codes and taxids.
#include <algorithm>

#include "ukm_bytes.h"

namespace {

constexpr int FIXV_RECS = 1024;  // lines per tile of the fixed-width view
constexpr int FIXV_IMG = FIXV_RECS * 33 + 32;
constexpr int VIEW_RECS = 512;   // records per tile of every other view
constexpr int VIEW_VT = VIEW_RECS / NT;
constexpr int VIEW_LINE_MAX = 121;  // FASTQ of hashed codes, k = 64, with taxid: 1 + 20 + 1 + 10 + 1 + 20 + 1 + 2 + 64 + 1
constexpr int DUMP_TILE = 2048;  // text bytes per tile
constexpr int DUMP_VT = DUMP_TILE / NT;
constexpr int DUMP_LINES = DUMP_TILE / 2;  // lines of a tile that hold a byte: a byte and its LF each
constexpr int DUMP_LVT = DUMP_LINES / NT;
constexpr int DUMP_LINE = 45;    // the longest legal line: 32 + TAB + 10 + CR + LF
constexpr int DUMP_TAIL = DUMP_LINE - 1;
constexpr int DUMP_IMG = 1 + DUMP_TILE + DUMP_TAIL + 19;  // + up to 15 bytes of alignment shift, rounded to 16
static_assert(FIXV_IMG % 16 == 0 && DUMP_IMG % 16 == 0 && DUMP_IMG >= 1 + DUMP_TILE + DUMP_TAIL + 15, "LDS images are whole 16-byte words");
static_assert(FIXV_IMG <= 65536 && VIEW_RECS * VIEW_LINE_MAX + 32 + NT * 4 <= 65536, "static LDS");

constexpr u32 FMT_MASK = 15u;

// ---- view -------------------------------------------------------------------------------------------------------------------
__device__ inline u32 dec_len64(u64 v) {
    u32 n = 1;
    u64 p = 10;
#pragma unroll
    for (int i = 1; i < 20; i++) {
        n += v >= p ? 1u : 0u;
        p *= 10;
    }
    return n;
}
__device__ inline u32 dec_len32(u32 v) {
    u32 n = 1, p = 10;
#pragma unroll
    for (int i = 1; i < 10; i++) {
        n += v >= p ? 1u : 0u;
        p *= 10;
    }
    return n;
}
// v as nd decimal digits at B[at, at + nd)
__device__ inline u32 put_dec(u8 *B, u32 at, u64 v, u32 nd) {
    for (u32 p = at + nd; p > at;) {
        const u64 q = v / 10;
        B[--p] = (u8)('0' + (u32)(v - q * 10));
        v = q;
    }
    return at + nd;
}
__device__ inline u32 put_kmer(u8 *B, u32 at, u64 code, int k) {
    for (int i = 0; i < k; i++) {
        const u32 b = (u32)(code >> (2 * (k - 1 - i))) & 3u;
        B[at + (u32)i] = (u8)((0x54474341u >> (8 * b)) & 255u);  // "ACGT"
    }
    return at + (u32)k;
}

struct ViewFmt {
    u32 base;     // UKM_VIEW_*
    u32 with_t;   // FASTA / FASTQ: the taxid in the header line
    int k, hashed;
};
__device__ inline u32 view_len(const ViewFmt f, u64 code, u32 taxid) {
    const u32 dc = dec_len64(code), dt = dec_len32(taxid), kl = f.hashed ? dc : (u32)f.k;
    switch (f.base) {
    case UKM_VIEW_KMER: return kl + 1;
    case UKM_VIEW_KMER_CODE: return kl + dc + 2;
    case UKM_VIEW_CODE: return dc + 1;
    case UKM_VIEW_KMER_TAXID: return kl + dt + 2;
    case UKM_VIEW_TAXID: return dt + 1;
    case UKM_VIEW_FASTA: return 1 + dc + (f.with_t ? 1 + dt : 0) + 1 + kl + 1;
    default: return 1 + dc + (f.with_t ? 1 + dt : 0) + 1 + kl + 1 + 2 + (u32)f.k + 1;  // FASTQ
    }
}
// a thread's VIEW_VT records from record r0 on (zeros behind record n - 1) and the bytes of their lines
__device__ inline u32 view_load(const u64 *keys, const u32 *tax, u32 file_taxid, u64 n, const ViewFmt f, u64 r0, u64 *code, u32 *tx) {
    u32 bytes = 0;
#pragma unroll
    for (int s = 0; s < VIEW_VT; s++) {
        code[s] = 0;
        tx[s] = 0;
        if (r0 + s >= n) continue;
        code[s] = keys[r0 + s];
        tx[s] = tax ? tax[r0 + s] : file_taxid;
        bytes += view_len(f, code[s], tx[s]);
    }
    return bytes;
}
__device__ inline u32 put_K(u8 *B, u32 at, const ViewFmt f, u64 code, u32 dc) {
    return f.hashed ? put_dec(B, at, code, dc) : put_kmer(B, at, code, f.k);
}
__device__ inline u32 view_put(u8 *B, u32 at, const ViewFmt f, u64 code, u32 taxid) {
    const u32 dc = dec_len64(code), dt = dec_len32(taxid);
    switch (f.base) {
    case UKM_VIEW_KMER:
        at = put_K(B, at, f, code, dc);
        break;
    case UKM_VIEW_KMER_CODE:
        at = put_K(B, at, f, code, dc);
        B[at++] = '\t';
        at = put_dec(B, at, code, dc);
        break;
    case UKM_VIEW_CODE:
        at = put_dec(B, at, code, dc);
        break;
    case UKM_VIEW_KMER_TAXID:
        at = put_K(B, at, f, code, dc);
        B[at++] = '\t';
        at = put_dec(B, at, taxid, dt);
        break;
    case UKM_VIEW_TAXID:
        at = put_dec(B, at, taxid, dt);
        break;
    default:  // FASTA, FASTQ
        B[at++] = f.base == UKM_VIEW_FASTA ? '>' : '@';
        at = put_dec(B, at, code, dc);
        if (f.with_t) {
            B[at++] = ' ';
            at = put_dec(B, at, taxid, dt);
        }
        B[at++] = '\n';
        at = put_K(B, at, f, code, dc);
        if (f.base == UKM_VIEW_FASTQ) {
            B[at++] = '\n';
            B[at++] = '+';
            B[at++] = '\n';
            for (int i = 0; i < f.k; i++) B[at++] = 'g';
        }
        break;
    }
    B[at++] = '\n';
    return at;
}

__global__ __launch_bounds__(NT) void view_fixed_kernel(const u64 *keys, u64 n, int k, u8 *out) {
    __shared__ uint4 s_img[FIXV_IMG / 16];
    const int tid = (int)threadIdx.x;
    const u64 r0 = (u64)blockIdx.x * FIXV_RECS;
    const u32 m = (u32)(n - r0 < (u64)FIXV_RECS ? n - r0 : (u64)FIXV_RECS);
    const u32 R = (u32)k + 1u;
    u8 *dst = out + r0 * R;
    int shift;
    u8 *B = image_at(dst, s_img, &shift);
    for (u32 r = (u32)tid; r < m; r += NT) {
        const u32 at = put_kmer(B, r * R, keys[r0 + r], k);
        B[at] = '\n';
    }
    __syncthreads();
    flush_image(dst, m * R, s_img, shift, tid);
}

__global__ __launch_bounds__(NT) void view_sum_kernel(const u64 *keys, const u32 *tax, u32 file_taxid, u64 n, ViewFmt f, u32 *sums) {
    __shared__ u32 s_scan[SCAN_LDS];
    const int tid = (int)threadIdx.x;
    u64 code[VIEW_VT];
    u32 tx[VIEW_VT];
    const u32 bytes = view_load(keys, tax, file_taxid, n, f, (u64)blockIdx.x * VIEW_RECS + (u64)tid * VIEW_VT, code, tx);
    u32 total;
    (void)block_excl_scan_u32<NT>(bytes, s_scan, &total);
    if (tid == 0) sums[blockIdx.x] = total;
}

// LINE: no line of the format is longer
template <int LINE>
__global__ __launch_bounds__(NT) void view_write_kernel(const u64 *keys, const u32 *tax, u32 file_taxid, u64 n, ViewFmt f, const u64 *offs,
                                                        u8 *out) {
    __shared__ uint4 s_img[(VIEW_RECS * LINE + 32) / 16];
    __shared__ u32 s_scan[SCAN_LDS];
    const int tid = (int)threadIdx.x;
    const u64 r0 = (u64)blockIdx.x * VIEW_RECS + (u64)tid * VIEW_VT;
    u64 code[VIEW_VT];
    u32 tx[VIEW_VT];
    const u32 bytes = view_load(keys, tax, file_taxid, n, f, r0, code, tx);
    u32 total;
    u32 at = block_excl_scan_u32<NT>(bytes, s_scan, &total);
    // one register: left alone the compiler carries `at` as the wave scan's ten unsummed terms through view_put (88 VGPRs
    // where 80 give six waves a SIMD)
    asm volatile("" : "+v"(at));
    u8 *dst = out + offs[blockIdx.x];
    int shift;
    u8 *B = image_at(dst, s_img, &shift);
#pragma unroll
    for (int s = 0; s < VIEW_VT; s++) {
        if (r0 + s >= n) break;
        at = view_put(B, at, f, code[s], tx[s]);
    }
    __syncthreads();
    flush_image(dst, total, s_img, shift, tid);
}

// the longest line of a format, codes and taxids at their widest
u32 view_line_max(u32 base, bool with_t, int k, bool hashed) {
    const u32 dc = 20, dt = 10, kl = hashed ? dc : (u32)k;
    switch (base) {
    case UKM_VIEW_KMER: return kl + 1;
    case UKM_VIEW_KMER_CODE: return kl + dc + 2;
    case UKM_VIEW_CODE: return dc + 1;
    case UKM_VIEW_KMER_TAXID: return kl + dt + 2;
    case UKM_VIEW_TAXID: return dt + 1;
    case UKM_VIEW_FASTA: return 1 + dc + (with_t ? 1 + dt : 0) + 1 + kl + 1;
    case UKM_VIEW_FASTQ: return 1 + dc + (with_t ? 1 + dt : 0) + 1 + kl + 1 + 2 + (u32)k + 1;
    default: return VIEW_LINE_MAX;
    }
}

// ---- dump -------------------------------------------------------------------------------------------------------------------
enum : int { LN_NONE = 0, LN_REC = 1, LN_BAD = 2 };

__device__ inline int base2bit(u32 c) {  // host/seqtext.hpp: base2bit
    switch (c | 32u) {  // (a byte that gives a lower-case letter here is that letter, in one case or the other)
    case 'a': case 'n': case 'm': case 'v': case 'h': case 'r': case 'd': case 'w': return 0;
    case 'c': case 's': case 'b': case 'y': return 1;
    case 'g': case 'k': return 2;
    case 't': case 'u': return 3;
    default: return 4;
    }
}
__device__ inline u64 revcomp(u64 code, int k) {  // host/seqtext.hpp: revcomp
    u64 c = ~code;
    c = ((c >> 2) & 0x3333333333333333ull) | ((c & 0x3333333333333333ull) << 2);
    c = ((c >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((c & 0x0F0F0F0F0F0F0F0Full) << 4);
    c = __builtin_bswap64(c);
    return c >> (64 - 2 * k);
}

// The line that starts at L[0]: `avail` bytes may be looked at (at most DUMP_LINE, never one at or beyond the end of the
// text), `to_end`: they reach the end of the text.
__device__ inline int parse_line(const u8 *L, u32 avail, bool to_end, int k, u32 flags, u64 *code, u32 *taxid) {
    u32 len = 0, f1 = ~0u;  // the line's bytes; the first TAB
    for (; len < avail; len++) {
        const u32 b = L[len];
        if (b == '\n') break;
        if (b == '\t' && f1 == ~0u) f1 = len;
    }
    if (len == avail && !to_end) return LN_BAD;  // no LF within the longest legal line
    if (len && L[len - 1] == '\r') len--;
    if (len == 0) return LN_NONE;
    if (f1 > len) f1 = len;
    u64 c = 0;
    if (flags & UKM_DUMP_DECIMAL) {
        if (f1 < 1 || f1 > 20) return LN_BAD;
        for (u32 i = 0; i < f1; i++) {
            const u32 d = (u32)L[i] - '0';
            if (d > 9u) return LN_BAD;
            if (c > (~0ull - d) / 10) return LN_BAD;
            c = c * 10 + d;
        }
    } else {
        if (f1 != (u32)k) return LN_BAD;
        for (u32 i = 0; i < f1; i++) {
            const int b = base2bit(L[i]);
            if (b > 3) return LN_BAD;
            c = (c << 2) | (u64)b;
        }
    }
    u32 t = 0;
    if (flags & UKM_DUMP_TAXID) {
        if (f1 == len) return LN_BAD;  // no TAB
        const u32 n2 = len - f1 - 1;
        if (n2 < 1 || n2 > 10) return LN_BAD;
        u64 v = 0;
        for (u32 i = f1 + 1; i < len; i++) {
            const u32 d = (u32)L[i] - '0';
            if (d > 9u) return LN_BAD;
            v = v * 10 + d;
        }
        if (v > 0xFFFFFFFFull) return LN_BAD;
        t = (u32)v;
    } else if (f1 != len) {
        return LN_BAD;  // a TAB
    }
    if (flags & (UKM_DUMP_CANONICAL | UKM_DUMP_CANONICAL_ONLY)) {
        const u64 rc = revcomp(c, k);
        if (flags & UKM_DUMP_CANONICAL_ONLY) {
            if (rc < c) return LN_NONE;
        } else if (rc < c) {
            c = rc;
        }
    }
    *code = c;
    *taxid = t;
    return LN_REC;
}

// the tile's text in LDS; returns B with B[i] = text[start + i] for -1 (where start > 0) <= i < min(n_bytes - start, tile + tail)
__device__ inline const u8 *dump_load(const u8 *text, u64 n_bytes, u64 start, uint4 *img, int tid) {
    const u64 lo = start ? start - 1 : 0;
    const u64 hi = n_bytes - start < (u64)(DUMP_TILE + DUMP_TAIL) ? n_bytes : start + (u64)(DUMP_TILE + DUMP_TAIL);
    const int shift = load_image(text, lo, (u32)(hi - lo), img, tid);
    return (const u8 *)img + shift + (start - lo);
}
// The starts of the tile's lines that hold a byte, in order, into s_start; returns their number.  Two of them are at least
// two bytes apart: at most DUMP_LINES.  All threads of the workgroup call this together.
__device__ inline u32 dump_starts(const u8 *B, u64 n_bytes, u64 start, unsigned short *s_start, u32 *s_scan, int tid) {
    u32 mask = 0;
    for (int j = 0; j < DUMP_VT; j++) {
        const u32 p = (u32)(tid * DUMP_VT + j);
        const u64 at = start + p;
        if (at < n_bytes && (at == 0 || B[(int)p - 1] == '\n') && B[p] != '\n') mask |= 1u << j;
    }
    u32 total;
    u32 r = block_excl_scan_u32<NT>((u32)__popc(mask), s_scan, &total);
    for (int j = 0; j < DUMP_VT; j++)
        if (mask & (1u << j)) s_start[r++] = (unsigned short)(tid * DUMP_VT + j);
    __syncthreads();
    return total;
}
// the line that starts at position p of the tile
__device__ inline int dump_line(const u8 *B, u64 n_bytes, u64 start, u32 p, int k, u32 flags, u64 *code, u32 *taxid) {
    const u64 rest = n_bytes - (start + p);
    const u32 avail = rest < (u64)DUMP_LINE ? (u32)rest : (u32)DUMP_LINE;
    return parse_line(B + p, avail, rest <= (u64)DUMP_LINE, k, flags, code, taxid);
}

__global__ __launch_bounds__(NT) void dump_count_kernel(const u8 *text, u64 n_bytes, int k, u32 flags, u32 *sums, u64 *ctl) {
    __shared__ uint4 s_img[DUMP_IMG / 16];
    __shared__ unsigned short s_start[DUMP_LINES];
    __shared__ u32 s_scan[SCAN_LDS];
    const int tid = (int)threadIdx.x;
    const u64 start = (u64)blockIdx.x * DUMP_TILE;
    const u8 *B = dump_load(text, n_bytes, start, s_img, tid);
    __syncthreads();
    const u32 nl = dump_starts(B, n_bytes, start, s_start, s_scan, tid);
    u32 cnt = 0;
    u64 bad = ~0ull;
    for (u32 i = (u32)tid; i < nl; i += NT) {  // line i by thread i: the parsing lanes are neighbours
        const u32 p = s_start[i];
        u64 code;
        u32 taxid;
        const int r = dump_line(B, n_bytes, start, p, k, flags, &code, &taxid);
        cnt += r == LN_REC ? 1u : 0u;
        if (r == LN_BAD && bad == ~0ull) bad = start + p;
    }
    u32 total;
    (void)block_excl_scan_u32<NT>(cnt, s_scan, &total);
    if (tid == 0) sums[blockIdx.x] = total;
    if (bad != ~0ull) atomicMin((unsigned long long *)&ctl[1], (unsigned long long)bad);
}

__global__ __launch_bounds__(NT) void dump_write_kernel(const u8 *text, u64 n_bytes, int k, u32 flags, const u64 *offs, u64 *out_keys,
                                                        u32 *out_tax) {
    __shared__ uint4 s_img[DUMP_IMG / 16];
    __shared__ u64 s_code[DUMP_LINES];
    __shared__ u32 s_tax[DUMP_LINES];
    __shared__ unsigned short s_start[DUMP_LINES];
    __shared__ u8 s_rec[DUMP_LINES];
    __shared__ u32 s_scan[SCAN_LDS];
    const int tid = (int)threadIdx.x;
    const u64 start = (u64)blockIdx.x * DUMP_TILE;
    const u8 *B = dump_load(text, n_bytes, start, s_img, tid);
    __syncthreads();
    const u32 nl = dump_starts(B, n_bytes, start, s_start, s_scan, tid);
    for (u32 i = (u32)tid; i < nl; i += NT) {
        u64 code = 0;
        u32 taxid = 0;
        const bool rec = dump_line(B, n_bytes, start, s_start[i], k, flags, &code, &taxid) == LN_REC;
        s_rec[i] = rec ? 1 : 0;
        s_code[i] = code;
        s_tax[i] = taxid;
    }
    __syncthreads();
    // line order is record order: thread t ranks lines [t * DUMP_LVT, (t + 1) * DUMP_LVT)
    const u32 i0 = (u32)tid * DUMP_LVT;
    u32 cnt = 0;
    for (u32 i = i0; i < i0 + DUMP_LVT && i < nl; i++) cnt += s_rec[i];
    u32 total;
    u64 o = offs[blockIdx.x] + block_excl_scan_u32<NT>(cnt, s_scan, &total);
    for (u32 i = i0; i < i0 + DUMP_LVT && i < nl; i++) {
        if (!s_rec[i]) continue;
        out_keys[o] = s_code[i];
        if (out_tax) out_tax[o] = s_tax[i];
        o++;
    }
}

}  // namespace

extern "C" uint64_t ukm_view_bound(uint64_t n, int k, int hashed, uint32_t format) {
    const int kk = std::min(std::max(k, 1), hashed ? 64 : 32);
    return n * (u64)view_line_max(format & FMT_MASK, (format & UKM_VIEW_WITH_TAXID) != 0, kk, hashed != 0);
}

extern "C" int ukm_view(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint32_t file_taxid, uint64_t n, int k, int hashed,
                        uint32_t format, uint8_t *out_bytes, uint64_t out_cap, uint64_t *n_out) {
    const char *name = "ukm_view";
    if (!ctx || !n_out || (!keys && n) || (!out_bytes && out_cap)) UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
    *n_out = 0;
    const u32 base = format & FMT_MASK;
    const bool with_t = (format & UKM_VIEW_WITH_TAXID) != 0;
    if ((format & ~(FMT_MASK | UKM_VIEW_WITH_TAXID)) || base > UKM_VIEW_FASTQ) UKM_FAIL(UKM_ERR_INVALID, "%s: unknown format %u", name, format);
    if (with_t && base != UKM_VIEW_FASTA && base != UKM_VIEW_FASTQ)
        UKM_FAIL(UKM_ERR_INVALID, "%s: UKM_VIEW_WITH_TAXID goes with UKM_VIEW_FASTA and UKM_VIEW_FASTQ only", name);
    if (k < 1 || k > (hashed ? 64 : 32)) UKM_FAIL(UKM_ERR_K, "%s: k = %d, must be 1..%d", name, k, hashed ? 64 : 32);
    if (n == 0) return UKM_OK;
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        const u64 *dk = nullptr;
        const u32 *dt = nullptr;
        u8 *ob = nullptr;
        if (base == UKM_VIEW_KMER && !hashed) {
            const u64 need = n * (u64)(k + 1);
            UKM_TRY(out_fits(name, "the text takes", "bytes", need, out_cap, n_out));
            const u64 nblocks = (n + FIXV_RECS - 1) / FIXV_RECS;
            if (nblocks > MAX_GRID) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu records in one call", name, (unsigned long long)n);
            UKM_TRY(ukm_in_t(ctx, keys, n, &dk));
            UKM_TRY(ukm_out_t(ctx, out_bytes, need, &ob));
            hipLaunchKernelGGL(view_fixed_kernel, dim3((unsigned)nblocks), dim3(NT), 0, ctx->stream, dk, n, k, ob);
            UKM_HIP(hipGetLastError());
            return UKM_OK;
        }
        const u64 ntiles = (n + VIEW_RECS - 1) / VIEW_RECS;
        if (ntiles > MAX_GRID) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu records in one call", name, (unsigned long long)n);
        ViewFmt f;
        f.base = base;
        f.with_t = with_t ? 1u : 0u;
        f.k = k;
        f.hashed = hashed ? 1 : 0;
        UKM_TRY(ukm_in_t(ctx, keys, n, &dk));
        const bool uses_t = base == UKM_VIEW_KMER_TAXID || base == UKM_VIEW_TAXID || with_t;
        if (taxids && uses_t) UKM_TRY(ukm_in_t(ctx, taxids, n, &dt));
        SizeScan z;
        UKM_TRY(size_alloc(ctx, ntiles, -1, &z));
        hipLaunchKernelGGL(view_sum_kernel, dim3((unsigned)ntiles), dim3(NT), 0, ctx->stream, dk, dt, file_taxid, n, f, z.sums);
        UKM_TRY(size_scan(ctx, ntiles, &z));
        UKM_TRY(out_fits(name, "the text takes", "bytes", z.total, out_cap, n_out));
        UKM_TRY(ukm_out_t(ctx, out_bytes, z.total, &ob));
        write_begins(ctx);
        const u32 line = view_line_max(base, with_t, k, hashed != 0);
        const dim3 grid((unsigned)ntiles), block(NT);
        const u64 *offs = z.offs;
        if (line <= 32)
            hipLaunchKernelGGL(view_write_kernel<32>, grid, block, 0, ctx->stream, dk, dt, file_taxid, n, f, offs, ob);
        else if (line <= 64)
            hipLaunchKernelGGL(view_write_kernel<64>, grid, block, 0, ctx->stream, dk, dt, file_taxid, n, f, offs, ob);
        else
            hipLaunchKernelGGL(view_write_kernel<VIEW_LINE_MAX>, grid, block, 0, ctx->stream, dk, dt, file_taxid, n, f, offs, ob);
        UKM_HIP(hipGetLastError());
        return UKM_OK;
    }();
    return ukm_finish(&s, rc);
}

extern "C" int ukm_dump(ukm_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int k, uint32_t flags, uint64_t *out_keys,
                        uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out, uint64_t *bad_off) {
    const char *name = "ukm_dump";
    if (!ctx || !n_out || (!text && n_bytes) || (!out_keys && out_cap)) UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
    *n_out = 0;
    const u32 all = UKM_DUMP_TAXID | UKM_DUMP_DECIMAL | UKM_DUMP_CANONICAL | UKM_DUMP_CANONICAL_ONLY;
    if (flags & ~all) UKM_FAIL(UKM_ERR_INVALID, "%s: unknown flags %u", name, flags);
    if ((flags & UKM_DUMP_DECIMAL) && (flags & (UKM_DUMP_CANONICAL | UKM_DUMP_CANONICAL_ONLY)))
        UKM_FAIL(UKM_ERR_INVALID, "%s: decimal codes have no canonical form", name);
    if (!(flags & UKM_DUMP_DECIMAL) && (k < 1 || k > 32)) UKM_FAIL(UKM_ERR_K, "%s: k = %d, must be 1..32", name, k);
    if (n_bytes == 0) return UKM_OK;
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        const u64 ntiles = (n_bytes + DUMP_TILE - 1) / DUMP_TILE;
        if (ntiles > MAX_GRID) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu bytes in one call", name, (unsigned long long)n_bytes);
        const u8 *b = nullptr;
        UKM_TRY(ukm_in_t(ctx, text, n_bytes, &b));
        SizeScan z;
        UKM_TRY(size_alloc(ctx, ntiles, 0xFF, &z));  // the flag: the lowest bad line start, none yet
        hipLaunchKernelGGL(dump_count_kernel, dim3((unsigned)ntiles), dim3(NT), 0, ctx->stream, b, n_bytes, k, flags, z.sums, z.ctl);
        UKM_TRY(size_scan(ctx, ntiles, &z));
        if (z.flag != ~0ull) {
            if (bad_off) *bad_off = z.flag;
            UKM_FAIL(UKM_ERR_FORMAT, "%s: the line at byte %llu is not %s", name, (unsigned long long)z.flag,
                     (flags & UKM_DUMP_TAXID) ? "a code, a TAB and a taxid" : "a code");
        }
        UKM_TRY(out_fits(name, "the text holds", "records", z.total, out_cap, n_out));
        if (z.total == 0) return UKM_OK;
        u64 *ok = nullptr;
        u32 *ot = nullptr;
        UKM_TRY(ukm_out_t(ctx, out_keys, z.total, &ok));
        if (out_taxids) UKM_TRY(ukm_out_t(ctx, out_taxids, z.total, &ot));
        write_begins(ctx);
        hipLaunchKernelGGL(dump_write_kernel, dim3((unsigned)ntiles), dim3(NT), 0, ctx->stream, b, n_bytes, k, flags, (const u64 *)z.offs, ok, ot);
        UKM_HIP(hipGetLastError());
        return UKM_OK;
    }();
    return ukm_finish(&s, rc);
}
