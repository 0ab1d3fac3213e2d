// ukm_deflate.hip — ukm_deflate: bytes to a byte-aligned run of RFC 1951 blocks, Huffman coding only, in independent chunks.
// A sorted .unik body is delta bytes: LZ77 finds nothing in it, all that zlib gains there is its Huffman code.
//
// The source is cut into chunks of DFL_CHUNK bytes.  A chunk becomes ONE dynamic block of literals and end-of-block followed
// by an empty stored block (the sync-flush marker 00 00 FF FF, which restores byte alignment) -- or, where that would not be
// smaller, one stored block of the chunk's bytes: 5 bytes more than the input and never worse.  Chunks start and end on byte
// boundaries, so their outputs concatenate.  Size-then-write (ukm_bytes.h: SizeScan), no look-back:
//   1. dfl_sum_kernel, a workgroup per chunk: the chunk to LDS as aligned 16-byte words (load_image), a histogram in LDS
//      with a private copy per wave, the chunk's raw CRC-32 from per-thread slices, the used symbols ranked by (frequency,
//      symbol) by all threads, then ONE lane merges the Huffman tree, limits the lengths (ukm_huff.h) and sizes the block
//      header; the chunk's output size, its 257 code lengths, its stored-or-dynamic choice and its raw CRC go to the workspace.
//   2. the protocol's scan and capacity step: the size query and a capacity failure end here.  Behind them the chunks' CRCs
//      are read back and combined on the host.
//   3. dfl_write_kernel, a workgroup per chunk: canonical codes from the stored lengths, one lane writes the block header into
//      a zeroed LDS image that starts at the output's address mod 16, every thread sizes its slice, a workgroup scan gives
//      bit offsets, the codes are OR-ed into the image 32 bits at a time, flush_image writes whole aligned words with a head
//      and a tail of single bytes.
// OR and integer counts commute: the output is a pure function of the input bytes.
#include <algorithm>
#include <vector>

#include "ukm_bytes.h"
#include "ukm_huff.h"

namespace {

namespace H = ukm_huff;

constexpr int DFL_CHUNK = 32768;  // source bytes per chunk: at most 65535, a chunk must fit one stored block
constexpr int DFL_VT = DFL_CHUNK / NT;         // bytes of a thread's slice
constexpr int DFL_STORED = 5;                  // bytes a stored block adds: 00, LEN, NLEN
constexpr int DFL_IN_IMG = DFL_CHUNK + 16;     // up to 15 bytes of alignment shift, rounded to 16
constexpr int DFL_OUT_IMG = DFL_CHUNK + 32;    // ... and DFL_STORED
constexpr int DFL_META = 264;                  // workspace bytes per chunk: 257 code lengths, [257] = 1: stored
constexpr int DFL_WAVES = NT / 64;
static_assert(DFL_CHUNK <= 65535 && DFL_CHUNK % NT == 0 && DFL_VT * NT == DFL_CHUNK, "chunk size");
static_assert(NT == 256, "one thread per byte value");
static_assert(DFL_IN_IMG % 16 == 0 && DFL_OUT_IMG % 16 == 0 && DFL_META % 4 == 0 && DFL_META > H::LIT_SYMS, "LDS images are whole 16-byte words");
static_assert(DFL_CHUNK + DFL_STORED + 15 <= DFL_OUT_IMG, "the largest chunk output at the largest shift fits its image");

__device__ inline u32 chunk_len(u64 n_bytes, u64 chunk) {
    const u64 rest = n_bytes - chunk * (u64)DFL_CHUNK;
    return (u32)(rest < (u64)DFL_CHUNK ? rest : (u64)DFL_CHUNK);
}

__global__ __launch_bounds__(NT) void dfl_sum_kernel(const u8 *src, u64 n_bytes, u32 *sums, u8 *meta, u32 *crcs) {
    __shared__ uint4 s_img[DFL_IN_IMG / 16];
    __shared__ H::HeaderScratch s_hs;
    __shared__ u32 s_hist[DFL_WAVES * H::LIT_SYMS];
    __shared__ u32 s_freq[H::LIT_SYMS];
    __shared__ u32 s_tab[256], s_pow[16], s_scan[SCAN_LDS];
    __shared__ u32 s_len32[DFL_META / 4];
    __shared__ u32 s_crc, s_used, s_hdr_bits;
    u8 *s_len = (u8 *)s_len32;
    const int tid = (int)threadIdx.x;
    const u64 chunk = blockIdx.x;
    const u32 len = chunk_len(n_bytes, chunk);
    const int shift = load_image(src, chunk * (u64)DFL_CHUNK, len, s_img, tid);
    for (int i = tid; i < DFL_WAVES * H::LIT_SYMS; i += NT) s_hist[i] = 0;
    for (int i = tid; i < DFL_META / 4; i += NT) s_len32[i] = 0;
    H::crc_lds_tables(s_tab, s_pow, tid);
    if (tid == 0) s_crc = s_used = 0;
    __syncthreads();
    // histogram: the image's 4-byte words, bytes outside [shift, shift + len) masked; a copy of the bins per wave
    {
        u32 *hist = s_hist + (tid >> 6) * H::LIT_SYMS;
        const u32 *words = (const u32 *)s_img;
        const u32 nwords = ((u32)shift + len + 3u) >> 2;
        for (u32 w = (u32)tid; w < nwords; w += NT) {
            const u32 v = words[w];
            for (u32 j = 0; j < 4; j++)
                if (w * 4u + j - (u32)shift < len) atomicAdd(&hist[(v >> (8u * j)) & 255u], 1u);
        }
    }
    // the raw CRC (zero register, no inversion) of this thread's slice, times x^(8 * bytes behind it in the chunk)
    {
        const u8 *B = (const u8 *)s_img + shift;
        const u32 lo = (u32)tid * DFL_VT;
        if (lo < len) {
            const u32 hi = lo + DFL_VT < len ? lo + DFL_VT : len;
            atomicXor(&s_crc, H::crc_slice(B, lo, hi, len, s_tab, s_pow));
        }
    }
    __syncthreads();
    for (int s = tid; s < H::LIT_SYMS; s += NT) {
        u32 f = 1;  // end-of-block
        if (s < 256) {
            f = 0;
            for (int w = 0; w < DFL_WAVES; w++) f += s_hist[w * H::LIT_SYMS + s];
        }
        s_freq[s] = f;
    }
    __syncthreads();
    // the used symbols by (frequency, symbol): every symbol counts those in front of it
    for (int s = tid; s < H::LIT_SYMS; s += NT) {
        const u32 f = s_freq[s];
        if (!f) continue;
        u32 rank = 0;
        for (int q = 0; q < H::LIT_SYMS; q++) {
            const u32 fq = s_freq[q];
            rank += (fq && (fq < f || (fq == f && q < s))) ? 1u : 0u;
        }
        s_hs.lengths.order[rank] = (unsigned short)s;
        atomicAdd(&s_used, 1u);
    }
    __syncthreads();
    if (tid == 0) {
        H::lengths_from_sorted(s_freq, H::LIT_SYMS, (int)s_used, H::LIT_LIMIT, &s_hs.lengths, s_len);
        H::BitWriter count = {nullptr, 0};
        H::block_header(s_len, &s_hs, &count);
        s_hdr_bits = (u32)count.pos;
    }
    __syncthreads();
    u32 literal_bits;
    (void)block_excl_scan_u32<NT>(s_freq[tid] * (u32)s_len[tid], s_scan, &literal_bits);
    if (tid == 0) {
        const u32 dynamic = H::dynamic_bytes(s_hdr_bits, literal_bits, s_len[H::EOB]), stored = len + (u32)DFL_STORED;
        const bool keep = dynamic < stored;
        s_len[H::LIT_SYMS] = keep ? 0 : 1;
        sums[chunk] = keep ? dynamic : stored;
        crcs[chunk] = s_crc;
    }
    __syncthreads();
    u32 *m = (u32 *)(meta + chunk * (u64)DFL_META);
    for (int i = tid; i < DFL_META / 4; i += NT) m[i] = s_len32[i];
}

// n <= 32 bits at bit `pos` of a zeroed image
__device__ inline void or_bits(u32 *img, u32 pos, u32 v, u32 n) {
    const u32 w = pos >> 5, sh = pos & 31u;
    atomicOr(&img[w], v << sh);
    if (sh + n > 32u) atomicOr(&img[w + 1], v >> (32u - sh));
}

__global__ __launch_bounds__(NT) void dfl_write_kernel(const u8 *src, u64 n_bytes, const u8 *meta, const u64 *offs, const u32 *sums, u8 *out) {
    __shared__ uint4 s_in[DFL_IN_IMG / 16];
    __shared__ uint4 s_out[DFL_OUT_IMG / 16];
    __shared__ H::HeaderScratch s_hs;
    __shared__ u32 s_code[H::LIT_SYMS];  // code | length << 16
    __shared__ u32 s_len32[DFL_META / 4];
    __shared__ u32 s_scan[SCAN_LDS];
    __shared__ u32 s_count[16], s_first[16];
    __shared__ u32 s_hdr_end;
    const u8 *s_len = (const u8 *)s_len32;
    const int tid = (int)threadIdx.x;
    const u64 chunk = blockIdx.x;
    const u32 len = chunk_len(n_bytes, chunk);
    const u32 nbytes = sums[chunk];
    u8 *dst = out + offs[chunk];
    int shift;
    u8 *O = image_at(dst, s_out, &shift);
    const int shift_in = load_image(src, chunk * (u64)DFL_CHUNK, len, s_in, tid);
    const u32 *m = (const u32 *)(meta + chunk * (u64)DFL_META);
    for (int i = tid; i < DFL_META / 4; i += NT) s_len32[i] = m[i];
    for (u32 i = (u32)tid; i < ((u32)shift + nbytes + 15u) >> 4; i += NT) s_out[i] = make_uint4(0, 0, 0, 0);
    if (tid < 16) s_count[tid] = 0;
    __syncthreads();
    const u8 *B = (const u8 *)s_in + shift_in;
    if (s_len[H::LIT_SYMS]) {  // stored: 00 (not final, BTYPE 00, padding), LEN, NLEN, the bytes
        if (tid == 0) {
            O[0] = 0;
            O[1] = (u8)len;
            O[2] = (u8)(len >> 8);
            O[3] = (u8)~len;
            O[4] = (u8)(~len >> 8);
        }
        for (u32 p = (u32)tid; p < len; p += NT) O[DFL_STORED + p] = B[p];
        __syncthreads();
        flush_image(dst, nbytes, s_out, shift, tid);
        return;
    }
    for (int s = tid; s < H::LIT_SYMS; s += NT)
        if (s_len[s]) atomicAdd(&s_count[s_len[s]], 1u);
    __syncthreads();
    if (tid == 0) {  // the block header, from the image's bit 8 * shift on
        H::BitWriter w = {(u8 *)s_out, 8ull * (u64)shift};
        H::block_header(s_len, &s_hs, &w);
        s_hdr_end = (u32)w.pos;
    }
    if (tid == 64) {  // the first code of every length (RFC 1951 3.2.2)
        u32 code = 0;
        s_first[0] = 0;
        for (int b = 1; b < 16; b++) {
            code = (code + (b > 1 ? s_count[b - 1] : 0u)) << 1;
            s_first[b] = code;
        }
    }
    __syncthreads();
    for (int s = tid; s < H::LIT_SYMS; s += NT) {
        const u32 l = s_len[s];
        u32 before = 0;  // symbols in front with the same length
        for (int q = 0; q < s; q++) before += s_len[q] == l ? 1u : 0u;
        s_code[s] = l ? (H::bit_reverse(s_first[l] + before, (int)l) | (l << 16)) : 0u;
    }
    __syncthreads();
    const u32 lo = (u32)tid * DFL_VT, hi = lo + DFL_VT < len ? lo + DFL_VT : len;
    u32 bits = 0;
    for (u32 p = lo; p < hi; p++) bits += s_code[B[p]] >> 16;
    u32 literal_bits;
    const u32 at = block_excl_scan_u32<NT>(bits, s_scan, &literal_bits);
    u32 *img = (u32 *)s_out;
    if (lo < hi) {
        const u32 pos = s_hdr_end + at;
        u32 w = pos >> 5, nb = pos & 31u;
        u64 acc = 0;
        for (u32 p = lo; p < hi; p++) {
            const u32 c = s_code[B[p]];
            acc |= (u64)(c & 0xFFFFu) << nb;
            nb += c >> 16;
            if (nb >= 32u) {
                atomicOr(&img[w++], (u32)acc);
                acc >>= 32;
                nb -= 32u;
            }
        }
        if (nb) atomicOr(&img[w], (u32)acc);
    }
    if (tid == 0) {  // end-of-block; the empty stored block's 3 header bits and its padding are zeros; LEN = 0, NLEN = FFFF
        const u32 c = s_code[H::EOB];
        const u32 pos = s_hdr_end + literal_bits;
        or_bits(img, pos, c & 0xFFFFu, c >> 16);
        const u32 byte = (pos + (c >> 16) + 3u + 7u) >> 3;
        or_bits(img, (byte + 2u) * 8u, 0xFFFFu, 16u);
    }
    __syncthreads();
    flush_image(dst, nbytes, s_out, shift, tid);
}

struct Edges {  // the bytes in front of and behind the chunks' blocks
    u8 head[10], tail[10];
    int nhead, ntail;
};
__global__ void dfl_edges_kernel(Edges e, u8 *head_at, u8 *tail_at) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int i = 0; i < e.nhead; i++) head_at[i] = e.head[i];
    for (int i = 0; i < e.ntail; i++) tail_at[i] = e.tail[i];
}

u64 edge_bytes(uint32_t flags, bool head) {
    const bool gz = flags & UKM_DEFLATE_GZIP, fin = gz || (flags & UKM_DEFLATE_FINAL);
    return head ? (gz ? 10u : 0u) : (fin ? 2u : 0u) + (gz ? 8u : 0u);
}

}  // namespace

extern "C" uint64_t ukm_deflate_bound(uint64_t n_bytes, uint32_t flags) {
    const u64 nchunks = n_bytes / DFL_CHUNK + (n_bytes % DFL_CHUNK ? 1 : 0);
    return n_bytes + (u64)DFL_STORED * nchunks + edge_bytes(flags, true) + edge_bytes(flags, false);
}

extern "C" uint32_t ukm_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return H::crc_combine(crc_a, crc_b, len_b); }

extern "C" int ukm_deflate(ukm_ctx *ctx, const uint8_t *src, uint64_t n_bytes, uint32_t flags, uint8_t *out, uint64_t out_cap,
                           uint64_t *n_out, uint32_t *crc32) {
    const char *name = "ukm_deflate";
    if (!ctx || !n_out || !crc32 || (!src && n_bytes) || (!out && out_cap)) UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
    *n_out = 0;
    if (flags & ~(UKM_DEFLATE_FINAL | UKM_DEFLATE_GZIP)) UKM_FAIL(UKM_ERR_INVALID, "%s: unknown flags %#x", name, flags);
    const bool gz = flags & UKM_DEFLATE_GZIP;
    if (gz && *crc32) UKM_FAIL(UKM_ERR_INVALID, "%s: a gzip member starts with *crc32 = 0: nothing precedes its bytes", name);
    const u64 nhead = edge_bytes(flags, true), ntail = edge_bytes(flags, false);
    if (n_bytes == 0 && nhead + ntail == 0) return UKM_OK;
    const u64 nchunks = n_bytes / DFL_CHUNK + (n_bytes % DFL_CHUNK ? 1 : 0);
    if (nchunks > MAX_GRID) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu bytes in one call", name, (unsigned long long)n_bytes);
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        const u8 *b = nullptr;
        u8 *ob = nullptr, *meta = nullptr;
        u32 *crcs = nullptr;
        SizeScan z;  // of the chunks: z.total stays 0 without one
        if (nchunks) {
            UKM_TRY(ukm_in_t(ctx, src, n_bytes, &b));
            UKM_TRY(size_alloc(ctx, nchunks, -1, &z));
            UKM_TRY(ws_alloc_t(ctx, nchunks, &crcs));
            UKM_TRY(ws_alloc_t(ctx, nchunks * DFL_META, &meta));
            hipLaunchKernelGGL(dfl_sum_kernel, dim3((unsigned)nchunks), dim3(NT), 0, ctx->stream, b, n_bytes, z.sums, meta, crcs);
            UKM_TRY(size_scan(ctx, nchunks, &z));
        }
        const u64 body = z.total, need = nhead + body + ntail;
        UKM_TRY(out_fits(name, "the fragment takes", "bytes", need, out_cap, n_out));
        u32 crc = *crc32;
        if (nchunks) {  // the register after every chunk: times x^(8 * the chunk's bytes), plus the chunk's raw CRC
            std::vector<u32> raw(nchunks);
            UKM_HIP(hipMemcpyAsync(raw.data(), crcs, nchunks * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
            UKM_HIP(hipStreamSynchronize(ctx->stream));
            const u32 full = H::crc_x8n(DFL_CHUNK);
            u32 reg = crc ^ 0xFFFFFFFFu;
            for (u64 i = 0; i + 1 < nchunks; i++) reg = H::crc_mul(reg, full) ^ raw[i];
            reg = H::crc_mul(reg, H::crc_x8n(n_bytes - (nchunks - 1) * (u64)DFL_CHUNK)) ^ raw[nchunks - 1];
            crc = reg ^ 0xFFFFFFFFu;
        }
        UKM_TRY(ukm_out_t(ctx, out, need, &ob));
        if (nchunks) {
            write_begins(ctx);
            hipLaunchKernelGGL(dfl_write_kernel, dim3((unsigned)nchunks), dim3(NT), 0, ctx->stream, b, n_bytes, (const u8 *)meta,
                               (const u64 *)z.offs, (const u32 *)z.sums, ob + nhead);
        }
        if (nhead + ntail) {
            Edges e;
            memset(&e, 0, sizeof e);
            e.nhead = (int)nhead;
            e.ntail = (int)ntail;
            if (gz) {  // RFC 1952: ID1 ID2, CM = 8, no flags, no time, XFL = 0, OS = 255 (unknown)
                const u8 h[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255};
                memcpy(e.head, h, 10);
            }
            e.tail[0] = 3;  // the final block: BFINAL = 1, BTYPE = 01, end-of-block (7 zero bits)
            e.tail[1] = 0;
            if (gz)
                for (int i = 0; i < 4; i++) {
                    e.tail[2 + i] = (u8)(crc >> (8 * i));
                    e.tail[6 + i] = (u8)(n_bytes >> (8 * i));  // ISIZE: the length mod 2^32
                }
            hipLaunchKernelGGL(dfl_edges_kernel, dim3(1), dim3(64), 0, ctx->stream, e, ob, ob + nhead + body);
        }
        UKM_HIP(hipGetLastError());
        *crc32 = crc;
        return UKM_OK;
    }();
    return ukm_finish(&s, rc);
}
