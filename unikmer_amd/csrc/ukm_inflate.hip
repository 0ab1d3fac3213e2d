// ukm_inflate.hip — ukm_inflate: the longest prefix of a raw RFC 1951 fragment that is non-final blocks of literals (what
// ukm_deflate writes, and what zlib writes under Z_HUFFMAN_ONLY with a flush per chunk) back to bytes, in parallel.
//
// Such a stream returns to a byte boundary behind every empty stored block: the marker 00 00 FF FF.  The marker is searched
// for, and a hit is never trusted on its own: segment ends are CHAINED from offset 0, and only segments on the chain count.
// A hit inside Huffman bits or inside a stored payload starts a segment that parses or not, and is never looked at.
//   1. inf_cand_kernel, twice (count, scan, write): every offset behind a marker, and offset 0, ascending.
//   2. inf_size_kernel, a LANE per candidate (its tables in LDS: canonical decode, a 9-bit lookup in front of it): walk_segment (ukm_inflate.h) parses blocks to the segment's end or to the
//      first block the device does not take, and leaves the end, the output size and the number of checkpoints.
//   3. the chain, on the host: from candidate 0, end -> candidate by binary search, to the first segment that stopped early
//      (its byte-aligned prefix still counts).  The protocol's scan (ukm_bytes.h: SizeScan) over the chain's sizes; the
//      size query and a capacity failure end here.
//   4. inf_cp_kernel, a lane per chain segment: the same walk, now leaving a checkpoint every CP_BYTES output bytes (the
//      chain's counts say where: the size pass cannot, a candidate off the chain would need room that nobody can bound).
//   5. inf_write_kernel, a workgroup per INF_GROUP checkpoints -- a tile of the OUTPUT, whatever segment it came from: the
//      tables of the blocks the tile touches, one per block, built by the first lane that sits in it; a lane per checkpoint
//      decodes into an LDS image that starts at the output's address mod 16; pieces of stored blocks are cooperative
//      copies; the tile's raw CRC-32 from per-thread slices; flush_image writes whole aligned words.
// The tiles' CRCs are folded on the host, as ukm_deflate folds its chunks'.
#include <algorithm>
#include <vector>

#include "ukm_bytes.h"
#include "ukm_huff.h"
#include "ukm_inflate.h"

namespace {

namespace H = ukm_huff;
namespace I = ukm_puff;

constexpr int INF_CAND_TILE = 16384;  // source bytes per workgroup of the candidate search
constexpr int INF_CAND_VT = INF_CAND_TILE / NT;
constexpr int INF_HALO = 3;                          // bytes of the next tile a marker that begins in this one reaches into
constexpr int INF_CAND_IMG = INF_CAND_TILE + 32;     // the halo and up to 15 bytes of alignment shift, rounded to 16
constexpr int INF_LANES = 16;                        // segments per workgroup of the two walks: tables per lane in LDS, and a
                                                     // quarter wave: a chunk is 32 K serial symbols, few lanes diverge less and
                                                     // 16 500 segments per GB of body still reach every SIMD
constexpr int INF_GROUP = 32;                        // checkpoints per workgroup of the write pass
constexpr int INF_TILE = INF_GROUP * (int)I::CP_BYTES;  // output bytes of such a workgroup at most
constexpr int INF_OUT_IMG = INF_TILE + 16;
constexpr int INF_VT = INF_TILE / NT;
static_assert(INF_CAND_VT * NT == INF_CAND_TILE && INF_CAND_IMG % 16 == 0 && INF_CAND_TILE + INF_HALO + 15 <= INF_CAND_IMG, "candidate tile");
static_assert(INF_OUT_IMG % 16 == 0 && INF_VT * NT == INF_TILE && INF_TILE < 65536, "output tile: crc_slice takes 16 bits of length");
static_assert(INF_GROUP * I::LENS <= INF_TILE, "the header scratch of every leader fits the output image");
static_assert(INF_GROUP <= 64 && NT == 256, "one wave decodes; 256 threads fill the CRC table");

// WRITE false: sums[tile] = the candidates of the tile; true: they go to cand[offs[tile] ...], ascending
template <bool WRITE>
__global__ __launch_bounds__(NT) void inf_cand_kernel(const u8 *src, u64 n_bytes, u32 *sums, const u64 *offs, u64 *cand) {
    __shared__ uint4 s_img[INF_CAND_IMG / 16];
    __shared__ u32 s_scan[SCAN_LDS];
    const int tid = (int)threadIdx.x;
    const u64 tile = blockIdx.x, t0 = tile * (u64)INF_CAND_TILE;
    const u64 rest = n_bytes - t0;
    const u32 len = (u32)(rest < (u64)(INF_CAND_TILE + INF_HALO) ? rest : (u64)(INF_CAND_TILE + INF_HALO));
    const int shift = load_image(src, t0, len, s_img, tid);
    __syncthreads();
    const u8 *B = (const u8 *)s_img + shift;
    u32 npos = len > (u32)INF_HALO ? len - (u32)INF_HALO : 0u;  // offsets at which four bytes are inside the source
    if (npos > (u32)INF_CAND_TILE) npos = (u32)INF_CAND_TILE;
    const u32 lo = (u32)tid * INF_CAND_VT, hi = lo + INF_CAND_VT < npos ? lo + INF_CAND_VT : npos;
    const bool zero = tile == 0 && tid == 0;  // offset 0 always is a candidate
    u32 mine = zero ? 1u : 0u;
    for (u32 p = lo; p < hi; p++) mine += (B[p] == 0 && B[p + 1] == 0 && B[p + 2] == 0xFF && B[p + 3] == 0xFF) ? 1u : 0u;
    u32 total;
    const u32 at = block_excl_scan_u32<NT>(mine, s_scan, &total);
    if (!WRITE) {
        if (tid == 0) sums[tile] = total;
        return;
    }
    u64 k = offs[tile] + at;
    if (zero) cand[k++] = 0;
    for (u32 p = lo; p < hi; p++)
        if (B[p] == 0 && B[p + 1] == 0 && B[p + 2] == 0xFF && B[p + 3] == 0xFF) cand[k++] = t0 + p + 4;
}

struct WalkLds {
    I::Table table[INF_LANES];
    u8 lens[INF_LANES][I::LENS];
    uint16_t lut[INF_LANES][I::LUT_SIZE];
};

constexpr u32 SEG_EARLY = 1u << 31;  // in seg_out: the segment stopped in front of a block it does not take

__global__ __launch_bounds__(INF_LANES) void inf_size_kernel(const u8 *src, u64 n_bytes, const u64 *cand, u64 ncand, u64 *seg_end,
                                                             u32 *seg_out, u32 *seg_ncp) {
    __shared__ WalkLds s;
    const int tid = (int)threadIdx.x;
    const u64 i = (u64)blockIdx.x * INF_LANES + (u64)tid;
    if (i >= ncand) return;
    const I::SegResult r = I::walk_segment(src, n_bytes, cand[i], ~0ull, &s.table[tid], s.lens[tid], s.lut[tid], [](u64, u64, u64, u32) {});
    seg_end[i] = r.end;
    seg_out[i] = (u32)r.out | (r.early ? SEG_EARLY : 0u);  // r.out < SEG_LIMIT = 2^31
    seg_ncp[i] = (u32)r.ncp;                               // at most one per output byte
}

// chain segment s: src[start[s], end[s]) gives out[offs[s], offs[s] + sums[s]) and the checkpoints cp_at[s] .. cp_at[s + 1]
__global__ __launch_bounds__(INF_LANES) void inf_cp_kernel(const u8 *src, u64 n_bytes, const u64 *start, const u64 *end, const u64 *cp_at,
                                                           const u64 *offs, u64 nseg, I::Checkpoint *cps) {
    __shared__ WalkLds s;
    const int tid = (int)threadIdx.x;
    const u64 i = (u64)blockIdx.x * INF_LANES + (u64)tid;
    if (i >= nseg) return;
    const u64 base = offs[i], k0 = cp_at[i], kn = cp_at[i + 1] - k0;
    u64 k = 0;
    (void)I::walk_segment(src, n_bytes, start[i], end[i], &s.table[tid], s.lens[tid], s.lut[tid], [&](u64 bit, u64 hdr, u64 out, u32 n) {
        if (k < kn) {
            I::Checkpoint c = {bit, hdr, base + out, n, 0u};
            cps[k0 + k] = c;
        }
        k++;
    });
}

__global__ __launch_bounds__(NT) void inf_write_kernel(const u8 *src, u64 n_bytes, const I::Checkpoint *cps, u64 ncp, u8 *out, u64 n_out,
                                                       u32 *crcs, u32 *lens_out) {
    __shared__ uint4 s_img[INF_OUT_IMG / 16];
    __shared__ I::Table s_table[INF_GROUP];
    __shared__ I::Checkpoint s_cp[INF_GROUP];
    __shared__ u32 s_ok[INF_GROUP];
    __shared__ u32 s_tab[256], s_pow[16];
    __shared__ u32 s_crc;
    const int tid = (int)threadIdx.x;
    const u64 k0 = (u64)blockIdx.x * INF_GROUP;
    const int cnt = (int)(ncp - k0 < (u64)INF_GROUP ? ncp - k0 : (u64)INF_GROUP);
    if (tid < cnt) s_cp[tid] = cps[k0 + (u64)tid];
    if (tid < INF_GROUP) s_ok[tid] = 0;
    H::crc_lds_tables(s_tab, s_pow, tid);
    if (tid == 0) s_crc = 0;
    __syncthreads();
    const u64 base = s_cp[0].out;
    u64 span = s_cp[cnt - 1].out + s_cp[cnt - 1].n - base;  // consecutive checkpoints are consecutive output
    if (base > n_out || span > n_out - base) span = 0;      // (never: the checkpoints tile out[0, n_out))
    const u32 total = (u32)(span < (u64)INF_TILE ? span : (u64)INF_TILE);
    u8 *dst = out + base;
    int shift;
    u8 *O = image_at(dst, s_img, &shift);
    const bool huff = tid < cnt && s_cp[tid].hdr != I::STORED_CP;
    // a table per block: the first lane that sits in a block builds it; the image is its scratch until the barrier
    if (huff && (tid == 0 || s_cp[tid - 1].hdr != s_cp[tid].hdr)) {
        I::BitReader br;
        br.src = src;
        br.n_bytes = n_bytes;
        br.seek(s_cp[tid].hdr);
        u32 h;
        if (br.take(3, &h) && (h == 2u || h == 4u)) s_ok[tid] = I::build_table(&br, (int)(h >> 1), &s_table[tid], (u8 *)s_img + tid * I::LENS) ? 1u : 0u;
    }
    __syncthreads();
    if (huff) {
        int slot = tid;
        while (slot > 0 && s_cp[slot - 1].hdr == s_cp[tid].hdr) slot--;
        const u64 rel = s_cp[tid].out - base;
        const u32 n = s_cp[tid].n;
        if (s_ok[slot] && rel + n <= (u64)total) {
            I::BitReader br;
            br.src = src;
            br.n_bytes = n_bytes;
            br.seek(s_cp[tid].bit);
            for (u32 i = 0; i < n; i++) {
                const int sym = I::decode_symbol(&br, &s_table[slot]);
                if (sym < 0 || sym > 255) break;
                O[rel + i] = (u8)sym;
            }
        }
    }
    for (int j = 0; j < cnt; j++) {
        if (s_cp[j].hdr != I::STORED_CP) continue;
        const u64 from = s_cp[j].bit >> 3, rel = s_cp[j].out - base;
        const u32 n = s_cp[j].n;
        if (from + n > n_bytes || rel + n > (u64)total) continue;
        for (u32 i = (u32)tid; i < n; i += NT) O[rel + i] = src[from + i];
    }
    __syncthreads();
    const u32 lo = (u32)tid * INF_VT, hi = lo + INF_VT < total ? lo + INF_VT : total;
    if (lo < total) atomicXor(&s_crc, H::crc_slice(O, lo, hi, total, s_tab, s_pow));
    __syncthreads();
    if (tid == 0) {
        crcs[blockIdx.x] = s_crc;
        lens_out[blockIdx.x] = total;
    }
    flush_image(dst, total, s_img, shift, tid);
}

template <typename T>
int to_host(ukm_ctx *ctx, const T *dev, u64 n, std::vector<T> *v) {
    v->resize(n);
    if (n) UKM_HIP(hipMemcpyAsync(v->data(), dev, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return UKM_OK;
}
template <typename T>
int to_device(ukm_ctx *ctx, const std::vector<T> &v, T **dev) {
    UKM_TRY(ws_alloc_t(ctx, v.size(), dev));
    UKM_HIP(hipMemcpyAsync(*dev, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return UKM_OK;
}

}  // namespace

extern "C" uint64_t ukm_inflate_bound(uint64_t n_bytes) { return n_bytes > ~0ull / 8 ? ~0ull : 8 * n_bytes; }

extern "C" int ukm_inflate(ukm_ctx *ctx, const uint8_t *src, uint64_t n_bytes, uint32_t flags, uint8_t *out, uint64_t out_cap,
                           uint64_t *n_out, uint64_t *n_consumed, uint32_t *crc32) {
    const char *name = "ukm_inflate";
    if (!ctx || !n_out || !n_consumed || !crc32 || (!src && n_bytes) || (!out && out_cap)) UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
    *n_out = 0;
    *n_consumed = 0;
    if (flags) UKM_FAIL(UKM_ERR_INVALID, "%s: unknown flags %#x", name, flags);
    if (n_bytes == 0) return UKM_OK;
    const u64 ntiles = n_bytes / INF_CAND_TILE + (n_bytes % INF_CAND_TILE ? 1 : 0);
    if (ntiles > MAX_GRID) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu bytes in one call", name, (unsigned long long)n_bytes);
    // what asynchronous copies read and write on the host lives out here: the stream is drained before any of it goes away
    std::vector<u64> h_cand, h_end, c_start, c_end, c_cp(1, 0);
    std::vector<u32> h_out, h_ncp, c_size, raw, len;
    hipEvent_t ev_cp0 = nullptr, ev_cp1 = nullptr;  // around the second walk: statistic "inflate_cp_walk_us"
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        const u8 *b = nullptr;
        UKM_TRY(ukm_in_t(ctx, src, n_bytes, &b));
        // 1. candidates
        SizeScan zc;
        UKM_TRY(size_alloc(ctx, ntiles, -1, &zc));
        hipLaunchKernelGGL(inf_cand_kernel<false>, dim3((unsigned)ntiles), dim3(NT), 0, ctx->stream, b, n_bytes, zc.sums, (const u64 *)nullptr,
                           (u64 *)nullptr);
        UKM_TRY(size_scan(ctx, ntiles, &zc));
        const u64 ncand = zc.total;
        u64 *cand = nullptr, *seg_end = nullptr;
        u32 *seg_out = nullptr, *seg_ncp = nullptr;
        UKM_TRY(ws_alloc_t(ctx, ncand, &cand));
        UKM_TRY(ws_alloc_t(ctx, ncand, &seg_end));
        UKM_TRY(ws_alloc_t(ctx, ncand, &seg_out));
        UKM_TRY(ws_alloc_t(ctx, ncand, &seg_ncp));
        hipLaunchKernelGGL(inf_cand_kernel<true>, dim3((unsigned)ntiles), dim3(NT), 0, ctx->stream, b, n_bytes, (u32 *)nullptr,
                           (const u64 *)zc.offs, cand);
        // 2. every candidate's segment
        const u64 ngrid = (ncand + INF_LANES - 1) / INF_LANES;
        if (ngrid > MAX_GRID) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu candidates in one call", name, (unsigned long long)ncand);
        hipLaunchKernelGGL(inf_size_kernel, dim3((unsigned)ngrid), dim3(INF_LANES), 0, ctx->stream, b, n_bytes, (const u64 *)cand, ncand, seg_end,
                           seg_out, seg_ncp);
        UKM_HIP(hipGetLastError());
        UKM_TRY(to_host(ctx, cand, ncand, &h_cand));
        UKM_TRY(to_host(ctx, seg_end, ncand, &h_end));
        UKM_TRY(to_host(ctx, seg_out, ncand, &h_out));
        UKM_TRY(to_host(ctx, seg_ncp, ncand, &h_ncp));
        UKM_HIP(hipStreamSynchronize(ctx->stream));
        // 3. the chain.  scan_sums_kernel adds NT sizes at a time in 32 bits: the chain also ends in front of the segment
        // that would take such a group to 2^32 (segments of 16 MiB and more: long runs of stored chunks)
        u64 consumed = 0, group = 0;
        for (u64 i = 0; ncand && h_cand[0] == 0;) {
            const bool early = h_out[i] & SEG_EARLY;
            const u32 size = h_out[i] & ~SEG_EARLY;
            const u64 end = h_end[i];
            if (end <= h_cand[i] || end > n_bytes) break;  // an early stop at its own start: nothing of it counts
            if (c_size.size() % NT == 0) group = 0;
            if (group + size > 0xFFFFFFFFull) break;
            group += size;
            c_start.push_back(h_cand[i]);
            c_end.push_back(end);
            c_size.push_back(size);
            c_cp.push_back(c_cp.back() + h_ncp[i]);
            consumed = end;
            if (early) break;
            const auto it = std::lower_bound(h_cand.begin() + (std::ptrdiff_t)i + 1, h_cand.end(), end);
            if (it == h_cand.end() || *it != end) break;
            i = (u64)(it - h_cand.begin());
        }
        const u64 nseg = c_size.size(), ncp = c_cp.back();
        *n_consumed = consumed;
        ctx->stat_inflate_candidates = ncand;
        ctx->stat_inflate_segments = nseg;
        ctx->stat_inflate_cp_walk_us = 0;
        if (nseg == 0) return UKM_OK;
        SizeScan z;
        UKM_TRY(size_alloc(ctx, nseg, -1, &z));
        UKM_HIP(hipMemcpyAsync(z.sums, c_size.data(), nseg * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
        UKM_TRY(size_scan(ctx, nseg, &z));
        UKM_TRY(out_fits(name, "the prefix inflates to", "bytes", z.total, out_cap, n_out));
        if (ncp == 0) return UKM_OK;  // empty blocks only
        u8 *ob = nullptr;
        UKM_TRY(ukm_out_t(ctx, out, z.total, &ob));
        // 4. and 5.: the write side
        u64 *d_start = nullptr, *d_end = nullptr, *d_cp = nullptr;
        I::Checkpoint *cps = nullptr;
        u32 *crcs = nullptr, *lens = nullptr;
        const u64 ngroups = (ncp + INF_GROUP - 1) / INF_GROUP;
        if (ngroups > MAX_GRID) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu output bytes in one call", name, (unsigned long long)z.total);
        UKM_TRY(to_device(ctx, c_start, &d_start));
        UKM_TRY(to_device(ctx, c_end, &d_end));
        UKM_TRY(to_device(ctx, c_cp, &d_cp));
        UKM_TRY(ws_alloc_t(ctx, ncp, &cps));
        UKM_TRY(ws_alloc_t(ctx, ngroups, &crcs));
        UKM_TRY(ws_alloc_t(ctx, ngroups, &lens));
        UKM_HIP(hipEventCreate(&ev_cp0));
        UKM_HIP(hipEventCreate(&ev_cp1));
        write_begins(ctx);
        (void)hipEventRecord(ev_cp0, ctx->stream);
        // (nseg <= ncand: the grid was checked above)
        hipLaunchKernelGGL(inf_cp_kernel, dim3((unsigned)((nseg + INF_LANES - 1) / INF_LANES)), dim3(INF_LANES), 0, ctx->stream, b, n_bytes,
                           (const u64 *)d_start, (const u64 *)d_end, (const u64 *)d_cp, (const u64 *)z.offs, nseg, cps);
        (void)hipEventRecord(ev_cp1, ctx->stream);
        hipLaunchKernelGGL(inf_write_kernel, dim3((unsigned)ngroups), dim3(NT), 0, ctx->stream, b, n_bytes, (const I::Checkpoint *)cps, ncp, ob,
                           z.total, crcs, lens);
        UKM_HIP(hipGetLastError());
        UKM_TRY(to_host(ctx, crcs, ngroups, &raw));
        UKM_TRY(to_host(ctx, lens, ngroups, &len));
        UKM_HIP(hipStreamSynchronize(ctx->stream));
        float cp_ms = 0;
        if (hipEventElapsedTime(&cp_ms, ev_cp0, ev_cp1) == hipSuccess) ctx->stat_inflate_cp_walk_us = (u64)(cp_ms * 1000.0f);
        // the register after every tile: times x^(8 * the tile's bytes), plus the tile's raw CRC
        u32 pw[16];
        pw[0] = H::CRC_X8;
        for (int k = 1; k < 16; k++) pw[k] = H::crc_mul(pw[k - 1], pw[k - 1]);
        const u32 full = H::crc_x8n(INF_TILE);
        u32 reg = *crc32 ^ 0xFFFFFFFFu;
        for (u64 g = 0; g < ngroups; g++) {
            if (len[g] == (u32)INF_TILE) {
                reg = H::crc_mul(reg, full);
            } else {
                for (int k = 0; k < 16; k++)
                    if ((len[g] >> k) & 1u) reg = H::crc_mul(reg, pw[k]);
            }
            reg ^= raw[g];
        }
        *crc32 = reg ^ 0xFFFFFFFFu;
        return UKM_OK;
    }();
    if (rc != UKM_OK) (void)hipStreamSynchronize(ctx->stream);  // a copy to or from the vectors above may still be pending
    if (ev_cp0) (void)hipEventDestroy(ev_cp0);
    if (ev_cp1) (void)hipEventDestroy(ev_cp1);
    return ukm_finish(&s, rc);
}
