// ukm_bytes.h — what the kernels that read or write unaligned byte streams share (ukm_unik.hip: .unik bodies, ukm_text.hip:
// k-mer text, ukm_deflate.hip and ukm_inflate.hip: deflate blocks): a range of bytes to and from an LDS image as aligned 16-byte words,
// big-endian fields, and the size-then-write protocol of the calls whose output size is known only after a pass over the
// input (below: SizeScan).  Workgroups of NT threads; the block scan is ukm_device.h's block_excl_scan_u32<NT>, the
// library's one.  Everything has internal linkage: each source that includes this gets kernels of its own.
#pragma once
#include "ukm_device.h"

namespace {

constexpr int NT = 256;
constexpr int SCAN_LDS = NT / 64 + 1;  // LDS words block_excl_scan_u32<NT> takes

// body[start, start + len), len > 0, into the LDS image: byte i of the range lands at image byte shift + i, shift = the
// range's address mod 16 (returned).  Every word loaded is an aligned 16-byte word that overlaps the range.
__device__ inline int load_image(const u8 *body, u64 start, u32 len, uint4 *img, int tid) {
    const uintptr_t a = (uintptr_t)(body + start);
    const int shift = (int)(a & 15);
    const uint4 *w0 = (const uint4 *)(a - (uintptr_t)shift);
    const u32 nwords = ((u32)shift + len + 15u) >> 4;
    for (u32 i = (u32)tid; i < nwords; i += NT) img[i] = w0[i];
    return shift;
}

// image bytes [shift, shift + len) to dst[0, len), shift = dst mod 16: whole aligned words inside, single bytes at the ends
__device__ inline void flush_image(u8 *dst, u32 len, const uint4 *img, int shift, int tid) {
    u8 *w0 = dst - shift;
    const u32 lo = (u32)shift, hi = (u32)shift + len;
    const u32 nwords = (hi + 15u) >> 4;
    const u8 *bytes = (const u8 *)img;
    for (u32 i = (u32)tid; i < nwords; i += NT) {
        const u32 b0 = i * 16u, b1 = b0 + 16u;
        if (b0 >= lo && b1 <= hi) {
            ((uint4 *)w0)[i] = img[i];
        } else {
            for (u32 b = b0 > lo ? b0 : lo; b < (b1 < hi ? b1 : hi); b++) w0[b] = bytes[b];
        }
    }
}

// the output image of a tile that lands at dst: B = the returned pointer has B[i] = dst[i]; *shift is what flush_image takes
__device__ inline u8 *image_at(const u8 *dst, uint4 *img, int *shift) {
    *shift = (int)((uintptr_t)dst & 15);
    return (u8 *)img + *shift;
}

__device__ inline u64 get_be(const u8 *p, int n) {
    u64 v = 0;
    for (int i = 0; i < n; i++) v = (v << 8) | p[i];
    return v;
}
__device__ inline void put_be(u8 *p, u64 v, int n) {
    for (int i = n - 1; i >= 0; i--) {
        p[i] = (u8)v;
        v >>= 8;
    }
}
__device__ inline int byte_len(u64 v) { return v ? (64 - __clzll((long long)v) + 7) >> 3 : 1; }

// one workgroup: offs[i] = the sum of sums[0 .. i), ctl[0] = the sum of all
__global__ __launch_bounds__(NT) void scan_sums_kernel(const u32 *sums, u64 ntiles, u64 *offs, u64 *ctl) {
    __shared__ u32 s_scan[SCAN_LDS];
    const int tid = (int)threadIdx.x;
    u64 carry = 0;
    for (u64 i0 = 0; i0 < ntiles; i0 += NT) {
        const u64 i = i0 + (u64)tid;
        const u32 v = i < ntiles ? sums[i] : 0u;
        u32 total;
        const u32 excl = block_excl_scan_u32<NT>(v, s_scan, &total);
        if (i < ntiles) offs[i] = carry + excl;
        carry += total;
    }
    if (tid == 0) ctl[0] = carry;
}

constexpr u64 MAX_GRID = 0x7fffffffull;

// ---- the size-then-write protocol ------------------------------------------------------------------------------------------
// A call whose output size depends on the data runs two passes over tiles of its input:
//   1. a size kernel leaves every tile's output size in sums[tile] (and may raise the flag word),
//   2. size_scan: scan_sums_kernel, one workgroup, turns them into offs[tile] and the total, which is read back -- with the
//      flag word where the call named a fill byte for it, and only there.  Such a call decides its own errors from the flag,
//      then out_fits sets *n_out and ends a size query or a capacity failure,
//   3. write_begins, then a write kernel that puts tile t's bytes (or records) at offs[t].
// ukm_last_kernel_ms of such a call is step 2: the scan between the two passes, its read-back(s) included.
struct SizeScan {
    u32 *sums = nullptr;  // [ntiles]
    u64 *offs = nullptr;  // [ntiles]
    u64 *ctl = nullptr;   // [0] the total, written by the scan; [1] the call's flag word, written by the size kernel
    u64 total = 0, flag = 0;  // ctl as size_scan read it back (flag: stays 0, unread, in a call that has none)
    bool flagged = false;
};
// flag_fill: the byte ctl[1] is filled with in front of the size kernel (0xFF for an atomicMin, 0 for an atomicOr); -1: the
// call has no flag word, and the word is neither filled nor read
inline int size_alloc(ukm_ctx *ctx, u64 ntiles, int flag_fill, SizeScan *z) {
    UKM_TRY(ws_alloc_t(ctx, ntiles, &z->sums));
    UKM_TRY(ws_alloc_t(ctx, ntiles, &z->offs));
    UKM_TRY(ws_alloc_t(ctx, 2, &z->ctl));
    z->flagged = flag_fill >= 0;
    if (z->flagged) UKM_HIP(hipMemsetAsync(z->ctl + 1, flag_fill, sizeof(u64), ctx->stream));
    return UKM_OK;
}
// behind the first pass of a call (the size kernel; the sorted decode's summaries): what ukm_last_kernel_ms times begins
inline void scan_begins(ukm_ctx *ctx) { (void)hipEventRecord(ctx->ev_k0, ctx->stream); }
// ... and ends, in front of the write pass
inline void write_begins(ukm_ctx *ctx) {
    (void)hipEventRecord(ctx->ev_k1, ctx->stream);
    ctx->evk_valid = true;
}
inline int size_scan(ukm_ctx *ctx, u64 ntiles, SizeScan *z) {
    scan_begins(ctx);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(NT), 0, ctx->stream, (const u32 *)z->sums, ntiles, z->offs, z->ctl);
    UKM_HIP(hipGetLastError());
    u64 res[2] = {0, 0};
    UKM_TRY(ukm_read_u64(ctx, z->ctl, res, z->flagged ? 2 : 1));
    z->total = res[0];
    z->flag = res[1];
    return UKM_OK;
}
// *n_out = need, and UKM_ERR_CAPACITY where the caller's arrays are smaller: "<name>: <what> <need> <unit>, out_cap is ..."
inline int out_fits(const char *name, const char *what, const char *unit, u64 need, u64 out_cap, u64 *n_out) {
    *n_out = need;
    if (out_cap < need) UKM_FAIL(UKM_ERR_CAPACITY, "%s: %s %llu %s, out_cap is %llu", name, what, (unsigned long long)need, unit,
                                 (unsigned long long)out_cap);
    return UKM_OK;
}

}  // namespace
