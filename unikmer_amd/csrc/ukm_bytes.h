// ukm_bytes.h — the byte-image machinery of the kernels that read or write unaligned byte streams (ukm_unik.hip: .unik bodies,
// ukm_text.hip: k-mer text): a range of bytes to and from an LDS image as aligned 16-byte words, big-endian fields, and the
// reduce-then-scan of per-tile sizes.  Workgroups of NT threads.  Everything has internal linkage: each source that
// includes this gets kernels of its own.
#pragma once
#include "ukm_internal.h"

namespace {

constexpr int NT = 256;

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

// exclusive scan of one u32 per thread; *total = the workgroup's sum.  s: NT words.
__device__ inline u32 block_excl_scan(u32 v, u32 *s, int tid, u32 *total) {
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        const u32 add = tid >= d ? s[tid - d] : 0u;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    const u32 incl = s[tid];
    *total = s[NT - 1];
    __syncthreads();
    return incl - v;
}

// one workgroup: offs[i] = the sum of sums[0 .. i), ctl[0] = the sum of all
__global__ __launch_bounds__(NT) void scan_sums_kernel(const u32 *sums, u64 ntiles, u64 *offs, u64 *ctl) {
    __shared__ u32 s_scan[NT];
    const int tid = (int)threadIdx.x;
    u64 carry = 0;
    for (u64 i0 = 0; i0 < ntiles; i0 += NT) {
        const u64 i = i0 + (u64)tid;
        const u32 v = i < ntiles ? sums[i] : 0u;
        u32 total;
        const u32 excl = block_excl_scan(v, s_scan, tid, &total);
        if (i < ntiles) offs[i] = carry + excl;
        carry += total;
    }
    if (tid == 0) ctl[0] = carry;
}

constexpr u64 MAX_GRID = 0x7fffffffull;

}  // namespace
