// ukm_dir.h — "is this code in a sorted array": the prefix directory and the short search behind it, shared by the window
// join of ukm_map.hip and the membership predicate of ukm_select.hip.
//   dir[p] = lower bound of prefix p in the sorted array, 2^B + 1 words with B = log2(n) - 1: the bucket of a prefix holds
//   2-4 codes, one 128-byte line most of the time -- one directory read and one or two reads of the array per lookup
//   instead of the ~log2(n) dependent gathers of a whole binary search.
// Everything here is local to the including translation unit.
#pragma once

#include <algorithm>

#include "ukm_device.h"

namespace {

// first index in [lo, hi) with a[i] >= x
__device__ __forceinline__ u64 lower_bound_u64(const u64 *a, u64 lo, u64 hi, u64 x) {
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// prefix directory of a sorted array: dir[p] = lower bound of (p << shift), p = 0 .. nb; dir[nb] = n
struct Dir {
    const u64 *keys;
    const u32 *dir;
    u64 n;
    int shift;
    u32 nb;
};

__global__ void dir_build_kernel(const u64 *keys, u64 n, int shift, u32 nb, u32 *dir) {
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > (u64)nb) return;
    dir[p] = p == (u64)nb ? (u32)n : (u32)lower_bound_u64(keys, 0, n, p << shift);
}

__device__ __forceinline__ void dir_bucket(const Dir &d, u64 x, u32 &lo, u32 &len) {
    u64 b = x >> d.shift;
    if (b >= (u64)d.nb) b = (u64)d.nb - 1;  // (a value wider than the directory's key width: behind everything in the last bucket)
    lo = d.dir[b];
    len = d.dir[b + 1] - lo;
}
__device__ __forceinline__ u32 dir_lower_bound(const Dir &d, u64 x) {
    u32 lo, len;
    dir_bucket(d, x, lo, len);
    return (u32)lower_bound_u64(d.keys, lo, (u64)lo + len, x);
}

// N lookups of one thread side by side: every round has N independent loads in flight (a bucket is a few codes: 2-3
// rounds).  The lower bound ends on the last probe that was not below x, so whether it IS x is known without another
// read; a search that never saw such a probe ends on the first code of a later prefix, which cannot be x.
// Bit s of `valid` says that x[s] takes part; returns the hit mask, lo[s] = the lower bound of x[s].
template <int N>
__device__ __forceinline__ u32 dir_search_n(const Dir &d, const u64 (&x)[N], u32 valid, u32 (&lo)[N]) {
    u32 len[N];
#pragma unroll
    for (int s = 0; s < N; s++) {
        lo[s] = 0; len[s] = 0;
        if ((valid >> s) & 1u) dir_bucket(d, x[s], lo[s], len[s]);
    }
    u32 hit = 0;
    for (;;) {
        bool any = false;
#pragma unroll
        for (int s = 0; s < N; s++)
            if (len[s]) {
                any = true;
                const u32 half = len[s] >> 1;
                const u64 v = d.keys[lo[s] + half];
                if (v < x[s]) { lo[s] += half + 1; len[s] -= half + 1; }
                else {
                    len[s] = half;
                    hit = (hit & ~(1u << s)) | (v == x[s] ? 1u << s : 0u);
                }
            }
        if (!any) break;
    }
    return hit;
}

// the directory of keys[n] (sorted, n >= 1, fewer than 2^32) in the context's arena; slack = log2 of the codes per prefix
// (the caller's choice: ukm_map.hip reads its developer knob, ukm_select.hip takes the measured default of DESIGN.md 4.14)
constexpr int DIR_SLACK_DEFAULT = 1;
int build_dir(ukm_ctx *c, const u64 *keys, u64 n, int key_bits, int slack, Dir *d) {
    int lg = 0;
    while (lg < 63 && (2ull << lg) <= n) lg++;  // floor(log2(n))
    slack = std::max(0, std::min(8, slack));
    const int B = std::max(1, std::min(std::min(lg - slack, 24), key_bits));
    u32 *dir = nullptr;
    UKM_TRY(ws_alloc_t(c, ((size_t)1 << B) + 1, &dir));
    d->keys = keys; d->dir = dir; d->n = n; d->shift = key_bits - B; d->nb = 1u << B;
    hipLaunchKernelGGL(dir_build_kernel, dim3((unsigned)(((u64)d->nb + 1 + 255) / 256)), dim3(256), 0, c->stream, keys, n, d->shift, d->nb, dir);
    UKM_HIP(hipGetLastError());
    return UKM_OK;
}

}  // namespace
