// ukm_route.hip — the pieces the n-way device routes share (ukm_route.h): the device stream table, the cut kernel of
// the range folds and the probe union, and the gather that ends a range-partitioned route.
#include <vector>

#include "ukm_device.h"
#include "ukm_route.h"

int ukm_stream_tab(ukm_ctx *c, const UkmStreams &in, StreamTab *t, const u64 *extra, size_t nextra) {
    const size_t S = (size_t)in.S;
    std::vector<u64> tab(4 * S + nextra);
    for (size_t j = 0; j < S; j++) {
        tab[j] = (u64)(uintptr_t)in.keys[j];
        tab[S + j] = (u64)(uintptr_t)((in.tax && in.taxids) ? in.taxids[j] : nullptr);
        tab[2 * S + j] = in.lens[j];
        tab[3 * S + j] = in.file_taxid((int)j);
    }
    for (size_t i = 0; i < nextra; i++) tab[4 * S + i] = extra[i];
    t->S = (u32)S;
    UKM_TRY(ws_alloc_t(c, tab.size(), &t->d));
    UKM_HIP(hipMemcpyAsync(t->d, tab.data(), tab.size() * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    UKM_HIP(hipStreamSynchronize(c->stream));  // `tab` is a pageable host buffer of this frame
    return UKM_OK;
}

namespace {

// (Bracketing every cut around its interpolated position made the kernel slower in round 3, 1.8 -> 2.9 ms; a two-level
//  search -- every 64th range, then an interpolated window between two coarse cuts -- measured the same 1.76 ms in round 6:
//  the kernel is bound by the ~8 cold lines of a search's last levels, which either form still touches.)
__global__ void range_cuts_kernel(RangeCuts a) {
    // (with the threads of a block on 256 ranges of ONE file every store was a line of its own: 1.77 -> 1.63 ms on config 3)
    const u32 tiles_j = (a.S1 + 15) / 16;
    const u32 tr = blockIdx.x / tiles_j, tj = blockIdx.x % tiles_j;
    const u32 j = tj * 16 + (threadIdx.x & 15), r = tr * 16 + (threadIdx.x >> 4);
    if (j >= a.S1 || r > a.R) return;
    const u64 len = a.lens[j];
    u64 res;
    if (r == 0) {
        res = 0;
    } else if (r == a.R) {
        res = len;
    } else {
        const u64 v = a.base[(u64)r * a.L];
        const auto f = as_global(a.files[j]);
        u64 lo = 0, hi = len;
        while (lo < hi) {
            const u64 mid = (lo + hi) >> 1;
            if (f[mid] < v) lo = mid + 1; else hi = mid;
        }
        res = lo;
    }
    a.cuts[(u64)r * a.S1 + j] = res;
}

__global__ void range_gather_kernel(RangeGather g, const u64 *excl, u64 *out, u32 *tout, u64 cap) {
    const u32 r = blockIdx.x / g.parts, part = blockIdx.x % g.parts;
    const u64 off = g.slot ? g.slot[r] : (u64)r * g.stride;
    const u64 n = g.cnt[r], d0 = excl[r];
    if (d0 + n > cap) return;  // the host reports UKM_ERR_CAPACITY
    const u64 lo = n * part / g.parts, hi = n * (part + 1) / g.parts;
    for (u64 i = lo + threadIdx.x; i < hi; i += blockDim.x) out[d0 + i] = g.src_k[off + i];
    if (tout)
        for (u64 i = lo + threadIdx.x; i < hi; i += blockDim.x) tout[d0 + i] = g.src_t[off + i];
}

}  // namespace

int ukm_launch_range_cuts(ukm_ctx *c, const RangeCuts &a) {
    const u64 blocks = (((u64)a.R + 1 + 15) / 16) * (((u64)a.S1 + 15) / 16);
    hipLaunchKernelGGL(range_cuts_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, a);
    UKM_HIP(hipGetLastError());
    return UKM_OK;
}

int ukm_range_finish(ukm_ctx *c, const RangeGather &g, u64 *ctl, const UkmOut &o, u64 h[2]) {
    if (g.cnt) {
        u64 *excl = nullptr;
        UKM_TRY(ws_alloc_t(c, (size_t)g.R + 1, &excl));
        UKM_TRY(ukm_dev_exclusive_scan_u64(c, g.cnt, excl, g.R, ctl));  // ctl[0] = total
        hipLaunchKernelGGL(range_gather_kernel, dim3(g.R * (unsigned)g.parts), dim3(256), 0, c->stream, g, excl, o.keys,
                           g.src_t ? o.taxids : nullptr, o.cap);
        UKM_HIP(hipGetLastError());
    }
    h[0] = h[1] = 0;
    return ukm_read_u64(c, ctl, h, 2);
}

int ukm_route_answer(u64 n, const UkmOut &o, bool *declined) {
    *o.n = n;
    if (n > o.cap)
        UKM_FAIL(UKM_ERR_CAPACITY, "output needs %llu records, capacity is %llu", (unsigned long long)n, (unsigned long long)o.cap);
    *declined = false;
    return UKM_OK;
}
