// ukm_tsplit.hip — ukm_tsplit: the records of a stream grouped by taxid (tsplit.go:112-192, the map taxid -> codes).
//
// A stable grouping is a stable sort of (taxid, record index) pairs: ukm_dev_sort with 32 key bits, the taxid widened to the
// sort's u64 key and the record index as its u32 payload.  One tiled kernel then does the rest in a single pass over the
// sorted pairs: it gathers out_keys[j] = keys[idx[j]], flags the run heads (sorted taxid differs from its predecessor's)
// and compacts them into (taxid, start) with the block scan and the look-back of ukm_device.h (launch protocol:
// ukm_lb_launch).  A tile is 256 threads x 8 consecutive positions.  The last tile leaves the number of groups in result
// word [0] and closes group_off with n.  Too small an out_keys: nothing is gathered; too small a group array: the heads
// that fit are written, the count goes on.
#include <algorithm>

#include "ukm_device.h"

namespace {

constexpr int NT = 256;
constexpr int VT = 8;
constexpr int TILE = NT * VT;
enum : u64 { TS_FLAG_TIMEOUT = 4 };  // result word [1]

struct SplitArgs {
    const u64 *keys;   // the caller's codes
    const u64 *stax;   // sorted taxids (as u64 sort keys)
    const u32 *idx;    // record index of every sorted position
    u64 n;
    u64 *out;          // null: out_cap < n, no gather
    u32 *gtax;
    u64 *goff;         // group_cap + 1 entries, or null (size query)
    u64 group_cap;
    u64 *status;
    u32 *ticket;
    u64 *result;       // [0] groups, [1] flags
    u64 ntiles;
};

__global__ void pairs_kernel(const u32 *taxids, u64 n, u64 *stax, u32 *idx) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        stax[i] = (u64)taxids[i];
        idx[i] = (u32)i;
    }
}

template <bool TICKET>
__global__ __launch_bounds__(NT) void split_kernel(SplitArgs p) {
    __shared__ u32 s_scan[NT / 64 + 1];
    __shared__ u64 s_misc[2];
    const int tid = (int)threadIdx.x, lane = lane_id();
    const u64 tile = lb_tile_id<TICKET>(p.ticket, &s_misc[0]);
    if (tile >= p.ntiles) return;
    const u64 j0 = tile * (u64)TILE + (u64)tid * VT;
    u64 tk[VT];
    u32 heads = 0;
    u64 prev = 0;
    if (j0 > 0 && j0 < p.n) prev = p.stax[j0 - 1];
#pragma unroll
    for (int s = 0; s < VT; s++) {
        const u64 j = j0 + s;
        const bool in = j < p.n;
        tk[s] = in ? p.stax[j] : 0;
        if (in && (j == 0 || tk[s] != prev)) heads |= 1u << s;
        prev = tk[s];
    }
    if (p.out) {
        u32 src[VT];
#pragma unroll
        for (int s = 0; s < VT; s++) src[s] = j0 + s < p.n ? p.idx[j0 + s] : 0u;
        u64 v[VT];
#pragma unroll
        for (int s = 0; s < VT; s++) v[s] = j0 + s < p.n ? p.keys[src[s]] : 0;  // (eight independent gathers in flight)
#pragma unroll
        for (int s = 0; s < VT; s++)
            if (j0 + s < p.n) p.out[j0 + s] = v[s];
    }
    u32 tot;
    const u32 excl = block_excl_scan_u32<NT>((u32)__popc(heads), s_scan, &tot);
    const u64 base = lb_tile_base<TICKET>(p.status, tile, (u64)tot, &p.result[1], TS_FLAG_TIMEOUT, &s_misc[1], tid, lane);
    u64 pos = base + excl;
#pragma unroll
    for (int s = 0; s < VT; s++)
        if ((heads >> s) & 1u) {
            if (pos < p.group_cap) {
                p.gtax[pos] = (u32)tk[s];
                p.goff[pos] = j0 + s;
            }
            pos++;
        }
    if (tid == 0 && tile == p.ntiles - 1) {
        const u64 groups = base + tot;
        p.result[0] = groups;
        if (p.goff && groups <= p.group_cap) p.goff[groups] = p.n;
    }
}

template <bool TICKET>
int launch_split(ukm_ctx *c, const SplitArgs &p) {
    hipLaunchKernelGGL((split_kernel<TICKET>), dim3((unsigned)p.ntiles), dim3(NT), 0, c->stream, p);
    return UKM_OK;
}

// all pointers are device pointers (out / gtax / goff: null where the caller gave none); 1 <= n < 2^32
int dev_tsplit(ukm_ctx *c, const u64 *keys, const u32 *taxids, u64 n, u64 *out, u64 out_cap, u32 *gtax, u64 *goff, u64 group_cap,
               u64 *n_groups) {
    const char *name = "ukm_tsplit";
    u64 *stax = nullptr;
    u32 *idx = nullptr;
    UKM_TRY(ws_alloc_t(c, n, &stax));
    UKM_TRY(ws_alloc_t(c, n, &idx));
    const unsigned blocks = (unsigned)std::max<u64>(1, std::min<u64>((n + NT - 1) / NT, (u64)c->num_cu * 16));
    hipLaunchKernelGGL(pairs_kernel, dim3(blocks), dim3(NT), 0, c->stream, taxids, n, stax, idx);
    UKM_HIP(hipGetLastError());
    UKM_TRY(ukm_dev_sort(c, stax, idx, n, 32));
    SplitArgs p;
    memset(&p, 0, sizeof(p));
    p.keys = keys; p.stax = stax; p.idx = idx; p.n = n;
    p.out = out_cap >= n ? out : nullptr;
    p.gtax = gtax; p.goff = goff;
    p.group_cap = (gtax && goff) ? group_cap : 0;
    p.ntiles = (n + TILE - 1) / TILE;
    LbCtl blk;
    UKM_TRY(ukm_lb_ctl_alloc(c, p.ntiles, 0, &blk));
    p.status = blk.status; p.ticket = blk.ticket; p.result = blk.result;
    u64 res[2] = {0, 0};
    const LbLaunch how = {name, "split kernel", TS_FLAG_TIMEOUT, false, false, false};
    UKM_TRY(ukm_lb_launch(c, blk, how, [&](bool ticket) { return ticket ? launch_split<true>(c, p) : launch_split<false>(c, p); }, res));
    *n_groups = res[0];
    if (out_cap < n || group_cap < res[0])
        UKM_FAIL(UKM_ERR_CAPACITY, "%s: the output needs %llu records and %llu groups, the capacities are %llu and %llu", name,
                 (unsigned long long)n, (unsigned long long)res[0], (unsigned long long)out_cap, (unsigned long long)group_cap);
    return UKM_OK;
}

}  // namespace

extern "C" int ukm_tsplit(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint64_t n, uint64_t *out_keys, uint64_t out_cap,
                          uint32_t *group_taxids, uint64_t *group_off, uint64_t group_cap, uint64_t *n_groups) {
    const char *name = "ukm_tsplit";
    if (!ctx || !n_groups || (!keys && n) || (!out_keys && out_cap) || ((!group_taxids || !group_off) && group_cap))
        UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
    if (!taxids && n) UKM_FAIL(UKM_ERR_INVALID, "%s: taxids is NULL; records without taxids of their own need no split", name);
    if (n >= (1ull << 32)) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu records in one call; the limit is 2^32 - 1", name, (unsigned long long)n);
    *n_groups = 0;
    if (n == 0) return UKM_OK;
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        const u64 *k = nullptr;
        const u32 *t = nullptr;
        u64 *out = nullptr, *goff = nullptr;
        u32 *gtax = nullptr;
        UKM_TRY(ukm_in_t(ctx, keys, n, &k));
        UKM_TRY(ukm_in_t(ctx, taxids, n, &t));
        UKM_TRY(ukm_out_t(ctx, out_keys, out_cap, &out));
        UKM_TRY(ukm_out_t(ctx, group_taxids, group_cap, &gtax));
        UKM_TRY(ukm_out_t(ctx, group_off, group_cap + 1, &goff));
        const int r = dev_tsplit(ctx, k, t, n, out, out_cap, gtax, goff, group_cap, n_groups);
        const u64 g = *n_groups;
        ukm_out_resize(ctx, out_keys, r == UKM_OK ? n * sizeof(u64) : 0);
        ukm_out_resize(ctx, group_taxids, r == UKM_OK ? g * sizeof(u32) : 0);
        ukm_out_resize(ctx, group_off, r == UKM_OK ? (g + 1) * sizeof(u64) : 0);
        return r;
    }();
    return ukm_finish(&s, rc);
}
