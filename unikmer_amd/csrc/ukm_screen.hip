// ukm_screen.hip — which records belong to a k-mer set: per record the number of windows, the number of windows whose value
// is in a sorted code set, and the LCA of the taxids of those hits (contract: include/unikmer_hip.h).
//
// A record's result is a fold with an order-independent combine over five integers:
//   hits (add) | min, max of the hits' RAW taxids ("all the same number") | min, max of their pre-order numbers euler[taxid]
//   (0 = taxid 0, absent or unknown: TaxDev::euler; the LCA of a set is the LCA of its members with the smallest and the
//   largest number).
// so tiles need no order among themselves and no look-back:
//   screen_kernel  one workgroup per tile of SCREEN_TILE consecutive windows (ukm_screen.h).  The tile finds the records that
//                  start inside it from win_off (one binary search for the record of its first window, then a walk) and
//                  raises head marks in LDS; every thread folds its SCREEN_VT consecutive windows and hands the part of a record
//                  that crosses a thread's edge to the LDS slot of the thread the record started in (slot 0: the record that
//                  was open when the tile began) with LDS atomics.  A record that lies wholly inside one thread or one tile is
//                  stored plainly; the at most two records that cross the tile's edges go to the per-record state with global
//                  atomics (the state is identity-initialised: zeros for add / max, ones for min).
//                  Source LOOKUP: the windows look their codes up through the prefix directory (ukm_dir.h) in genome order --
//                  no per-window array is written.  Source WORD: the sorted route has left one word per window (0 = miss, else
//                  1 + index into the set); the SAME kernel reads that word instead of searching.
//   finish_kernel  one thread per record: state -> out_hit, out_lca (closed form of the left fold: DESIGN.md 4.24).
// The routes and their option ("map_sorted") are ukm_map's; the threshold is this call's own (ukm_map.h).
#include <algorithm>

#include "ukm_device.h"
#include "ukm_dir.h"
#include "ukm_map.h"
#include "ukm_screen.h"

namespace {

constexpr int NT = SCREEN_NT, VT = SCREEN_VT, TILE = SCREEN_TILE;
constexpr u32 NO_REC = 0xFFFFFFFFu;

// the per-record state, [n_rec] words each: three columns that start as zeros, two that start as ones
struct RecState {
    u32 *hit, *max_raw, *max_e, *min_raw, *min_e;
};

struct Fold {
    u32 hit, min_raw, max_raw, min_e, max_e;
};
__device__ __forceinline__ Fold fold_identity() { return {0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u}; }

struct ScreenArgs {
    const u64 *w;        // LOOKUP: window values in genome order
    const u32 *word;     // WORD: per window 0 = miss, else 1 + the lower bound of its code in the set
    u64 n;               // windows
    const u64 *win_off;  // [n_rec + 1] first window of every record
    u64 n_rec;
    Dir d;
    const u32 *taxids;   // TAX: [d.n]
    TaxDev T;
    RecState st;
};

template <bool TAX>
struct ScreenLds {
    u32 head[TILE];                   // the record whose first window this is, or NO_REC
    u32 slot_rec[NT + 1];             // slot 0: the record of the tile's first window; slot t + 1: the last record that starts in thread t
    u32 acc[TAX ? 5 : 1][NT + 1];     // hit, max_raw, max_e, min_raw, min_e of every slot
    u32 wave_last[NT / 64];           // 1 + the last thread of the wave with a head, 0 = none
};

template <bool TAX>
__device__ __forceinline__ void store_plain(const RecState &st, u32 rec, const Fold &f) {
    st.hit[rec] = f.hit;
    if (TAX) { st.max_raw[rec] = f.max_raw; st.max_e[rec] = f.max_e; st.min_raw[rec] = f.min_raw; st.min_e[rec] = f.min_e; }
}

template <bool WORD, bool TAX>
__global__ __launch_bounds__(NT) void screen_kernel(ScreenArgs p) {
    __shared__ ScreenLds<TAX> L;
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const u64 t0 = (u64)blockIdx.x * TILE;                 // (t0 < n: the grid has ceil(n / TILE) workgroups)
    const u64 t1 = t0 + TILE < p.n ? t0 + TILE : p.n;
    const u64 i0 = t0 + (u64)tid * VT;

    // ---- the records that start inside the tile
#pragma unroll
    for (int s = 0; s < VT; s++) L.head[tid * VT + s] = NO_REC;
    for (int j = tid; j <= NT; j += NT) {
        L.slot_rec[j] = NO_REC;
        L.acc[0][j] = 0u;
        if (TAX) { L.acc[1][j] = 0u; L.acc[2][j] = 0u; L.acc[3][j] = 0xFFFFFFFFu; L.acc[4][j] = 0xFFFFFFFFu; }
    }
    // the record of window t0: the last one with win_off[r] <= t0 (empty records in front of t0 are skipped by the search;
    // win_off[0] = 0 <= t0 < n = win_off[n_rec], so 0 <= r_first < n_rec)
    const u64 r_first = lower_bound_u64(p.win_off, 0, p.n_rec + 1, t0 + 1) - 1;
    __syncthreads();
    for (u64 base = r_first + 1;; base += NT) {
        const u64 r = base + (u64)tid;
        if (r < p.n_rec) {
            const u64 a = p.win_off[r];  // (> t0 for every r > r_first)
            if (a < t1 && p.win_off[r + 1] > a) L.head[a - t0] = (u32)r;  // (records without windows raise no mark)
        }
        const u64 last = base + NT - 1;  // (uniform: does the next chunk still start inside the tile?)
        if (last >= p.n_rec || p.win_off[last] >= t1) break;
    }
    __syncthreads();

    u32 head[VT];
    u32 last_head = NO_REC;
#pragma unroll
    for (int s = 0; s < VT; s++) {
        head[s] = L.head[tid * VT + s];
        if (head[s] != NO_REC) last_head = head[s];
    }
    const bool has_head = last_head != NO_REC;
    const u64 hm = __ballot(has_head);
    if (lane == 0) L.wave_last[wave] = hm ? (u32)(wave * 64 + 63 - __builtin_clzll(hm) + 1) : 0u;
    if (has_head) L.slot_rec[tid + 1] = last_head;
    if (tid == 0) L.slot_rec[0] = (u32)r_first;

    // ---- membership (and the hits' taxids) of this thread's windows
    u32 valid = 0;
#pragma unroll
    for (int s = 0; s < VT; s++) valid |= (i0 + s < p.n) ? 1u << s : 0u;
    u32 hit = 0;
    u32 lo[VT];
    if (WORD) {
#pragma unroll
        for (int s = 0; s < VT; s++) {
            const u32 wd = ((valid >> s) & 1u) ? p.word[i0 + s] : 0u;
            lo[s] = wd - 1u;
            hit |= wd ? 1u << s : 0u;
        }
    } else {
        u64 x[VT];
#pragma unroll
        for (int s = 0; s < VT; s++) x[s] = ((valid >> s) & 1u) ? p.w[i0 + s] : 0;
        hit = dir_search_n<VT>(p.d, x, valid, lo);  // (ukm_dir.h: the eight searches side by side)
    }
    u32 raw[VT], eul[VT];
    if (TAX) {
#pragma unroll
        for (int s = 0; s < VT; s++) raw[s] = ((hit >> s) & 1u) ? p.taxids[lo[s]] : 0u;
#pragma unroll
        for (int s = 0; s < VT; s++) eul[s] = (((hit >> s) & 1u) && raw[s] < p.T.size) ? p.T.euler[raw[s]] : 0u;
    }
    __syncthreads();

    // the slot of the record that is open at this thread's first window: the nearest thread in front with a head, else 0
    u32 in_slot = 0;
    {
        const u64 below = hm & ((1ull << lane) - 1ull);
        if (below) in_slot = (u32)(wave * 64 + 63 - __builtin_clzll(below) + 1);
        else
            for (int w2 = 0; w2 < wave; w2++) {
                const u32 v = L.wave_last[w2];
                if (v) in_slot = v;
            }
    }
    auto to_slot = [&](u32 slot, const Fold &f) {
        if (f.hit == 0) return;  // (the identity)
        atomicAdd(&L.acc[0][slot], f.hit);
        if (TAX) {
            atomicMax(&L.acc[1][slot], f.max_raw);
            atomicMax(&L.acc[2][slot], f.max_e);
            atomicMin(&L.acc[3][slot], f.min_raw);
            atomicMin(&L.acc[4][slot], f.min_e);
        }
    };
    Fold cur = fold_identity();
    bool own = false;  // the record being folded started in this thread
    u32 cur_rec = 0;
#pragma unroll
    for (int s = 0; s < VT; s++) {
        if (head[s] != NO_REC) {
            // a record ends in front of window s.  Started in this thread: all of it is here.
            if (own) { if (cur.hit) store_plain<TAX>(p.st, cur_rec, cur); }
            else to_slot(in_slot, cur);
            cur = fold_identity();
            own = true;
            cur_rec = head[s];
        }
        if ((hit >> s) & 1u) {
            cur.hit++;
            if (TAX) {
                cur.min_raw = raw[s] < cur.min_raw ? raw[s] : cur.min_raw;
                cur.max_raw = raw[s] > cur.max_raw ? raw[s] : cur.max_raw;
                cur.min_e = eul[s] < cur.min_e ? eul[s] : cur.min_e;
                cur.max_e = eul[s] > cur.max_e ? eul[s] : cur.max_e;
            }
        }
    }
    to_slot(own ? (u32)tid + 1u : in_slot, cur);  // (the record that is open at the thread's end)
    __syncthreads();

    // ---- the slots: a record wholly inside the tile is stored, one that crosses an edge is combined
    for (int j = tid; j <= NT; j += NT) {
        Fold f;
        f.hit = L.acc[0][j];
        if (f.hit == 0) continue;
        if (TAX) { f.max_raw = L.acc[1][j]; f.max_e = L.acc[2][j]; f.min_raw = L.acc[3][j]; f.min_e = L.acc[4][j]; }
        const u32 rec = L.slot_rec[j];  // (a slot with hits has its record: slot 0 always, slot t + 1 when thread t has a head)
        if (rec == NO_REC) continue;
        if (p.win_off[rec] >= t0 && p.win_off[(u64)rec + 1] <= t1) {
            store_plain<TAX>(p.st, rec, f);
        } else {
            atomicAdd(&p.st.hit[rec], f.hit);
            if (TAX) {
                atomicMax(&p.st.max_raw[rec], f.max_raw);
                atomicMax(&p.st.max_e[rec], f.max_e);
                atomicMin(&p.st.min_raw[rec], f.min_raw);
                atomicMin(&p.st.min_e[rec], f.min_e);
            }
        }
    }
}

// the sorted route: (hk, hv) = every (code, window) sorted by code; one word per window, scattered back to window order
__global__ void sorted_lookup_kernel(const u64 *hk, const u32 *hv, u64 n, Dir d, u32 *word) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const u64 code = hk[j];
    const u32 lb = dir_lower_bound(d, code);
    word[hv[j]] = ((u64)lb < d.n && d.keys[lb] == code) ? lb + 1u : 0u;
}

__global__ void win_count_kernel(const u64 *win_off, u64 n_rec, u32 *out_win) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_rec) out_win[r] = (u32)(win_off[r + 1] - win_off[r]);
}

// The left fold of ukm_lca's contract over a record's hit taxids, from the state: no hit 0; one raw number
// that number; a member without a pre-order number 0; else the LCA of the members with the smallest and the largest number.
__global__ void finish_kernel(RecState st, u64 n_rec, TaxDev T, int tax, u32 *out_hit, u32 *out_lca) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rec) return;
    const u32 hit = st.hit[r];
    if (out_hit) out_hit[r] = hit;
    if (!out_lca) return;
    u32 l = 0;
    if (tax && hit) {
        const u32 mn = st.min_raw[r], mx = st.max_raw[r], e0 = st.min_e[r], e1 = st.max_e[r];
        if (mn == mx) l = mn;
        else if (e0 != 0) l = lca_dev(T, T.node_at[e0], T.node_at[e1]);
    }
    out_lca[r] = l;
}

unsigned blocks_for(u64 n) { return (unsigned)((n + NT - 1) / NT); }

template <bool WORD>
void launch_screen(ukm_ctx *c, const ScreenArgs &p, bool tax) {
    const unsigned ntiles = (unsigned)((p.n + TILE - 1) / TILE);
    if (tax) hipLaunchKernelGGL((screen_kernel<WORD, true>), dim3(ntiles), dim3(NT), 0, c->stream, p);
    else hipLaunchKernelGGL((screen_kernel<WORD, false>), dim3(ntiles), dim3(NT), 0, c->stream, p);
}

// everything behind the argument checks; ow / oh / ol = the outputs on the device (each may be null)
int screen_records(ukm_ctx *ctx, const char *name, const u8 *bases, const u64 *rec_off, u64 n_rec, int k, int canonical, int circular,
                   int hashed, const u64 *set_keys, const u32 *set_taxids, u64 n_set, u32 *ow, u32 *oh, u32 *ol) {
    const bool tax = ol != nullptr && set_taxids != nullptr && n_set != 0;
    const u64 *set = nullptr;
    const u32 *tx = nullptr;
    if (n_set) {
        UKM_TRY(ukm_in_t(ctx, set_keys, n_set, &set));
        bool sorted = true, strict = true;
        UKM_TRY(ukm_dev_check_sorted(ctx, set, n_set, &sorted, &strict));
        if (!sorted) UKM_FAIL(UKM_ERR_UNSORTED, "%s: the code set is not sorted", name);
        if (tax) UKM_TRY(ukm_in_t(ctx, set_taxids, n_set, &tx));
    }
    auto zero = [&](u32 *o) -> int {
        if (o) UKM_HIP(hipMemsetAsync(o, 0, n_rec * sizeof(u32), ctx->stream));
        return UKM_OK;
    };
    if (!bases) {  // (records without a single base need no text: a caller's empty array has no address)
        u64 total = 0;
        if (ukm_is_device_ptr(rec_off)) UKM_TRY(ukm_read_u64(ctx, rec_off + n_rec, &total));
        else total = rec_off[n_rec];
        if (total) UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
        UKM_TRY(zero(ow));
        UKM_TRY(zero(oh));
        return zero(ol);
    }
    MapWindows W;  // (also without a set: an illegal base is an error)
    UKM_TRY(ukm_dev_make_windows(ctx, name, bases, rec_off, n_rec, k, canonical, circular, hashed, &W));
    if (W.n == 0) {  // (every record is shorter than k; win_off may be null)
        UKM_TRY(zero(ow));
        UKM_TRY(zero(oh));
        return zero(ol);
    }
    if (ow) {
        hipLaunchKernelGGL(win_count_kernel, dim3(blocks_for(n_rec)), dim3(NT), 0, ctx->stream, W.win_off, n_rec, ow);
        UKM_HIP(hipGetLastError());
    }
    if (n_set == 0) {
        UKM_TRY(zero(oh));
        return zero(ol);
    }
    if (!oh && !ol) return UKM_OK;
    // the state: [hit | max_raw | max_e] zeros, [min_raw | min_e] ones (without taxids: the hits alone)
    u32 *state = nullptr;
    UKM_TRY(ws_alloc_t(ctx, (size_t)(tax ? 5 : 1) * n_rec, &state));
    UKM_HIP(hipMemsetAsync(state, 0, (size_t)(tax ? 3 : 1) * n_rec * sizeof(u32), ctx->stream));
    if (tax) UKM_HIP(hipMemsetAsync(state + 3 * n_rec, 0xFF, (size_t)2 * n_rec * sizeof(u32), ctx->stream));
    ScreenArgs p;
    memset(&p, 0, sizeof(p));
    p.n = W.n; p.win_off = W.win_off; p.n_rec = n_rec; p.taxids = tx; p.T = ukm_taxdev(ctx);
    p.st.hit = state;
    if (tax) { p.st.max_raw = state + n_rec; p.st.max_e = state + 2 * n_rec; p.st.min_raw = state + 3 * n_rec; p.st.min_e = state + 4 * n_rec; }
    const int key_bits = hashed ? 64 : 2 * k;
    UKM_TRY(build_dir(ctx, set, n_set, key_bits, ukm_map_dir_slack(ctx), &p.d));
    if (ukm_map_sorted_route(ctx, n_set, SCREEN_SORTED_MIN_KEYS)) {
        u32 *wi = nullptr, *word = nullptr;
        UKM_TRY(ukm_dev_sort_windows(ctx, W.w, W.n, key_bits, &wi));
        UKM_TRY(ws_alloc_t(ctx, W.n, &word));
        (void)hipEventRecord(ctx->ev_k0, ctx->stream);
        hipLaunchKernelGGL(sorted_lookup_kernel, dim3(blocks_for(W.n)), dim3(NT), 0, ctx->stream, W.w, wi, W.n, p.d, word);
        p.word = word;
        launch_screen<true>(ctx, p, tax);
    } else {
        p.w = W.w;
        (void)hipEventRecord(ctx->ev_k0, ctx->stream);
        launch_screen<false>(ctx, p, tax);
    }
    (void)hipEventRecord(ctx->ev_k1, ctx->stream);
    ctx->evk_valid = true;
    UKM_HIP(hipGetLastError());
    hipLaunchKernelGGL(finish_kernel, dim3(blocks_for(n_rec)), dim3(NT), 0, ctx->stream, p.st, n_rec, p.T, tax ? 1 : 0, oh, ol);
    UKM_HIP(hipGetLastError());
    return UKM_OK;
}

}  // namespace

extern "C" int ukm_screen(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off, uint64_t n_rec, int k, int canonical,
                          int circular, int hashed, const uint64_t *set_keys, const uint32_t *set_taxids, uint64_t n_set,
                          uint32_t *out_win, uint32_t *out_hit, uint32_t *out_lca) {
    const char *name = "ukm_screen";
    if (!ctx || (n_rec && !rec_off) || (n_set && !set_keys)) UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
    if (k < 1 || k > (hashed ? 64 : 32)) UKM_FAIL(UKM_ERR_K, "%s: k = %d out of range", name, k);
    if (out_lca && !set_taxids && n_set) UKM_FAIL(UKM_ERR_INVALID, "%s: out_lca needs set_taxids", name);
    if (n_rec >= (1ull << 32))
        UKM_FAIL(UKM_ERR_INVALID, "%s: %llu records in one call; the limit is 2^32 - 1: split the records over several calls", name,
                 (unsigned long long)n_rec);
    if (n_set >= (1ull << 32)) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu codes in the set; the limit is 2^32 - 1", name, (unsigned long long)n_set);
    if (out_lca && set_taxids && !ctx->tax_parent) UKM_FAIL(UKM_ERR_NO_TAXONOMY, "%s: no taxonomy loaded", name);
    if (n_rec == 0) return UKM_OK;
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        u32 *ow = nullptr, *oh = nullptr, *ol = nullptr;
        UKM_TRY(ukm_out_t(ctx, out_win, n_rec, &ow));
        UKM_TRY(ukm_out_t(ctx, out_hit, n_rec, &oh));
        UKM_TRY(ukm_out_t(ctx, out_lca, n_rec, &ol));
        return screen_records(ctx, name, bases, rec_off, n_rec, k, canonical, circular, hashed, set_keys, set_taxids, n_set, ow, oh, ol);
    }();
    return ukm_finish(&s, rc);
}
