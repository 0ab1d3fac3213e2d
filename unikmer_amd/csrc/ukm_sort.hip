// ukm_sort.hip — LSD radix sort of uint64 codes (optionally carrying uint32 taxids), the
// MI355X replacement for sortutil.Uint64s / sorts.Quicksort(CodeTaxidSlice)
// (twotwotwo/sorts; call sites count.go:581, union.go:274,295, sort.go:268,331,457,463 ...).
//
// Design (HBM-bound, integer):
//   * one histogram kernel reads the keys once and builds the 256-bin digit histograms of ALL
//     passes (LDS atomics, with a wave-uniform fast path so sorted/skewed input does not
//     serialise on one bin); the host turns them into per-pass digit bases and drops passes
//     whose digit is constant (k=31 -> 62 significant bits; top bits of k=21 codes are zero);
//   * per executed pass ONE "onesweep" kernel: each 1024-thread workgroup takes a ticketed tile
//     of 14336 keys (1024 threads x 14; 11264 = 1024 x 11 with taxids), ranks them stably with wave64 ballot match-any (8 ballots per key) into
//     per-wave LDS digit counters, resolves the tile's global digit offsets by a per-digit
//     decoupled look-back over the previous tiles' counts (thread d owns digit d), reorders
//     the tile through LDS so that global stores are contiguous per digit, and scatters.
//   Algorithmic bytes: 8n (histogram) + P * (8n read + 8n write) [+ P * 8n for taxids].
//
// The unit by layer:
//   ukm_sort_plan.h     plain host C++: knobs and thresholds, the bucket route's plan and admission test, the route choice
//                       (SortRoute), the size classes, the skew verdicts
//   ukm_sort_state.h    plain host C++: the policy and statistics a context keeps between sorts (SortPolicy; in ukm_ctx as SortState)
//   ukm_sort_kernels.h  radix_hist_kernel, radix_bases_kernel, match_any8, PassArgs, onesweep_kernel
//   ukm_sort_buckets.h  LocalSortArgs and the ls_* kernels of the bucket route
//   this file           the steps the routes share, one function per route (sort_chunked, sort_buckets, sort_fused,
//                       sort_host_hist), ukm_dev_sort_hist that asks the plan for a route and runs it, the C entries
#include <algorithm>
#include <utility>
#include <vector>

#include "ukm_device.h"
#include "ukm_sort_plan.h"

namespace {

#include "ukm_sort_kernels.h"
#include "ukm_sort_buckets.h"

// ---- steps the routes share ------------------------------------------------------------------------------------------------
bool sort_local_enabled(const ukm_ctx *c) { return !ukm_env_is(c, "UKM_SORT_LOCAL", '0'); }  // developer knob: 0 = all passes through HBM

// a scratch copy of n records: what the scatter passes, and the merges of the chunks, ping-pong with
int scratch_pair(ukm_ctx *c, u64 n, bool pairs, u64 **tk, u32 **tv) {
    *tv = nullptr;
    UKM_TRY(ws_alloc_t(c, n, tk));
    return pairs ? ws_alloc_t(c, n, tv) : UKM_OK;
}

// the result sits in the scratch copy: back to the caller's array
int copy_back(ukm_ctx *c, u64 *keys, u32 *vals, const u64 *tk, const u32 *tv, u64 n, bool in_tmp) {
    if (in_tmp) {
        UKM_HIP(hipMemcpyAsync(keys, tk, n * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
        if (vals) UKM_HIP(hipMemcpyAsync(vals, tv, n * sizeof(u32), hipMemcpyDeviceToDevice, c->stream));
    }
    return UKM_OK;
}

// the histograms of `passes` digits from shift0 on (and the OR of all keys, when asked for) by one pass over the keys
int launch_first_hist(ukm_ctx *c, const u64 *keys, u64 n, int passes, u64 *hist, u64 *or_all, int shift0) {
    const unsigned blocks = (unsigned)std::min<u64>((n + 4095) / 4096, (u64)c->num_cu * 8);
    hipLaunchKernelGGL(radix_hist_kernel, dim3(blocks), dim3(NT), 0, c->stream, keys, n, passes, hist, or_all, shift0);
    UKM_HIP(hipGetLastError());
    return UKM_OK;
}

// A caller that could not narrow key_bits (64) gets ONE 8-byte read-back: the OR of all keys, gathered by the histogram
// pre-pass for free, tells which high digits are zero everywhere (hashes restricted by a Scaled threshold, k <= 28 codes
// handed over as plain uint64).
int key_width_from_or(ukm_ctx *c, const u64 *or_all, int *bits) {
    u64 orv = 0;
    UKM_TRY(ukm_read_u64(c, or_all, &orv));
    *bits = orv ? 64 - __builtin_clzll(orv) : 1;
    return UKM_OK;
}

template <typename SW, bool PAIRS, int NT_, int VT_>
int run_passes(ukm_ctx *c, u64 *keys, u32 *vals, u64 *tk, u32 *tv, u64 n, int npass,
               const int *shifts, const u64 *gbase_dev, bool *result_in_tmp, u64 *fused_hist) {
    constexpr int TILE = NT_ * VT_;
    const u64 ntiles = (n + TILE - 1) / TILE;
    SW *status = nullptr;
    u32 *ticket = nullptr;
    UKM_TRY(ws_alloc_t(c, ntiles * RADIX, &status));
    UKM_TRY(ws_alloc_t(c, 1, &ticket));
    u64 *src_k = keys, *dst_k = tk;
    u32 *src_v = vals, *dst_v = tv;
    for (int i = 0; i < npass; i++) {
        UKM_HIP(hipMemsetAsync(status, 0, ntiles * RADIX * sizeof(SW), c->stream));
        UKM_HIP(hipMemsetAsync(ticket, 0, sizeof(u32), c->stream));
        PassArgs<SW> p;
        p.kin = src_k; p.kout = dst_k; p.vin = src_v; p.vout = dst_v;
        p.n = n; p.shift = shifts[i];
        p.status = status; p.ticket = ticket;
        p.gbase = gbase_dev + (size_t)i * RADIX;
        p.ntiles = ntiles;
        p.next_hist = nullptr;
        p.next_shift = 0;
        if (fused_hist) {
            // bases of this pass from its histogram (built by the pre-pass for i = 0, by pass i - 1 otherwise)
            hipLaunchKernelGGL(radix_bases_kernel, dim3(1), dim3(RADIX), 0, c->stream, fused_hist + (size_t)i * RADIX,
                               const_cast<u64 *>(p.gbase));
            if (i + 1 < npass) {
                p.next_hist = fused_hist + (size_t)(i + 1) * RADIX;
                p.next_shift = shifts[i + 1];
            }
        }
        hipLaunchKernelGGL((onesweep_kernel<SW, PAIRS, NT_, VT_>), dim3((unsigned)ntiles), dim3(NT_), 0, c->stream, p);
        UKM_HIP(hipGetLastError());
        std::swap(src_k, dst_k);
        std::swap(src_v, dst_v);
    }
    *result_in_tmp = (src_k != keys);
    return UKM_OK;
}

// npass scatter passes over the digits at `shifts`, ping-pong between the caller's arrays and a scratch copy (*tk, *tv:
// allocated here; *in_tmp: the result sits there); the status words of the look-back are 32-bit below 2^30 keys.  fused_hist (or nullptr: gbase_dev holds every pass's bases already):
// [npass][256], the first digit's histogram filled in; every pass counts the next digit on the fly and a 256-thread kernel
// turns the counts into bases between two passes, so the histograms never leave the device.
int scatter_passes(ukm_ctx *c, u64 *keys, u32 *vals, u64 n, int npass, const int *shifts, const u64 *gbase_dev, u64 *fused_hist,
                   u64 **tk_out, u32 **tv_out, bool *in_tmp) {
    UKM_TRY(scratch_pair(c, n, vals != nullptr, tk_out, tv_out));
    u64 *tk = *tk_out;
    u32 *tv = *tv_out;
    const bool narrow = n < (1ull << 30);
    if (vals) {
        if (narrow) return run_passes<u32, true, SORT_NT_PAIRS, SORT_VT_PAIRS>(c, keys, vals, tk, tv, n, npass, shifts, gbase_dev, in_tmp, fused_hist);
        return run_passes<u64, true, SORT_NT_PAIRS, SORT_VT_PAIRS>(c, keys, vals, tk, tv, n, npass, shifts, gbase_dev, in_tmp, fused_hist);
    }
    if (narrow) return run_passes<u32, false, SORT_NT_KEYS, SORT_VT_KEYS>(c, keys, vals, tk, tv, n, npass, shifts, gbase_dev, in_tmp, fused_hist);
    return run_passes<u64, false, SORT_NT_KEYS, SORT_VT_KEYS>(c, keys, vals, tk, tv, n, npass, shifts, gbase_dev, in_tmp, fused_hist);
}

// ---- route BUCKETS: the top bits by scatter passes, then every bucket inside LDS (ukm_sort_buckets.h) ----------------------------
struct BucketSort {
    ukm_ctx *c;
    u64 *keys;
    u32 *vals;
    u64 n;
    BucketPlan plan;
    u32 nbuckets;
    int kb;                // the keys' width: as declared, or narrowed by the OR word
    u64 *fh, *gb, *start;  // first histogram (+ the OR word), digit bases, bucket bounds [nbuckets + 1]
    u64 *tk;               // the scratch copy (tv: its taxids)
    bool in_tmp;           // the array sorted by its top bits is the scratch copy (three passes)
    // classify's counters on the device, and the lists it fills: ids[k][...] the buckets of class k, big_ids the oversized
    // ones, big_size[b] = bucket b's size if it is oversized, else 0
    u64 *cls, *big_size;
    u32 *tv, *ids, *big_ids;
    // the counters read back: [k < LS_NCLASS] buckets of class k, [LS_NCLASS] oversized buckets, [LS_NCLASS + 1] keys in
    // those, [LS_NCLASS + 2] buckets of the previous bucket-route sort that fell back from the counting step
    u64 hc[LS_NCLASS + 3];
    const u64 *src() const { return in_tmp ? tk : keys; }
    const u32 *vsrc() const { return in_tmp ? tv : vals; }
    int low_bits() const { return kb - plan.topb; }
};

// A sample of 2^20 keys counted by bucket: do the buckets whose share says "beyond 4096 keys" make the route give up?  Run
// before the scatter passes on a context that has already met crowded keys (a wasted attempt costs two passes).
int skew_guard(BucketSort &b, int low_bits, bool *heavy) {
    ukm_ctx *c = b.c;
    u32 *scnt = nullptr;
    u64 *sout = nullptr;
    UKM_TRY(ws_alloc_t(c, (size_t)b.nbuckets, &scnt));
    UKM_TRY(ws_alloc_t(c, 2, &sout));
    UKM_HIP(hipMemsetAsync(scnt, 0, sizeof(u32) * (size_t)b.nbuckets, c->stream));
    UKM_HIP(hipMemsetAsync(sout, 0, 2 * sizeof(u64), c->stream));
    hipLaunchKernelGGL(ls_sample_kernel, dim3(LS_NSAMP / 256), dim3(256), 0, c->stream, b.keys, b.n, low_bits, b.plan.topb, scnt, LS_NSAMP);
    const u32 thr = ls_sample_threshold(b.n, LS_NSAMP);
    hipLaunchKernelGGL(ls_sample_count_kernel, dim3(b.nbuckets / 256), dim3(256), 0, c->stream, scnt, thr, sout);
    UKM_HIP(hipGetLastError());
    u64 found[2] = {0, 0};
    UKM_TRY(ukm_read_u64(c, sout, found, 2));
    if (ukm_env(c, "UKM_SORT_DEBUG"))
        fprintf(stderr, "[sort] sample: %llu buckets look heavier than %u samples, %llu of %u samples in them\n", (unsigned long long)found[0], thr,
                (unsigned long long)found[1], LS_NSAMP);
    *heavy = ls_too_crowded(found[0], found[1], LS_NSAMP);
    return UKM_OK;
}

// The histogram of the first top digit into b.fh, and the keys' width into b.kb.  first_hist (may be null): that histogram
// at first_shift, counted by whoever PRODUCED the keys (ukm_count: the encode kernel) -- it replaces the pre-pass when the
// shift is the one this route uses.  Keys declared 64 bits wide: the pre-pass gathers their OR, and when that is narrower
// the histogram is built again at the narrowed shift.  (57 .. 63 significant bits too: with the width left at 64 only
// 2^(bits - 48) of the top buckets would be populated, the route would run its scatter passes, give up and mark the context
// as one that has met crowded keys.)  b.kb < min_bits on return: narrow keys, nothing more was spent.
int first_hist_and_width(BucketSort &b, int key_bits, const u64 *first_hist, int first_shift) {
    ukm_ctx *c = b.c;
    b.kb = key_bits;
    for (int attempt = 0; attempt < 2; attempt++) {
        const int shift = b.kb - RB * b.plan.npass;
        UKM_HIP(hipMemsetAsync(b.fh, 0, (MAX_PASSES * RADIX + 1) * sizeof(u64), c->stream));
        u64 *or_all = (key_bits == 64 && attempt == 0) ? b.fh + (size_t)MAX_PASSES * RADIX : nullptr;
        if (first_hist && !or_all && first_shift == shift) {
            UKM_HIP(hipMemcpyAsync(b.fh, first_hist, RADIX * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
            c->sort.stat_fused_hist++;
        } else
            UKM_TRY(launch_first_hist(c, b.keys, b.n, 1, b.fh, or_all, shift));
        if (!or_all) break;
        int bits = 64;
        UKM_TRY(key_width_from_or(c, or_all, &bits));
        if (bits == 64) break;  // the histogram above is the right one
        b.kb = bits;
        if (b.kb < b.plan.min_bits) break;
    }
    return UKM_OK;
}

// Buckets differ in size (canonical k-mers: twice the average at the low end of the code space, none at the top), so
// every bucket goes to the instantiation of ITS size class: the bounds of every bucket, then a tiny kernel that lists the
// buckets of every class, and the few beyond 4096 keys for the general route.  The read-back of its counters also brings
// the previous bucket-route sort's fall-backs from the counting step (the context's device word, created on first use).
int classify(BucketSort &b, u64 **stat) {
    ukm_ctx *c = b.c;
    const int topb = b.plan.topb;
    hipLaunchKernelGGL(ls_bounds_kernel, dim3((b.nbuckets + 1 + 255) / 256), dim3(256), 0, c->stream, b.src(), b.n, b.low_bits(), topb, b.start);
    UKM_TRY(c->sort.stat_word(c->stream, stat));
    static_assert(LS_NCLASS + 3 <= 64, "read-back through the scratch");
    UKM_TRY(ws_alloc_t(c, (size_t)LS_NCLASS + 3, &b.cls));
    UKM_TRY(ws_alloc_t(c, (size_t)LS_NCLASS << topb, &b.ids));
    UKM_TRY(ws_alloc_t(c, (size_t)LS_MAX_BIG, &b.big_ids));
    UKM_TRY(ws_alloc_t(c, (size_t)b.nbuckets + 1, &b.big_size));
    UKM_HIP(hipMemsetAsync(b.cls, 0, (LS_NCLASS + 3) * sizeof(u64), c->stream));
    hipLaunchKernelGGL(ls_classify_kernel, dim3(b.nbuckets / 256), dim3(256), 0, c->stream, b.start, b.cls, b.ids, topb, b.big_ids, b.big_size, *stat);
    UKM_HIP(hipGetLastError());
    return ukm_read_u64(c, b.cls, b.hc, LS_NCLASS + 3);
}

// the bucket kernel of size class k: the instantiations follow LS_CLASS_KPT, entry by entry
template <int K = 0>
void launch_class(int k, bool pairs, dim3 grid, hipStream_t st, const LocalSortArgs &a) {
    if constexpr (K < LS_NCLASS) {
        if (k != K) return launch_class<K + 1>(k, pairs, grid, st, a);
        if (pairs) hipLaunchKernelGGL((ls_sort_kernel<LS_CLASS_KPT[K], true>), grid, dim3(LS_NT), 0, st, a);
        else hipLaunchKernelGGL((ls_sort_kernel<LS_CLASS_KPT[K], false>), grid, dim3(LS_NT), 0, st, a);
    }
}

// One launch per class that occurs.  The launches do not depend on each other and the small ones leave most of the chip
// idle (canonical k-mers: ten classes occur, eight of them 16-60 us each): they go round robin over the call's stream and two
// side streams, largest class first, forked from / joined to the call's stream by events.
int launch_classes(BucketSort &b, u64 *stat, bool counting) {
    ukm_ctx *c = b.c;
    ukm_ctx::SortState &st = c->sort;
    LocalSortArgs a;
    a.src = b.src(); a.vsrc = b.vsrc(); a.keys = b.keys; a.vals = b.vals; a.n = b.n; a.start = b.start; a.low_bits = b.low_bits();
    a.counting = counting ? 1 : 0;
    a.stat = stat;
    int nocc = 0;
    for (int k = 0; k < LS_NCLASS; k++) nocc += b.hc[k] != 0;
    const bool fan = nocc >= 3 && !ukm_env_is(c, "UKM_SORT_FAN", '0');
    if (fan) {
        UKM_TRY(st.side_streams());
        UKM_HIP(hipEventRecord(st.ev_fork, c->stream));
        for (int i = 0; i < 2; i++) UKM_HIP(hipStreamWaitEvent(st.side[i], st.ev_fork, 0));
    }
    int turn = 0;
    hipStream_t lst = c->stream;
    for (int k = LS_NCLASS - 1; k >= 0; k--) {  // (the classes with the most keys per bucket first)
        if (b.hc[k] == 0) continue;
        if (fan) lst = turn % 3 == 0 ? c->stream : st.side[turn % 3 - 1];
        turn++;
        a.ids = b.ids + ((size_t)k << b.plan.topb);
        launch_class(k, b.vals != nullptr, dim3((unsigned)b.hc[k]), lst, a);
    }
    UKM_HIP(hipGetLastError());
    if (fan)
        for (int i = 0; i < 2; i++) {
            UKM_HIP(hipEventRecord(st.ev_side[i], st.side[i]));
            UKM_HIP(hipStreamWaitEvent(c->stream, st.ev_side[i], 0));
        }
    return UKM_OK;
}

// The oversized buckets -- low-complexity k-mers of a real genome crowd a few dozen to a few thousand of them --
// side by side in a scratch array, in bucket order: sorted by the whole key they stay side by side (their top bits
// differ), each one sorted; one general sort instead of one per bucket (48 small sorts took 8 ms).  Where a bucket
// lies in that array is the exclusive scan of the oversized buckets' sizes over the bucket index, so gather and
// scatter are one kernel each, whatever the number of buckets (round 3 read the list back and issued two copies
// per bucket from the host, which is why it gave up beyond 32 of them).
int sort_oversized(BucketSort &b) {
    ukm_ctx *c = b.c;
    const unsigned nb = (unsigned)b.hc[LS_NCLASS];
    const u64 big_keys = b.hc[LS_NCLASS + 1];
    if (c->sort.depth == 1) c->sort.stat_oversized_buckets = nb;
    u64 *big_off = nullptr, *bk = nullptr, *tot = nullptr;
    u32 *bv = nullptr;
    UKM_TRY(ws_alloc_t(c, (size_t)b.nbuckets + 1, &big_off));
    UKM_TRY(ws_alloc_t(c, 1, &tot));
    UKM_TRY(ws_alloc_t(c, big_keys, &bk));
    if (b.vals) UKM_TRY(ws_alloc_t(c, big_keys, &bv));
    UKM_TRY(ukm_dev_exclusive_scan_u64(c, b.big_size, big_off, b.nbuckets, tot));
    const dim3 cg(nb, 16);
    hipLaunchKernelGGL(ls_big_copy_kernel<false>, cg, dim3(256), 0, c->stream, b.big_ids, b.start, big_off, b.src(), b.vsrc(), bk, bv);
    UKM_HIP(hipGetLastError());
    c->sort.general_only = true;  // (crowded by construction: not through this route again)
    const int rc = ukm_dev_sort(c, bk, bv, big_keys, b.kb);
    c->sort.general_only = false;
    UKM_TRY(rc);
    hipLaunchKernelGGL(ls_big_copy_kernel<true>, cg, dim3(256), 0, c->stream, b.big_ids, b.start, big_off, bk, bv, b.keys, b.vals);
    UKM_HIP(hipGetLastError());
    return UKM_OK;
}

// SORT_LOCAL_MIN <= n < 2^32, key_bits >= 32.  *done = false: not this route after all (narrow keys, crowded keys): the
// caller runs the general passes over the keys as they are now (a permutation of the input).  Stable, so taxids may ride along.
int sort_buckets(ukm_ctx *c, u64 *keys, u32 *vals, u64 n, int key_bits, const u64 *first_hist, int first_shift, bool *done) {
    *done = false;
    ukm_ctx::SortState &st = c->sort;
    if (st.depth == 1) st.stat_oversized_buckets = 0;  // (like the route: the chunks' sorts do not overwrite it)
    BucketSort b = {};
    b.c = c; b.keys = keys; b.vals = vals; b.n = n;
    b.plan = bucket_plan(n, key_bits, true, false);
    b.nbuckets = 1u << b.plan.topb;
    UKM_TRY(ws_alloc_t(c, (size_t)MAX_PASSES * RADIX + 1, &b.fh));
    UKM_TRY(ws_alloc_t(c, (size_t)MAX_PASSES * RADIX, &b.gb));
    UKM_TRY(ws_alloc_t(c, (size_t)b.nbuckets + 2, &b.start));
    // skew guard: a context that has met crowded keys looks at a sample before anything else is spent on this route -- at
    // once for a declared width, behind the OR word's read-back for 64
    bool heavy = false;
    if (st.skew_seen && key_bits < 64) {
        if (key_bits < b.plan.min_bits) return UKM_OK;
        UKM_TRY(skew_guard(b, key_bits - b.plan.topb, &heavy));
        if (heavy) return UKM_OK;
    }
    UKM_TRY(first_hist_and_width(b, key_bits, first_hist, first_shift));
    if (b.kb < b.plan.min_bits) return UKM_OK;  // (narrow keys)
    if (st.skew_seen && key_bits == 64) UKM_TRY(skew_guard(b, b.low_bits(), &heavy));
    if (heavy) return UKM_OK;
    int sh[3];  // top passes: the array sorted by its top digits, in place after two of them, in the scratch copy after three
    for (int i = 0; i < b.plan.npass; i++) sh[i] = b.kb - RB * (b.plan.npass - i);
    UKM_TRY(scatter_passes(c, keys, vals, n, b.plan.npass, sh, b.gb, b.fh, &b.tk, &b.tv, &b.in_tmp));
    u64 *stat = nullptr;
    UKM_TRY(classify(b, &stat));
    st.note_fallbacks(b.hc[LS_NCLASS + 2]);
    if (ls_too_crowded(b.hc[LS_NCLASS], b.hc[LS_NCLASS + 1], n)) {
        st.note_skew();  // (and the next sort on this context looks at a sample before it tries)
        if (ukm_env(c, "UKM_SORT_DEBUG")) fprintf(stderr, "[sort] %llu buckets beyond every class: general route\n", (unsigned long long)b.hc[LS_NCLASS]);
        return copy_back(c, keys, vals, b.tk, b.tv, n, b.in_tmp);  // the general passes work on the caller's array
    }
    // counting policy (developer knob UKM_SORT_COUNTING: 0 = digit passes in every bucket, 1 = the counting step whatever earlier sorts met)
    const bool counting = st.want_counting(ukm_env_is(c, "UKM_SORT_COUNTING", '0') ? 0 : ukm_env_is(c, "UKM_SORT_COUNTING", '1') ? 1 : -1);
    u64 classed = 0;
    for (int k = 0; k < LS_NCLASS; k++) classed += b.hc[k];
    st.note_launch(counting, classed);
    UKM_TRY(launch_classes(b, stat, counting));
    if (b.hc[LS_NCLASS]) UKM_TRY(sort_oversized(b));
    *done = true;
    return UKM_OK;
}

// ---- route CHUNKED -------------------------------------------------------------------------------------------------------
// The onesweep tile / status arithmetic is 32-bit: larger inputs are sorted as chunks of 2^31 records
// and combined by the keep-everything 2-way merge (pairwise tree, ping-pong between the input and a
// scratch copy) -- the reference's `sort -m` protocol, in HBM.
int sort_chunked(ukm_ctx *c, u64 *keys, u32 *vals, u64 n, int key_bits) {
    const u64 CH = 1ull << 31;
    const u64 nch = (n + CH - 1) / CH;
    for (u64 i = 0; i < nch; i++) {
        const u64 m = std::min<u64>(CH, n - i * CH);
        WsMark mark = ws_mark(c);
        UKM_TRY(ukm_dev_sort(c, keys + i * CH, vals ? vals + i * CH : nullptr, m, key_bits));
        ws_release(c, mark);
    }
    u64 *tk = nullptr;
    u32 *tv = nullptr;
    UKM_TRY(scratch_pair(c, n, vals != nullptr, &tk, &tv));
    u64 *src_k = keys, *dst_k = tk;
    u32 *src_v = vals, *dst_v = tv;
    for (u64 run = CH; run < n; run *= 2) {  // runs of `run` records are sorted; merge neighbours
        for (u64 lo = 0; lo < n; lo += 2 * run) {
            const u64 na = std::min<u64>(run, n - lo);
            const u64 nb = (lo + run < n) ? std::min<u64>(run, n - lo - run) : 0;
            if (nb == 0) {  // no neighbour: the run moves as it is
                UKM_TRY(copy_back(c, dst_k + lo, vals ? dst_v + lo : nullptr, src_k + lo, vals ? src_v + lo : nullptr, na, true));
                continue;
            }
            u64 nm = 0;
            WsMark mark = ws_mark(c);
            UKM_TRY(ukm_dev_setop2(c, UKM_OP_MERGE_INTERNAL, src_k + lo, vals ? src_v + lo : nullptr, na, src_k + lo + run,
                                   vals ? src_v + lo + run : nullptr, nb, 0, dst_k + lo, vals ? dst_v + lo : nullptr,
                                   na + nb, &nm));
            ws_release(c, mark);
        }
        std::swap(src_k, dst_k);
        std::swap(src_v, dst_v);
    }
    return copy_back(c, keys, vals, src_k, src_v, n, src_k != keys);
}

// ---- route FUSED ---------------------------------------------------------------------------------------------------------
// Large inputs: only the FIRST digit's histogram is built by a pass over the keys; every scatter pass counts
// the next digit on the fly (scatter_passes).  The passes take their tile ids from a ticket counter (no watchdog
// flag to read back), so a sort with a known key width has no host round trip at all; constant
// digits inside the key width are not detected here.  Keys declared 64 bits wide: the OR word drops the passes over
// high digits that are zero everywhere (5-7 passes instead of 8).
int sort_fused(ukm_ctx *c, u64 *keys, u32 *vals, u64 n, int key_bits) {
    u64 *fh = nullptr, *gb = nullptr, *tk = nullptr;
    u32 *tv = nullptr;
    UKM_TRY(ws_alloc_t(c, (size_t)MAX_PASSES * RADIX + 1, &fh));
    UKM_TRY(ws_alloc_t(c, (size_t)MAX_PASSES * RADIX, &gb));
    UKM_HIP(hipMemsetAsync(fh, 0, (MAX_PASSES * RADIX + 1) * sizeof(u64), c->stream));
    u64 *or_all = key_bits == 64 ? fh + (size_t)MAX_PASSES * RADIX : nullptr;
    UKM_TRY(launch_first_hist(c, keys, n, 1, fh, or_all, 0));
    int bits = key_bits;
    if (or_all) UKM_TRY(key_width_from_or(c, or_all, &bits));
    const int npass = (bits + RB - 1) / RB;
    int sh[MAX_PASSES];
    for (int p = 0; p < npass; p++) sh[p] = RB * p;
    bool in_tmp = false;
    UKM_TRY(scatter_passes(c, keys, vals, n, npass, sh, gb, fh, &tk, &tv, &in_tmp));
    return copy_back(c, keys, vals, tk, tv, n, in_tmp);
}

// ---- route HOST_HIST -----------------------------------------------------------------------------------------------------
// Small inputs: the histograms of all digits by one pass over the keys, read back; the host turns them into per-pass digit
// bases and drops the passes whose digit is constant.
int sort_host_hist(ukm_ctx *c, u64 *keys, u32 *vals, u64 n, int key_bits) {
    const int passes = (key_bits + RB - 1) / RB;
    u64 *ghist = nullptr;
    UKM_TRY(ws_alloc_t(c, MAX_PASSES * RADIX, &ghist));
    UKM_HIP(hipMemsetAsync(ghist, 0, MAX_PASSES * RADIX * sizeof(u64), c->stream));
    UKM_TRY(launch_first_hist(c, keys, n, passes, ghist, nullptr, 0));
    std::vector<u64> h((size_t)passes * RADIX);
    UKM_HIP(hipMemcpyAsync(h.data(), ghist, h.size() * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    UKM_HIP(hipStreamSynchronize(c->stream));

    int shifts[MAX_PASSES];
    std::vector<u64> gb;
    int npass = 0;
    for (int p = 0; p < passes; p++) {
        const u64 *hp = &h[(size_t)p * RADIX];
        if (std::find(hp, hp + RADIX, n) != hp + RADIX) continue;  // every key has the same digit: the pass is the identity
        shifts[npass++] = RB * p;
        u64 sum = 0;
        for (int d = 0; d < RADIX; d++) {
            gb.push_back(sum);
            sum += hp[d];
        }
    }
    if (npass == 0) return UKM_OK;

    u64 *gbase_dev = nullptr, *tk = nullptr;
    u32 *tv = nullptr;
    UKM_TRY(ws_alloc_t(c, gb.size(), &gbase_dev));
    UKM_HIP(hipMemcpyAsync(gbase_dev, gb.data(), gb.size() * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    UKM_HIP(hipStreamSynchronize(c->stream));  // gb is a local
    bool in_tmp = false;
    UKM_TRY(scatter_passes(c, keys, vals, n, npass, shifts, gbase_dev, nullptr, &tk, &tv, &in_tmp));
    return copy_back(c, keys, vals, tk, tv, n, in_tmp);
}

}  // namespace

// The shift of the digit whose histogram the bucket route's pre-pass would build for n keys of key_bits bits, or -1 when
// a sort of such keys does not take that route (or reads an OR of all keys first: key_bits = 64).
int ukm_sort_first_shift(const ukm_ctx *c, u64 n, int key_bits) { return sort_first_shift(n, key_bits, sort_local_enabled(c), c->sort.general_only); }

// keys (and vals, may be NULL) are device pointers; sorted in place (stable for pairs)
int ukm_dev_sort(ukm_ctx *c, u64 *keys, u32 *vals, u64 n, int key_bits) { return ukm_dev_sort_hist(c, keys, vals, n, key_bits, nullptr, -1); }

// first_hist (may be null): the 256-bin histogram of digit (key >> first_shift) & 255 over exactly these n keys (see
// first_hist_and_width)
int ukm_dev_sort_hist(ukm_ctx *c, u64 *keys, u32 *vals, u64 n, int key_bits, const u64 *first_hist, int first_shift) {
    if (n < 2) return UKM_OK;
    if (key_bits <= 0 || key_bits > 64) key_bits = 64;
    ukm_ctx::SortState &st = c->sort;
    SortRoute route = sort_route(n, key_bits, sort_local_enabled(c), st.general_only);
    st.depth++;
    int rc = UKM_OK;
    if (route == SortRoute::BUCKETS) {
        bool done = false;
        WsMark mark = ws_mark(c);
        rc = sort_buckets(c, keys, vals, n, key_bits, first_hist, first_shift, &done);
        ws_release(c, mark);
        if (rc == UKM_OK && !done) {  // handed back: the general passes, over the keys as they are now
            st.stat_bucket_declined++;
            route = sort_general_route(n);
        }
    }
    if (rc == UKM_OK && route == SortRoute::CHUNKED) rc = sort_chunked(c, keys, vals, n, key_bits);
    if (rc == UKM_OK && route == SortRoute::FUSED) rc = sort_fused(c, keys, vals, n, key_bits);
    if (rc == UKM_OK && route == SortRoute::HOST_HIST) rc = sort_host_hist(c, keys, vals, n, key_bits);
    st.depth--;
    if (rc == UKM_OK && st.depth == 0) st.stat_route = (u64)route;  // (the chunks' and the gathered buckets' sorts do not overwrite it)
    return rc;
}

extern "C" int ukm_sort_u64(ukm_ctx *ctx, uint64_t *keys, uint64_t n, int key_bits) {
    if (!ctx || (!keys && n)) UKM_FAIL(UKM_ERR_INVALID, "ukm_sort_u64: NULL argument");
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        void *d = nullptr;
        UKM_TRY(ukm_inout(ctx, keys, n * sizeof(u64), &d));
        return ukm_dev_sort(ctx, (u64 *)d, nullptr, n, key_bits);
    }();
    return ukm_finish(&s, rc);
}

extern "C" int ukm_sort_pairs(ukm_ctx *ctx, uint64_t *keys, uint32_t *taxids, uint64_t n, int key_bits) {
    if (!ctx || (!keys && n) || (!taxids && n)) UKM_FAIL(UKM_ERR_INVALID, "ukm_sort_pairs: NULL argument");
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        void *dk = nullptr, *dv = nullptr;
        UKM_TRY(ukm_inout(ctx, keys, n * sizeof(u64), &dk));
        UKM_TRY(ukm_inout(ctx, taxids, n * sizeof(u32), &dv));
        return ukm_dev_sort(ctx, (u64 *)dk, (u32 *)dv, n, key_bits);
    }();
    return ukm_finish(&s, rc);
}
