// ukm_setop_part.h — what every kernel of the 2-way set operation is handed (SetopArgs, the result flags) and the
// merge-path partition: the search helpers, the fine / wave / fused kernels, the verification of a cached table, the match
// counts, and the host's launch_partition.  Part of ukm_setops.hip's translation unit (included there, inside its
// anonymous namespace) and of nothing else.

// FLAG_STALE: the launch ran on a merge-path table taken from the context's partition cache and the verification found a
// boundary that does not hold for the inputs as they are now (setop_partition_verify_kernel): no tile has run
// FLAG_OFFS: the launch took its tiles' output offsets from the cached match counts (TABLE instantiation, below) and a tile
// counted another number of records than its step of the table: the output is void, the pass runs again with the look-back
enum { FLAG_DUP = 1, FLAG_UNSORTED = 2, FLAG_TIMEOUT = 4, FLAG_STALE = 8, FLAG_OFFS = 16 };

struct SetopArgs {
    const u64 *a, *b;
    const u32 *ta, *tb;
    const u32 *ra, *rb;
    u64 na, nb;
    u64 *mp;      // [ntiles + 1]
    u64 *status;  // [ntiles]
    u32 *ticket;
    u64 *result;  // [0] total, [1] flags
    u64 *out;
    u32 *tout;
    u64 out_cap;
    u64 ntiles;
    TaxDev tax;
    u32 flags;
    u32 xcd_order;  // TABLE instantiation only: non-zero = block -> tile by ukm_setop_order.h, 0 = tile = block
    u64 *dbg;  // UKM_PROFILE_PHASES only
    // chained folds (ukm_inter / ukm_diff over many files): |A| is the previous call's result count and stays
    // on the device; na / ntiles above are then upper bounds used for the launch geometry only
    const u64 *na_dev;
    u32 zero_status;  // chained links with few tiles: the partition kernel clears this many status lines (one launch less)
    // Per-FILE taxids (round 5; the .unik header's global taxid, count.go:466-468: the reader hands the same value to the
    // set operation for every record of the file): a stream whose taxid pointer is null carries `cta` / `ctb` in every
    // record.  One such stream beside per-record taxids: the tile loader fills the constant in (no loads).  BOTH streams
    // constant: the plain-key kernel runs (CT instantiation: LDS-DMA staging, 19 items per thread, no taxid in LDS) and the
    // output taxid is one of three values -- A's, B's, or LCA(A's, B's) on a match -- resolved ONCE by setop_ct_kernel into
    // result[4] = lca | keep << 32 (keep: diff -t leaves a matched code in the result, diff.go:404-409).
    u32 cta, ctb;
    // DEFER instantiation (round 6): the pairs a tile does not settle itself -- relatives inside one clade, unknown and merged
    // ids: the root-path reads -- go to the tile's FIX_SLOTS places of this list as (output position, A's taxid, B's taxid) and
    // setop_taxid_fix_kernel settles them behind the launch; fix_cnt[tile] = how many (every tile writes it).  nullptr: none.
    uint4 *fix;
    u32 *fix_cnt;
    // the stale word of the context's partition cache when `mp` is the cached table (ukm_ctx::PartCache), else nullptr.  Non-zero:
    // the table failed its verification -- NO kernel of the launch may take an address from it.
    const u64 *stale;
    // TABLE instantiation only: the exclusive output offset of every tile and, in [ntiles], the total -- written by
    // setop_partition_verify_kernel from the cached match counts for THIS operation (run_setop_pass)
    u64 *base;
};
constexpr u32 FIX_SLOTS = 16;

// (workgroup-uniform: one scalar load, in front of every read of p.mp)
__device__ __forceinline__ bool setop_table_stale(const SetopArgs &p) { return p.stale != nullptr && sload_u64(p.stale) != 0; }

// the actual sizes of a chained call (workgroup-uniform: one scalar load)
__device__ __forceinline__ void setop_resolve_sizes(SetopArgs &p, u64 tile_items) {
    if (p.na_dev) {
        p.na = *p.na_dev;
        p.ntiles = (p.na + p.nb + tile_items - 1) / tile_items;
    }
}

template <bool RANK>
__device__ __forceinline__ bool key_le(u64 ka, u32 ra, u64 kb, u32 rb) {
    if (RANK) return ka < kb || (ka == kb && ra <= rb);
    return ka <= kb;
}
template <bool RANK>
__device__ __forceinline__ bool key_eq(u64 ka, u32 ra, u64 kb, u32 rb) {
    if (RANK) return ka == kb && ra == rb;
    return ka == kb;
}

// ---- the merge-path partition: mp[t] = how many records of A lie in front of tile boundary t (A before B on ties) ----
// With 2.4e5 tiles a 30-step search over the whole inputs per boundary is ~7e6 dependent random reads across 16 GB
// (0.3 ms, TLB-miss bound), so the search is done in two levels: the COARSE level places every PART_COARSE-th boundary
// (and the last one) with a full search, one wave per boundary; the FINE level searches the others only between their
// two coarse neighbours (the path is monotone), i.e. inside a few MB that the group's threads share in cache, one thread
// per boundary.  Small inputs: every boundary by the coarse level's search (single level).  The search itself is written
// once, in the mp_ helpers; the kernels below are index mappings around them.
#ifndef SETOP_PART_COARSE
#define SETOP_PART_COARSE 64
#endif
#ifndef SETOP_PART_INTERP1
#define SETOP_PART_INTERP1 (1 << 17)  // the same for the coarse level (whole-input diagonal): +-1 MB of keys
#endif
#ifndef SETOP_PART_INTERP
#define SETOP_PART_INTERP 512  // half-width of the bracket around the interpolated split (0: plain binary search)
#endif
constexpr int PART_COARSE = SETOP_PART_COARSE;

// diagonal of boundary t and the legal range [lo, hi] of its split
struct MpDiag { u64 diag, lo, hi; };
__device__ __forceinline__ MpDiag mp_diag(const SetopArgs &p, u64 t, int tile_items) {
    const u64 N = p.na + p.nb;
    u64 diag = t * (u64)tile_items;
    if (diag > N) diag = N;
    return {diag, diag > p.nb ? diag - p.nb : 0, diag < p.na ? diag : p.na};
}

// the probe: does A[i] come in front of its partner on the diagonal, B[diag - 1 - i]?  (monotone in i: true, then false)
template <bool RANK>
__device__ __forceinline__ bool mp_le(const SetopArgs &p, u64 diag, u64 i) {
    const u64 j = diag - 1 - i;
    return key_le<RANK>(p.a[i], RANK ? p.ra[i] : 0, p.b[j], RANK ? p.rb[j] : 0);
}

// The path is close to a straight line when the keys are spread evenly (k-mer codes, hashes): two probes W positions
// either side of an interpolated split `est` usually bracket it, and the search that follows stays inside a few KB (the
// probes of a plain binary search over the window each touch another page).  Whatever the probes say narrows [lo, hi]
// correctly, so skewed inputs only lose the two probes.  Needs lo < hi.
template <bool RANK>
__device__ __forceinline__ void mp_bracket(const SetopArgs &p, u64 diag, u64 est, u64 W, u64 &lo, u64 &hi) {
    est = est < lo ? lo : (est > hi ? hi : est);
    const u64 L = est > lo + W ? est - W : lo;
    const u64 R = est + W < hi ? est + W : hi;
    bool pl = true, pr = false;
    if (L > lo) pl = mp_le<RANK>(p, diag, L - 1);
    if (R < hi) pr = mp_le<RANK>(p, diag, R);
    if (L > lo) { if (pl) lo = L; else hi = L - 1; }
    if (R < hi) { if (!pr) hi = R; else lo = R + 1; }  // (R < hi fails when the left probe already cut below R)
}

// one thread: binary search
template <bool RANK>
__device__ __forceinline__ u64 mp_search_thread(const SetopArgs &p, u64 diag, u64 lo, u64 hi) {
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (mp_le<RANK>(p, diag, mid)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One wave: 64-ary search.  Each round the 64 lanes probe 64 split candidates at once (the predicate is monotone along
// the diagonal, so the true lanes form a prefix and a ballot + popcount narrows [lo, hi) to one of 65 sub-ranges): log64
// instead of log2 dependent round trips -- 4-5 instead of 20-30 for the few boundaries of a small input or of the coarse
// level, whose cost is pure latency (measured: the coarse level at 2 x 1e9 40 us, the single-level kernel of a 2 x 1e6
// call 12 us).  [lo, hi] wave-uniform; the split comes back in every lane.
template <bool RANK>
__device__ __forceinline__ u64 mp_search_wave(const SetopArgs &p, u64 diag, u64 lo, u64 hi, int lane) {
    while (lo < hi) {
        const u64 span = hi - lo;
        // candidates: strictly increasing positions in [lo, hi); fewer than 64 when the span is short
        const u64 cand = span <= 64 ? lo + (u64)lane
                                    : lo + (span / 65) * (u64)(lane + 1) + ((span % 65) * (u64)(lane + 1)) / 65;  // = lo + span*(lane+1)/65, no overflow
        const bool active = cand < hi;
        const bool le = active && mp_le<RANK>(p, diag, cand);
        const u64 m_le = __ballot(le), m_act = __ballot(active);
        const int n_true = __popcll(m_le), n_act = __popcll(m_act);  // lanes 0 .. n_true-1 are true (monotone)
        // first false candidate = lane n_true (if active) -> new hi; last true candidate -> new lo
        const u64 c_last_true = __shfl(cand, n_true > 0 ? n_true - 1 : 0, 64);
        const u64 c_first_false = __shfl(cand, n_true < 64 ? n_true : 63, 64);
        const u64 nlo = n_true > 0 ? c_last_true + 1 : lo;
        const u64 nhi = n_true < n_act ? c_first_false : hi;
        lo = nlo;
        hi = nhi;
    }
    return lo;
}

// boundary t over the whole inputs, by one wave (the coarse level; the single level)
template <bool RANK>
__device__ __forceinline__ u64 mp_split_wave(const SetopArgs &p, u64 t, int tile_items, int lane) {
    const MpDiag d = mp_diag(p, t, tile_items);
    u64 lo = d.lo, hi = d.hi;
#if SETOP_PART_INTERP1
    // evenly spread keys: the split of diagonal d lies near d * |A| / (|A| + |B|); the two (wave-uniform) probes cut two or
    // three of the five 64-ary rounds
    if (lo < hi) mp_bracket<RANK>(p, d.diag, (u64)((double)d.diag * ((double)p.na / (double)(p.na + p.nb))), SETOP_PART_INTERP1, lo, hi);
#endif
    return mp_search_wave<RANK>(p, d.diag, lo, hi, lane);
}

// boundary t between its coarse neighbours c0 < t < c1, whose splits are l0 and h0, by one thread (the fine level)
template <bool RANK>
__device__ __forceinline__ u64 mp_split_between(const SetopArgs &p, u64 t, int tile_items, u64 c0, u64 c1, u64 l0, u64 h0) {
    const MpDiag d = mp_diag(p, t, tile_items);
    u64 lo = d.lo > l0 ? d.lo : l0;
    u64 hi = d.hi < h0 ? d.hi : h0;
#if SETOP_PART_INTERP
    if (lo < hi) mp_bracket<RANK>(p, d.diag, l0 + (h0 - l0) * (t - c0) / (c1 - c0), SETOP_PART_INTERP, lo, hi);
#endif
    return mp_search_thread<RANK>(p, d.diag, lo, hi);
}

// The fine level as a kernel of its own (behind the coarse one below), one thread per boundary: a chained link of many
// tiles, and a pass under UKM_SETOP_FUSED_PART=0.
template <bool RANK>
__global__ void setop_partition_fine_kernel(SetopArgs p, int tile_items) {
    setop_resolve_sizes(p, (u64)tile_items);
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p.ntiles || t % PART_COARSE == 0) return;  // (the last boundary too: placed by the coarse level)
    const u64 c0 = t / PART_COARSE * PART_COARSE;
    const u64 c1 = (c0 + PART_COARSE < p.ntiles) ? c0 + PART_COARSE : p.ntiles;
    p.mp[t] = mp_split_between<RANK>(p, t, tile_items, c0, c1, p.mp[c0], p.mp[c1]);
}

// ONE WAVE per boundary.  COARSE: every PART_COARSE-th boundary and the last one; else every boundary (single level), and
// the launch then also clears p.zero_status status lines, 64 per wave (a chained link with few tiles: one launch less).
template <bool RANK, bool COARSE>
__global__ void setop_partition_wave_kernel(SetopArgs p, int tile_items) {
    setop_resolve_sizes(p, (u64)tile_items);
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (!COARSE && gid < p.zero_status) p.status[gid * LB_STRIDE] = 0;
    u64 t = gid >> 6;
    const int lane = (int)(threadIdx.x & 63);
    if (COARSE) {
        t *= PART_COARSE;
        if (t > p.ntiles + PART_COARSE - 1) return;
        if (t > p.ntiles) t = p.ntiles;
    } else if (t > p.ntiles) {
        return;
    }
    const u64 a = mp_split_wave<RANK>(p, t, tile_items, lane);
    if (lane == 0) p.mp[t] = a;
}

// Both levels AND the clearing of the status lines in ONE launch (round 4): a workgroup owns one coarse segment of
// PART_COARSE boundaries.  Waves 0 and 1 place the segment's two coarse ends with the 64-ary search (every coarse end is
// found twice, by its two neighbouring segments: ~10 of them per CU, pure latency), the other boundaries are then searched
// between the two by one thread each, and the segment's status lines (and, by segment 0, the control words) are zeroed on
// the way.  Replaces hipMemsetAsync + the coarse kernel + the fine kernel in front of every tile kernel of a plain
// call: three launches and two dependent kernel tails less (2 x 1e9 codes: 0.19 -> see profiles/r04_notes.md).
template <bool RANK>
__global__ __launch_bounds__(256) void setop_partition_fused_kernel(SetopArgs p, int tile_items, u32 nclear) {
    __shared__ u64 s_end[2];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 c0 = (u64)blockIdx.x * PART_COARSE;
    const u64 c1 = (c0 + PART_COARSE < p.ntiles) ? c0 + PART_COARSE : p.ntiles;
    // status lines of this segment's tiles; the control words in front of them
    if (tid < PART_COARSE && c0 + (u64)tid < p.ntiles) p.status[(c0 + (u64)tid) * LB_STRIDE] = 0;
    if (blockIdx.x == 0 && tid < (int)nclear) p.result[tid] = 0;
    if (blockIdx.x == 0 && tid == 0 && p.stale) *const_cast<u64 *>(p.stale) = 0;  // a fresh table: whatever a verification said about the old one is void
    if (wave < 2) {
        const u64 a = mp_split_wave<RANK>(p, wave == 0 ? c0 : c1, tile_items, lane);
        if (lane == 0) {
            s_end[wave] = a;
            if (wave == 0) p.mp[c0] = a;
            else if (c1 == p.ntiles) p.mp[c1] = a;  // the last boundary has no segment of its own
        }
    }
    __syncthreads();
    const u64 t = c0 + (u64)tid;
    if (tid == 0 || tid >= PART_COARSE || t >= c1) return;
    p.mp[t] = mp_split_between<RANK>(p, t, tile_items, c0, c1, s_end[0], s_end[1]);
}

// The slot's second column (ukm_ctx::PartCache): MP[t] = how many matched pairs have their A record in front of boundary t
// (the merge loop attributes a match to its A step, peeking at B's halo) -- a property of the pair, not of the operation.
// With the diagonal d_t, the split a_t (b_t = d_t - a_t) and s_t = [A[a_t - 1] == B[b_t]] (a matched pair that straddles the
// boundary) the exclusive output offset of tile t is
//     inter: MP[t]      diff: a_t - MP[t]      union: d_t - MP[t] + s_t   (the union drops a pair's B record, in B's tile)
// forwards (setop_partition_verify_kernel) and backwards (setop_counts_record_kernel, from the look-back's prefixes):
__device__ __forceinline__ u64 setop_offset_of(int op, u64 m, u64 a, u64 d, u64 s) {
    return op == UKM_OP_INTER ? m : (op == UKM_OP_DIFF ? a - m : d - m + s);
}
__device__ __forceinline__ u64 setop_matches_of(int op, u64 e, u64 a, u64 d, u64 s) {
    return op == UKM_OP_INTER ? e : (op == UKM_OP_DIFF ? a - e : d + s - e);
}
// A[ia] and B[ib] where the caller's test needs them (`in`).  Both loads are issued whatever `in` says -- clamped, harmless
// indices where the test holds trivially -- so that all keys of a boundary are in flight together.
struct MpKeys { u64 ka, kb; };
__device__ __forceinline__ MpKeys mp_keys(const SetopArgs &p, bool in, u64 ia, u64 ib) { return {p.a[in ? ia : 0], p.b[in ? ib : 0]}; }

// A hit of the partition cache: the table in p.mp was computed by the kernel above for the same (a, b, na, nb, tile_items),
// but the buffers may have been rewritten since.  Searching again costs ~17 dependent round trips; CHECKING costs one:
// the split a of diagonal d (b = d - a) is the merge path's if and only if A[a-1] <= B[b] and B[b-1] < A[a] (A before B on
// ties, as in the searches above; each half holds trivially at an end of its input) -- four keys per boundary, all in
// flight together.  The table may hold anything, so a split is checked against its legal range BEFORE a key is read, and
// against its left neighbour's so that no tile is larger than the LDS it is staged in.  One thread per boundary; thread t
// also clears tile t's status line, block 0 the control words (what the fused kernel does on a miss).  A bad boundary sets
// the cache's stale word -- a word of its own: an OR into the control words would race with their clearing -- and every
// kernel of the launch behind this one returns at its top (setop_table_stale).
//
// `counts` != nullptr: the launch behind this one takes its output offsets from the slot's second column instead of a
// look-back, and p.base[0 .. ntiles] gets this operation's (setop_offset_of; both keys of s_t are loaded for the check
// anyway).  The column may hold anything too: MP[0] = 0 and every step within 0 <= MP[t] - MP[t-1] <= a_t - a_{t-1}, or the
// table is stale -- which leaves 0 <= base[t] <= d_t + 1 for every operation.  The tile kernel then checks every tile's
// count against its step (FLAG_OFFS), so a table that merely belongs to other contents costs a second pass, never a wrong
// result.  No status line is read by that launch: none is cleared.
__global__ __launch_bounds__(256) void setop_partition_verify_kernel(SetopArgs p, int tile_items, u32 nclear, const u64 *counts, int op) {
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < nclear) p.result[threadIdx.x] = 0;
    if (!counts && t < p.ntiles) p.status[t * LB_STRIDE] = 0;
    if (t > p.ntiles) return;
    const MpDiag g = mp_diag(p, t, tile_items);
    const u64 d = g.diag, a = p.mp[t];
    bool good = a >= g.lo && a <= g.hi;
    u64 ap = 0;
    if (good && t > 0) {
        // the tile in front of this boundary: 0 <= its A items <= its items (<= tile_items), which leaves its B items >= 0 too
        const u64 dp = (t - 1) * (u64)tile_items;  // (< N: t <= ntiles)
        ap = p.mp[t - 1];
        good = a >= ap && a - ap <= d - dp;
    }
    u64 m = 0, s = 0;
    if (good && counts) {
        m = counts[t];
        const u64 mprev = t > 0 ? counts[t - 1] : 0;
        good = t > 0 ? (m >= mprev && m - mprev <= a - ap) : m == 0;
    }
    if (good) {
        const u64 b = d - a;  // <= nb by a >= lo
        const bool t1 = a != 0 && b != p.nb, t2 = b != 0 && a != p.na;
        const MpKeys k1 = mp_keys(p, t1, a - 1, b), k2 = mp_keys(p, t2, a, b - 1);
        good = (!t1 || k1.ka <= k1.kb) && (!t2 || k2.kb < k2.ka);
        s = (t1 && k1.ka == k1.kb) ? 1 : 0;
    }
    if (!good) *const_cast<u64 *>(p.stale) = 1;  // (every writer writes the same value)
    else if (counts) p.base[t] = setop_offset_of(op, m, a, d, s);
}

// Behind a plain-key pass that ran WITH the look-back on the slot's table: every status word now holds LB_INCL | the
// inclusive prefix of its tile, i.e. the exclusive offset of the next one.  One thread per boundary turns that into MP[t]
// (setop_matches_of).  The host declares the column valid only after the read-back of this launch shows no flag; until
// then nothing reads it.  (A stale table: no tile has run, nothing to do.)
__global__ __launch_bounds__(256) void setop_counts_record_kernel(SetopArgs p, int tile_items, int op, u64 *counts) {
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    if (t > p.ntiles || setop_table_stale(p)) return;
    u64 m = 0;
    if (t > 0) {
        const u64 d = mp_diag(p, t, tile_items).diag, a = p.mp[t];
        const u64 e = lb_load(&p.status[(t - 1) * LB_STRIDE]) & LB_VAL;
        u64 s = 0;
        if (op == UKM_OP_UNION) {  // (the only operation whose offsets have the straddle term)
            const u64 b = d - a;
            const bool t1 = a != 0 && a <= p.na && b < p.nb;  // (a fresh or verified table: always in range)
            const MpKeys k1 = mp_keys(p, t1, a - 1, b);
            s = (t1 && k1.ka == k1.kb) ? 1 : 0;
        }
        m = setop_matches_of(op, e, a, d, s);
    }
    counts[t] = m;
}

// The partition launch(es) that fill p.mp.  FUSED also zeroes the control block and the status lines (and p.stale's word);
// SINGLE clears p.zero_status status lines; TWO_LEVEL clears nothing.
enum class PartKernels { FUSED, TWO_LEVEL, SINGLE };
template <bool RANK>
void launch_partition_as(hipStream_t st, const SetopArgs &p, int tile_items, PartKernels which) {
    const dim3 wg(256);
    const auto blocks = [](u64 items, u64 per_block) { return dim3((unsigned)((items + per_block - 1) / per_block)); };
    if (which == PartKernels::FUSED) {  // a workgroup per coarse segment
        hipLaunchKernelGGL((setop_partition_fused_kernel<RANK>), blocks(p.ntiles, PART_COARSE), wg, 0, st, p, tile_items, (u32)LbCtl::HEAD);
    } else if (which == PartKernels::TWO_LEVEL) {  // a wave per coarse boundary (four to a workgroup), then a thread per boundary
        hipLaunchKernelGGL((setop_partition_wave_kernel<RANK, true>), blocks(p.ntiles / PART_COARSE + 2, 4), wg, 0, st, p, tile_items);
        hipLaunchKernelGGL((setop_partition_fine_kernel<RANK>), blocks(p.ntiles + 1, 256), wg, 0, st, p, tile_items);
    } else {  // a wave per boundary
        hipLaunchKernelGGL((setop_partition_wave_kernel<RANK, false>), blocks(p.ntiles + 1, 4), wg, 0, st, p, tile_items);
    }
}
int launch_partition(ukm_ctx *c, const SetopArgs &p, u64 tile_items, bool rank, PartKernels which) {
    if (rank) launch_partition_as<true>(c->stream, p, (int)tile_items, which);
    else launch_partition_as<false>(c->stream, p, (int)tile_items, which);
    UKM_HIP(hipGetLastError());
    return UKM_OK;
}
