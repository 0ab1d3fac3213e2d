// ukm_probe_union.hip — `union` of MANY sorted sets that overlap heavily, the shape of an n-file `unikmer union` over
// related genomes (BASELINE config 3: 100 files drawn from one universe).  The reference answers every k-mer of every
// file with one probe of a hash map (union.go:186-208, 225-246); the k-way streaming merge of ukm_kway.hip pays three
// in-LDS merge rounds per input record instead (VALU bound: 119 lane-instructions per record, 34 ms of the 46.7 ms of
// config 3 for level 0 alone) although after the first few files nearly every record is already in the result.
//
// Here the reference's algorithm is laid out for the chip:
//   1. BASE  = k-way union of the first PU_K0 files (ukm_kway.hip): a sorted, duplicate-free set.
//   2. A sample of later records is looked up in BASE (global binary search): when fewer than PU_MIN_HIT of them are
//      found the inputs do not have this shape and the caller's k-way merge answers.
//   3. The VALUE SPACE is cut into ranges of PU_RANGE consecutive BASE entries.  One workgroup per range builds a
//      bucketised table of its entries in LDS (2048 buckets of four, 64 KB) and streams through its slice of EVERY later
//      file (lower-bound cuts of the range limits, one thread per (range, file)): per record one multiplicative hash
//      and one 32-byte bucket read; the order of every file is checked on the way (neighbouring records are compared once).
//      Records that are not in the table — not in BASE — are appended to a miss list (one atomic per 64 slots).
//   4. Result = 2-way union of BASE and sort + unique of the miss list (ukm_sort.hip, ukm_scan.hip, ukm_setops.hip).
// Whatever the data, BASE ∪ later records = BASE ∪ misses, because a hit is an exact 64-bit match; a bad hash or an
// unlucky range only costs probes.  An unsorted file or a full miss list raise a flag and the caller falls back.
// Records WITH TaxIds (round 4, pt_probe_kernel below): every table entry carries the TaxId it came with and the smallest /
// largest pre-order number of the records that differ from it; one table LCA per entry when its range is done.
// Algorithmic bytes: 8 B (12 B with TaxIds) per input record read once (+ the base and miss passes); nothing is written
// per hit.
// The TaxId and counting tables (pt_probe_kernel) also answer `common` below the number of files (ukm_dev_probe_common).
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "ukm_probe.h"

namespace {

__device__ __forceinline__ u32 pu_hash(u64 x) {
    const u32 lo = (u32)x, hi = (u32)(x >> 32);
    return ((lo ^ __builtin_rotateleft32(hi, 15) ^ (hi >> 3)) * 0x9E3779B1u) >> (32 - PU_BUCKET_BITS);
}

// ---- the plain pass (pu2_probe_kernel, round 6; rounds 3-5: pu_probe_kernel) -------------------------------------------------
// What bound pu_probe_kernel (profiles/r03_punion_pmc.txt, r05_notes.md 1c): it had three step shapes (U = 4 / 2 / 1) x two
// validity paths with the list code inlined in each -- 16,000 lines of ISA --, a THIRD load per lane and step for the order
// check (the record behind a lane's pair), 64-bit clamps on every address, 45 scalar instructions per record of slice
// bookkeeping, and four waves per SIMD at 93 registers: 16.5 ms on config 3 (4.5 TB/s).  Here (12.9 ms, 5.7 TB/s; what was
// measured on the way: profiles/r06_notes.md 1):
//   * ONE step shape: 128 records, two per lane, one 16-byte load per lane from a wave-uniform base + a 32-bit lane offset.
//     A slice = one general first step, batches of FULL steps (no validity masks, the batch's loads in flight together,
//     straight-line code: the compiler's s_waitcnt counts are exact), general steps for what is left;
//   * the order check needs no third load: the record in front of a lane's pair is its neighbour's second record (DPP
//     wave_shr:1), lane 0 takes the previous step's last record from a scalar; a slice that does not begin its file starts
//     one record early, so the boundary pair is checked inside lane 0 like every other pair;
//   * 1024 threads share the 64 KB table: two workgroups = eight waves per SIMD (55 registers);
//   * the table in two halves, P pair first (below); the list / claim code exists once, behind one wave-uniform branch.
// (A pipeline ACROSS slices with loads in inline assembly and hand-written waits was built first and measured the same for
//  2 / 3 / 4 steps in flight: latency was not the limit -- and inline-assembly loads hide hazards from the compiler, see the
//  notes.)
#ifndef PU2_NT_N
#define PU2_NT_N 1024
#endif
#ifndef PU2_U_N
#define PU2_U_N 2
#endif
constexpr int PU2_NT = PU2_NT_N;
constexpr int PU2_U = PU2_U_N;  // steps of a batch: their loads are in flight together
constexpr int PU2_WAVES = PU2_NT == 1024 ? 8 : 4;


__global__ __launch_bounds__(PU2_NT) __attribute__((amdgpu_waves_per_eu(PU2_WAVES, PU2_WAVES))) void pu2_probe_kernel(PuArgs a) {
    // the table in two halves: slots 0 and 1 of every bucket in the first 32 KB (P), slots 2 and 3 behind them (Q).  Slots
    // fill in order, so a record is looked up in its bucket's P pair first (one 16-byte read at a 16-byte stride: all bank
    // groups in use) and only the lanes that did not find it there AND see slot 1 taken read the Q pair: a tenth of them.
    __shared__ __attribute__((aligned(32))) u64 s_tab[PU_SLOTS];
    __shared__ u64 s_miss[PU_LMISS];
    auto slot = [&](u32 h, int q) -> u64 * { return &s_tab[(q >> 1) * (PU_SLOTS / 2) + 2 * h + (q & 1)]; };
    __shared__ u32 s_next, s_nmiss, s_nins;
    __shared__ u64 s_flush_at;
    const int tid = (int)threadIdx.x, lane = lane_id();
    const u32 r = blockIdx.x, S1 = a.S1;
    for (int i = tid; i < PU_SLOTS; i += PU2_NT) s_tab[i] = PU_EMPTY;
    if (tid == 0) { s_next = 0; s_nmiss = 0; s_nins = 0; }
    __syncthreads();
    {   // the table of this range's base entries (distinct; an all-ones code can not be told from an empty slot and is left
        // out: records with that code are "misses" and meet their base entry again in the final union)
        const u64 b0 = (u64)r * PU_RANGE;
        const u32 nb = (u32)((a.n0 - b0 < (u64)PU_RANGE) ? (a.n0 - b0) : (u64)PU_RANGE);
        constexpr int PER = (PU_RANGE + PU2_NT - 1) / PU2_NT;
        u64 ent[PER];
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const u32 idx = (u32)tid + (u32)i * PU2_NT;
            ent[i] = a.base[b0 + (idx < nb ? idx : 0)];
            if (idx >= nb) ent[i] = PU_EMPTY;
        }
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const u64 e = ent[i];
            if (e == PU_EMPTY) continue;
            u32 h = pu_hash(e);
            for (bool placed = false; !placed; h = (h + 1) & (PU_BUCKETS - 1)) {
#pragma unroll
                for (int k = 0; k < 4 && !placed; k++) {
                    const u64 old = atomicCAS((unsigned long long *)slot(h, k), (unsigned long long)PU_EMPTY, (unsigned long long)e);
                    placed = old == PU_EMPTY || old == e;
                }
            }
        }
    }
    __syncthreads();
    auto member_from = [&](u64 x, u32 h) -> bool {
        for (;;) {
            const ulonglong2 p = *reinterpret_cast<const ulonglong2 *>(slot(h, 0)), q = *reinterpret_cast<const ulonglong2 *>(slot(h, 2));
            if (p.x == x || p.y == x || q.x == x || q.y == x) return x != PU_EMPTY;
            if (q.y == PU_EMPTY) return false;
            h = (h + 1) & (PU_BUCKETS - 1);
        }
    };
    auto claim = [&](u64 x) -> bool {
        if (x == PU_EMPTY || s_nins >= (u32)PU_RANGE) return true;
        u32 h = pu_hash(x);
        for (;; h = (h + 1) & (PU_BUCKETS - 1)) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const u64 old = atomicCAS((unsigned long long *)slot(h, k), (unsigned long long)PU_EMPTY, (unsigned long long)x);
                if (old == PU_EMPTY) { atomicAdd(&s_nins, 1u); return true; }
                if (old == x) return false;
            }
        }
    };
    const u64 lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    u64 chunk_at = 0, fill = 0;  // wave-uniform
    u32 chunk_cap = 0, chunk_used = 0;
    auto close_chunk = [&]() {
        if ((u32)lane < chunk_cap - chunk_used) a.miss[chunk_at + chunk_used + (u32)lane] = fill;
        chunk_cap = chunk_used = 0;
    };
    auto append_global = [&](bool m, u64 x) {
        const u64 mask = __ballot(m);
        if (mask == 0ull) return;
        const u32 n = (u32)__popcll(mask);
        const int lead = __ffsll((long long)mask) - 1;
        if (n > chunk_cap - chunk_used) {
            close_chunk();
            const u32 want = n > PU_CHUNK ? 64u : PU_CHUNK;
            u64 at = 0;
            if (lane == lead) at = atomicAdd((unsigned long long *)&a.ctl[0], (unsigned long long)want);
            at = __shfl(at, lead, 64);
            if (at + want > a.miss_cap) {
                if (lane == lead) atomicOr((unsigned long long *)&a.ctl[1], (unsigned long long)PU_FLAG_OVERFLOW);
                return;
            }
            chunk_at = at;
            chunk_cap = want;
        }
        fill = __shfl(x, lead, 64);
        if (m) a.miss[chunk_at + chunk_used + (u32)__popcll(mask & lt)] = x;
        chunk_used += n;
    };
    // (the one copy of the list code: both records of a step go through it in a loop that is NOT unrolled)
    auto append2 = [&](bool m0, u64 x0, bool m1, u64 x1) {
#pragma nounroll
        for (int h = 0; h < 2; h++) {
            const bool missing = h ? m1 : m0;
            const u64 x = h ? x1 : x0;
            if (__ballot(missing) == 0ull) continue;
            const bool m = missing && claim(x);
            const u64 mask = __ballot(m);
            if (mask == 0ull) continue;
            const int lead = __ffsll((long long)mask) - 1;
            u32 at = 0;
            if (lane == lead) at = atomicAdd(&s_nmiss, (u32)__popcll(mask));
            at = (u32)__shfl((int)at, lead, 64) + (u32)__popcll(mask & lt);
            const bool in_lds = m && at < (u32)PU_LMISS;
            if (in_lds) s_miss[at] = x;
            append_global(m && !in_lds, x);
        }
    };
    // ---- slices -> batches of PU2_U steps ----
    // A step = up to 128 records [lo, hi) of the 128 at `ptr` (two per lane: 2 l and 2 l + 1; lanes whose pair lies beyond
    // hi - 2 re-read the last pair that fits: duplicates of real records, harmless to the table and masked out of the order
    // check).  A slice that does not begin its file starts ONE RECORD EARLY with lo = 1: the pair (f[beg - 1], f[beg]) is
    // then checked inside lane 0 like every other pair -- no separate load for the record in front of the slice -- and a
    // last step of ONE record is moved back by one record the same way, so every load is a 16-byte pair inside the file
    // (files of fewer than two records never come here: the host lists their record itself).  The loads of a batch are
    // issued together and UNCONDITIONALLY (a step behind the slice's end re-reads the batch's first pair): straight-line
    // code, so the compiler's own s_waitcnt counts are exact; the scalar work per step is a handful of instructions.
    auto take = [&]() -> u32 {
        u32 j = 0;
        if (lane == 0) j = atomicAdd(&s_next, 1u);
        return (u32)__builtin_amdgcn_readfirstlane((int)j);
    };
    struct Meta { u64 beg, end, f; };
    auto fetch = [&](u32 j) -> Meta {
        Meta m = {0, 0, 0};
        if (j < S1) {
            m.beg = sload_u64(&a.cuts[(u64)r * S1 + j]);
            m.end = sload_u64(&a.cuts[(u64)(r + 1) * S1 + j]);
            m.f = sload_u64((const u64 *)&a.files[j]);
        }
        return m;
    };
    bool bad = false, raw = false;
    const u32 l2 = 2u * (u32)lane;
    u64 run_carry = 0;
    // FULL: all 128 records of the step are the slice's (lo = 0, hi = 128): no validity masks
    auto consume = [&](auto FULL, const pu_pair &pr, u32 lo, u32 hi) {
        constexpr bool full = decltype(FULL)::value;
        const u64 x0 = pr.x, x1 = pr.y;
        const u32 pmax = hi > 2u ? hi - 2u : 0u;
        const u64 prev = pu2_shr1(x1, run_carry);
        if (full) bad |= prev > x0 || x0 > x1;
        else bad |= (prev > x0 && l2 <= pmax) || x0 > x1;
        run_carry = ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(x1 >> 32), 63) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)x1, 63);
        const u32 h0 = pu_hash(x0), h1 = pu_hash(x1);
        const ulonglong2 p0 = *reinterpret_cast<const ulonglong2 *>(slot(h0, 0)), p1 = *reinterpret_cast<const ulonglong2 *>(slot(h1, 0));
        bool ha = p0.x == x0 || p0.y == x0, hb = p1.x == x1 || p1.y == x1;
        // ONE masked region for the lanes of which either record has to look at slots 2 and 3 (a tenth of the records)
        if ((!ha && p0.y != PU_EMPTY) || (!hb && p1.y != PU_EMPTY)) {
            const ulonglong2 q0 = *reinterpret_cast<const ulonglong2 *>(slot(h0, 2)), q1 = *reinterpret_cast<const ulonglong2 *>(slot(h1, 2));
            ha = ha || q0.x == x0 || q0.y == x0;
            hb = hb || q1.x == x1 || q1.y == x1;
            // a full bucket (0.4 %): the slow way
            if (!ha && q0.y != PU_EMPTY) ha = member_from(x0, (h0 + 1) & (PU_BUCKETS - 1));
            if (!hb && q1.y != PU_EMPTY) hb = member_from(x1, (h1 + 1) & (PU_BUCKETS - 1));
        }
        ha = ha && x0 != PU_EMPTY;  // (an all-ones record would "match" an empty slot)
        hb = hb && x1 != PU_EMPTY;
        bool m0 = !ha, m1 = !hb;
        if (!full) {
            const u32 i0 = l2 < pmax ? l2 : pmax;  // the records this lane holds: i0, i0 + 1
            m0 = m0 && i0 - lo < hi - lo;
            m1 = m1 && i0 + 1u - lo < hi - lo;
        }
        if (__ballot(m0 || m1)) append2(m0, x0, m1, x1);
    };
    u32 g_j = take();          // the next slice; its cut points and pointer are already on their way
    Meta g_m = fetch(g_j);
    u64 ptr = 0;
    u32 rem = 0;
    // one step that is not (known to be) full: the first step of a slice, and what is left behind its full steps
    auto general_step = [&](u32 lo, bool first) {
        const u32 cnt = rem < 128u ? rem : 128u;
        // one record: at the start of its file the pair (0, 1) -- the file has two records --, else the pair (-1, 0)
        const u32 back = (cnt == 1u && !first) ? 1u : 0u;
        const u32 slo = back ? 1u : lo, shi = cnt + back;
        const u32 pmax = shi > 2u ? shi - 2u : 0u;
        // (offsets from ptr - 8, so that the moved-back pair has a non-negative one)
        const u32 voff = 8u - 8u * back + 8u * (l2 < pmax ? l2 : pmax);
        const pu_pair pr = *(const pu_pair __attribute__((address_space(1))) *)((const char __attribute__((address_space(1))) *)(uintptr_t)(ptr - 8) + voff);
        consume(std::false_type{}, pr, slo, shi);
        rem -= cnt;
        ptr += 1024;
    };
    const u32 voff_full = 16u * (u32)lane;
    while (g_j < S1) {
        const Meta m = g_m;
        g_j = take();
        g_m = fetch(g_j);
        const u64 n = m.end > m.beg ? m.end - m.beg : 0ull;
        if (n == 0) continue;
        if (n >= 0xFFFFFF00ull) { raw = true; continue; }  // (a slice of 2^32 records: the caller's other routes)
        const u32 lo = m.beg ? 1u : 0u;                    // 1: the first loaded record lies in front of the slice
        ptr = m.f + 8ull * (m.beg - lo);
        rem = (u32)n + lo;
        run_carry = 0;
        general_step(lo, true);
        while (rem >= 128u * PU2_U) {                      // batches of full steps: their loads are in flight together
            pu_pair pr[PU2_U];
#pragma unroll
            for (int u = 0; u < PU2_U; u++)
                pr[u] = *(const pu_pair __attribute__((address_space(1))) *)((const char __attribute__((address_space(1))) *)(uintptr_t)ptr + (voff_full + 1024u * (u32)u));
#pragma unroll
            for (int u = 0; u < PU2_U; u++) consume(std::true_type{}, pr[u], 0u, 128u);
            rem -= 128u * PU2_U;
            ptr += 1024ull * PU2_U;
        }
        while (rem) general_step(0u, false);
    }
    if (raw && lane == 0) atomicOr((unsigned long long *)&a.ctl[1], (unsigned long long)PU_FLAG_OVERFLOW);
    close_chunk();
    if (bad) atomicOr((unsigned long long *)&a.ctl[1], (unsigned long long)PU_FLAG_UNSORTED);
    __syncthreads();
    const u32 nl = s_nmiss < (u32)PU_LMISS ? s_nmiss : (u32)PU_LMISS;
    if (nl == 0) return;
    if (tid == 0) {
        const u64 at = atomicAdd((unsigned long long *)&a.ctl[0], (unsigned long long)nl);
        if (at + nl > a.miss_cap) atomicOr((unsigned long long *)&a.ctl[1], (unsigned long long)PU_FLAG_OVERFLOW);
        s_flush_at = at;
    }
    __syncthreads();
    const u64 at = s_flush_at;
    if (at + nl <= a.miss_cap)
        for (u32 i = (u32)tid; i < nl; i += PU2_NT) a.miss[at + i] = s_miss[i];
}

// ---- the same pass over records WITH TaxIds (union.go:195-201: the TaxId of a code is the LCA over all its records) ----
// Beside every table slot one 16-byte word of LDS: the TaxId the entry came with (t0: the base files' fold, or the first
// record of a new code), the smallest pre-order number (TaxDev::euler) among its records, the COMPLEMENT of the largest
// (so that widening the interval at either end is the same instruction, an atomic minimum, on one of two words), and a
// flag for the one case the interval cannot show: a record with another TaxId but the same number as everything so far
// (an alias of a merged id; two different unknown ids).  A hit is one more LDS read and — only while it still widens the
// interval — one LDS atomic; the LCA of a set of nodes is the LCA of its members with the smallest and the largest
// number, so ONE table LCA per entry at the end equals the reference's left fold (the contract of lca_dev: 0 / unknown
// ids absorb unless every TaxId is the same).
// New codes are claimed in the table as in the plain pass and leave WITH their fold when the range is done; what
// cannot be claimed (all-ones codes, a table that has doubled) is listed record by record and folded by the final
// sort + unique + 2-way union.  The three words of a slot sit in ONE 16-byte LDS word (a hit reads them with one
// ds_read_b128 beside the two of its bucket): 24 bytes per slot, 1536 buckets of four (144 KB), one workgroup of 1024
// threads per CU (768 buckets and two workgroups of 512 measured the same probe time; the larger range halves the cut
// points and the per-slice steps: 31.0 -> 29.9 ms on config 3's shape at half size).
#ifndef PT_BUCKETS_N
#define PT_BUCKETS_N 1536
#endif
#ifndef PT_NT_N
#define PT_NT_N 1024
#endif
constexpr int PT_NT = PT_NT_N;
constexpr int PT_WAVES = PT_NT == 1024 ? 4 : PU_WAVES;
constexpr int PT_BUCKETS = PT_BUCKETS_N;
constexpr int PT_SLOTS = 4 * PT_BUCKETS;
constexpr int PT_RANGE = PT_BUCKETS;
constexpr int PT_K0 = 4;               // files merged into the base set
constexpr u32 PT_UNSET = 0xFFFFFFFFu;  // t0 of a slot: nobody has set it yet

__device__ __forceinline__ u32 pt_hash(u64 x) {
    const u32 lo = (u32)x, hi = (u32)(x >> 32);
    return (u32)(((u64)((lo ^ __builtin_rotateleft32(hi, 15) ^ (hi >> 3)) * 0x9E3779B1u) * (u64)PT_BUCKETS) >> 32);
}

typedef u32 pt_u32x2 __attribute__((ext_vector_type(2)));
typedef pt_u32x2 __attribute__((aligned(4))) pt_tpair;  // 8 bytes at 4-byte alignment

// COUNT = `common` (common.go:220-344) through the same tables: BASE is the first file (every code once: common.go:232,244),
// every slot also counts its records ([31:2] of the flag word), and when the range is done the codes that reached the
// threshold leave — base entries and new codes alike — with their fold; nothing is listed record by record (a record that
// cannot be counted in a table raises PU_FLAG_RAW and the caller's counting merge answers).
template <bool COUNT, bool CM = false>
__global__ __launch_bounds__(PT_NT) __attribute__((amdgpu_waves_per_eu(PT_WAVES, PT_WAVES))) void pt_probe_kernel(PuArgs a) {
    __shared__ __attribute__((aligned(32))) u64 s_tab[PT_SLOTS];
    // x = t0, y = smallest number, z = ~largest, w = [0] another TaxId with the same number was seen, [1] settled, [31:2] records (COUNT)
    __shared__ __attribute__((aligned(16))) uint4 s_st[PT_SLOTS];
    __shared__ u32 s_next, s_nins;
    __shared__ u32 s_scan[PT_NT / 64 + 1];
    __shared__ u64 s_flush_at;
    const int tid = (int)threadIdx.x, lane = lane_id();
    const u32 r = blockIdx.x, S1 = a.S1;
    const TaxDev &T = a.tax;
    for (int i = tid; i < PT_SLOTS; i += PT_NT) {
        s_tab[i] = PU_EMPTY;
        s_st[i] = make_uint4(PT_UNSET, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u);  // (an empty interval)
    }
    if (tid == 0) { s_next = 0; s_nins = 0; }
    __syncthreads();
    auto next_bucket = [](u32 h) -> u32 { return h + 1 == (u32)PT_BUCKETS ? 0u : h + 1; };
    // first free slot of the first bucket of the probe sequence that is not full, or the slot that already holds x
    auto insert = [&](u64 x, bool &fresh) -> int {
        u32 h = pt_hash(x);
        for (;; h = next_bucket(h)) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const u64 old = atomicCAS((unsigned long long *)&s_tab[4 * h + k], (unsigned long long)PU_EMPTY, (unsigned long long)x);
                if (old == PU_EMPTY || old == x) {
                    fresh = old == PU_EMPTY;
                    return (int)(4 * h + k);
                }
            }
        }
    };
    const u64 b0 = (u64)r * a.range;  // (a.range <= PT_RANGE: pt_range_for)
    const u32 nb = (u32)((a.n0 - b0 < (u64)a.range) ? (a.n0 - b0) : (u64)a.range);
    constexpr int PER = (PT_RANGE + PT_NT - 1) / PT_NT;
    u64 ent[PER];
    u32 et[PER];
    bool bad = false, bad_t = false, bad_raw = false;  // an unsorted file; a TaxId of 2^32 - 1 (the table's own "not set"); COUNT: a record no table could count
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const u32 idx = (u32)tid + (u32)i * PT_NT;
        ent[i] = a.base[b0 + (idx < nb ? idx : 0)];
        et[i] = a.base_tax ? a.base_tax[b0 + (idx < nb ? idx : 0)] : a.base_ct;  // (no array: COUNT only -- plain codes, or the first file's one taxid)
        if (idx >= nb) ent[i] = PU_EMPTY;
        else bad_t |= et[i] == PT_UNSET;
    }
    // Clade mode (PuArgs::clade_mode, round 5): a number is `clade code << 24 | pre-order number` -- codes are handed out in
    // pre-order, so the composite orders taxids as the numbers do -- and a record of a file with per-record taxids brings only
    // the code (one byte of a table that stays in L2, instead of 4 bytes of one that does not): see fold.
    constexpr bool cm = CM;  // (an instantiation of its own: the plain fold keeps its instruction count)
    u32 ee[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const u32 tq = et[i] < T.size ? et[i] : 0u;
        ee[i] = T.euler ? T.euler[tq] : 0u;
        if (cm && ee[i]) ee[i] |= (u32)T.clade8[tq] << 24;
    }
#pragma unroll
    for (int i = 0; i < PER; i++) {
        if (ent[i] == PU_EMPTY) continue;  // (an all-ones code: its records are listed, the final union folds them)
        bool fresh;
        const int slot = insert(ent[i], fresh);
        s_st[slot] = make_uint4(et[i], ee[i], ~ee[i], COUNT ? 4u * a.count0 : 0u);
    }
    __syncthreads();
    auto find_from = [&](u64 x, u32 h) -> int {
        for (;;) {
            const ulonglong2 *b = reinterpret_cast<const ulonglong2 *>(&s_tab[4 * h]);
            const ulonglong2 p = b[0], q = b[1];
            const int k = p.x == x ? 0 : (p.y == x ? 1 : (q.x == x ? 2 : (q.y == x ? 3 : -1)));
            if (k >= 0) return x != PU_EMPTY ? (int)(4 * h) + k : -1;
            if (q.y == PU_EMPTY) return -1;
            h = next_bucket(h);
        }
    };
    auto find2 = [&](u64 xa, u64 xb, int &sa, int &sb) {
        const u32 h0 = pt_hash(xa), h1 = pt_hash(xb);
        const ulonglong2 *b0p = reinterpret_cast<const ulonglong2 *>(&s_tab[4 * h0]);
        const ulonglong2 *b1p = reinterpret_cast<const ulonglong2 *>(&s_tab[4 * h1]);
        const ulonglong2 p0 = b0p[0], q0 = b0p[1], p1 = b1p[0], q1 = b1p[1];
        const int k0 = p0.x == xa ? 0 : (p0.y == xa ? 1 : (q0.x == xa ? 2 : (q0.y == xa ? 3 : -1)));
        const int k1 = p1.x == xb ? 0 : (p1.y == xb ? 1 : (q1.x == xb ? 2 : (q1.y == xb ? 3 : -1)));
        sa = (k0 >= 0 && xa != PU_EMPTY) ? (int)(4 * h0) + k0 : -1;
        sb = (k1 >= 0 && xb != PU_EMPTY) ? (int)(4 * h1) + k1 : -1;
        if (k0 < 0 && q0.y != PU_EMPTY) sa = find_from(xa, next_bucket(h0));
        if (k1 < 0 && q1.y != PU_EMPTY) sb = find_from(xb, next_bucket(h1));
    };
    // one record's TaxId into its entry; e = its pre-order number (0: taxid 0 / unknown)
    // Clade mode: e = code << 24 | number when `exact`, else code << 24 (the number was not read).  An entry whose interval
    // spans two clades has the LCA of those two clade nodes whatever the exact numbers are, so a record needs its number
    // only while the entry's interval lies inside ONE clade and the record is of that clade (or the interval is not written
    // yet): then -- for unrelated taxa next to never -- it is fetched here; a record outside the interval widens it with a
    // sentinel number (all ones below / zero above the code), one inside an interval of several clades does nothing.  The
    // interval only ever widens, so an entry that is still inside one clade at the end had every record folded exactly.
    auto fold = [&](int slot, u32 t, u32 e, bool exact) {
        uint4 st = s_st[slot];
        if (st.x == PT_UNSET) {  // a new code: whoever comes first gives it its TaxId (any order gives the same fold)
            const u32 old = atomicCAS(&s_st[slot].x, PT_UNSET, t);
            if (old == PT_UNSET) {
                if (cm && !exact && e != 0) e |= T.euler[t];  // (the claimer's own number: e != 0 says t is inside the table)
                atomicMin(&s_st[slot].y, e);
                atomicMin(&s_st[slot].z, ~e);
                return;
            }
            st = s_st[slot];
        }
        if (t == st.x) return;
        u32 e_lo = e, e_hi = e;  // what the record puts to the interval's two ends
        if (cm && !exact && e != 0) {
            const u32 c = e >> 24;
            if (st.y > ~st.z || ((st.y >> 24) == c && ((~st.z) >> 24) == c)) {
                e |= T.euler[t];
                e_lo = e_hi = e;
                exact = true;
            } else {
                e_lo = e | 0xFFFFFFu;
            }
        }
        const bool lo = e_lo < st.y, hi = ~e_hi < st.z;
        if (lo | hi) {
            atomicMin(lo ? &s_st[slot].y : &s_st[slot].z, lo ? e_lo : ~e_hi);
            if (lo & hi) atomicMin(&s_st[slot].z, ~e_hi);  // (an interval that is still empty: a new code a moment after its claim)
            // The snapshot was taken between the claimer's CAS on x and its two minima (empty or half-written interval:
            // smallest > largest): this record's number may be the CLAIMER'S -- the alias of a merged id, another unknown
            // id -- and the interval would then never show that two different taxids met.  Say so; a flag too many only
            // sends settle() through LCA(node_at[min], node_at[max]), which is always right.  (Base entries are written
            // in front of the barrier and are never seen half-way.)
            if (st.y > ~st.z && (st.w & 1u) == 0u) atomicOr(&s_st[slot].w, 1u);
        } else if ((!cm || exact || e == 0) && st.y == e && st.z == ~e && (st.w & 1u) == 0u) {
            atomicOr(&s_st[slot].w, 1u);
        }
    };
    const u64 lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    u64 chunk_at = 0, fill = 0;  // wave-uniform
    u32 fill_t = 0;
    u32 chunk_cap = 0, chunk_used = 0;
    auto close_chunk = [&]() {
        if ((u32)lane < chunk_cap - chunk_used) {
            a.miss[chunk_at + chunk_used + (u32)lane] = fill;
            if (a.miss_tax) a.miss_tax[chunk_at + chunk_used + (u32)lane] = fill_t;
        }
        chunk_cap = chunk_used = 0;
    };
    auto append_global = [&](bool m, u64 x, u32 t) {
        const u64 mask = __ballot(m);
        if (mask == 0ull) return;
        const u32 n = (u32)__popcll(mask);
        const int lead = __ffsll((long long)mask) - 1;
        if (n > chunk_cap - chunk_used) {
            close_chunk();
            const u32 want = n > PU_CHUNK ? 64u : PU_CHUNK;
            u64 at = 0;
            if (lane == lead) at = atomicAdd((unsigned long long *)&a.ctl[0], (unsigned long long)want);
            at = __shfl(at, lead, 64);
            if (at + want > a.miss_cap) {
                if (lane == lead) atomicOr((unsigned long long *)&a.ctl[1], (unsigned long long)PU_FLAG_OVERFLOW);
                return;  // (the host discards everything)
            }
            chunk_at = at;
            chunk_cap = want;
        }
        fill = __shfl(x, lead, 64);
        fill_t = (u32)__shfl((int)t, lead, 64);
        if (m) {
            const u64 at = chunk_at + chunk_used + (u32)__popcll(mask & lt);
            a.miss[at] = x;
            if (a.miss_tax) a.miss_tax[at] = t;
        }
        chunk_used += n;
    };
    // a record: found -> fold; not found -> claim a slot for its code (then it is a hit like any other), or list it
    // (plain codes -- no file has TaxIds -- through these tables: a hit has nothing to do beyond the count)
    const bool folds = a.base_tax != nullptr || a.miss_tax != nullptr;
    auto record = [&](bool valid, int slot, u64 x, u32 t, u32 e, bool exact) {
        bool raw = false;
        if (valid) {
            if (slot < 0) {
                if (x == PU_EMPTY || s_nins >= (u32)PT_RANGE) raw = true;
                else {
                    bool fresh;
                    slot = insert(x, fresh);
                    if (fresh) atomicAdd(&s_nins, 1u);
                }
            }
            if (!raw) {
                if (COUNT) atomicAdd(&s_st[slot].w, 4u);
                if (folds) fold(slot, t, e, exact);
            }
        }
        if (COUNT) bad_raw |= raw;
        else append_global(raw, x, t);
    };
    // The lanes stream a slice 128 records per step.  A step is three things that each wait for the one before: the loads
    // of codes and TaxIds (A), the pre-order numbers of those TaxIds (B: a second round trip), the probes (C).  Slices are
    // short here (a range of 1536 entries: several hundred records per file), so a wave that did A, B, C one after the other
    // spent its time waiting twice per step (24 ms on config 3's shape at half size).  The steps of ALL slices of the wave
    // form one sequence instead and run as a pipeline: A of step i + 2 and B of step i + 1 are issued before C of step i.
#ifndef PT_U
#define PT_U 1     /* 16-byte loads per lane and step (2: 31.0 ms on config 3's shape at half size with one taxid per file, 1: 29.5; without the pipeline 2: 33.6, 4: 31.9; one stage deeper 1: 29.9, 2: 34.2) */
#endif
    constexpr int U = PT_U;
    struct Desc { u64 f, tf, p0, end, len; u32 ct, ce; bool valid; };  // wave-uniform (ct, ce: the file's own taxid and its number when tf == 0)
    struct RegA { pu_pair pr[U]; pt_tpair tp[U]; u64 nx[U]; };
    struct RegB { u32 eu[U][2]; };
    auto issue_a = [&](const Desc &d, RegA &ra) {
        if (!d.valid) return;
        const auto f = as_global((const u64 *)(uintptr_t)d.f);
        const bool has_t = d.tf != 0;
        const auto tf = as_global((const u32 *)(uintptr_t)(has_t ? d.tf : d.f));
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u64 pos = d.p0 + (u64)u * 128 + 2u * (u32)lane;
            const u64 q = pos < d.len - 2 ? pos : d.len - 2;
            const u64 q2 = pos + 2 < d.len ? pos + 2 : d.len - 1;
            ra.pr[u] = *(const pu_pair __attribute__((address_space(1))) *)(f + q);
            ra.nx[u] = f[q2];
            ra.tp[u] = pt_tpair{d.ct, d.ct};
            if (has_t) ra.tp[u] = *(const pt_tpair __attribute__((address_space(1))) *)(tf + q);  // (wave-uniform branch)
        }
    };
    auto issue_b = [&](const Desc &d, const RegA &ra, RegB &rb) {
        if (!d.valid) return;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u32 ta = ra.tp[u].x, tb = ra.tp[u].y;
            bad_t |= ta == PT_UNSET || tb == PT_UNSET;
            rb.eu[u][0] = rb.eu[u][1] = d.ce;
            if (d.tf != 0) {  // (wave-uniform; a file without per-record TaxIds: its own one's number -- 0 without any, and there may be no taxonomy at all)
                if (cm) {     // the clade codes alone (fold fetches a number where it matters)
                    rb.eu[u][0] = (u32)T.clade8[ta < T.size ? ta : 0u] << 24;
                    rb.eu[u][1] = (u32)T.clade8[tb < T.size ? tb : 0u] << 24;
                } else {
                    rb.eu[u][0] = T.euler[ta < T.size ? ta : 0u];
                    rb.eu[u][1] = T.euler[tb < T.size ? tb : 0u];
                }
            }
        }
    };
    auto process = [&](const Desc &d, const RegA &ra, const RegB &rb) {
        const u64 p0 = d.p0, end = d.end, len = d.len;
        if (p0 + (u64)U * 128 + 2 <= len) {
            // every lane read two records of the file and the record behind them (wave-uniform test): the order check
            // needs no validity logic (what lies behind the slice's end is still the file), the probes only `pos < end`
#pragma unroll
            for (int u = 0; u < U; u++) {
                const u64 pos = p0 + (u64)u * 128 + 2u * (u32)lane;
                const u64 x0 = ra.pr[u].x, x1 = ra.pr[u].y;
                bad |= x0 > x1 || x1 > ra.nx[u];
                int s0, s1;
                find2(x0, x1, s0, s1);
                record(pos < end, s0, x0, ra.tp[u].x, rb.eu[u][0], d.tf == 0);
                record(pos + 1 < end, s1, x1, ra.tp[u].y, rb.eu[u][1], d.tf == 0);  // (a code claimed a moment ago is found again by the insert)
            }
            return;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u64 pos = p0 + (u64)u * 128 + 2u * (u32)lane;
            const u32 nv = pos + 1 < end ? 2u : (pos < end ? 1u : 0u);
            const bool shifted = pos > len - 2;  // pos = len - 1 (or beyond: nv = 0): the record is the pair's second
            const u64 x0 = shifted ? ra.pr[u].y : ra.pr[u].x;
            const u32 y0 = shifted ? ra.tp[u].y : ra.tp[u].x, e0 = shifted ? rb.eu[u][1] : rb.eu[u][0];
            const u64 x1 = nv == 2 ? ra.pr[u].y : x0;
            // the record behind the last valid one (order check, also across slices); all ones behind the file
            const u64 x2 = nv == 2 ? (pos + 2 < len ? ra.nx[u] : PU_EMPTY) : ((!shifted && pos + 1 < len) ? ra.pr[u].y : PU_EMPTY);
            const bool v0 = nv >= 1, v1 = nv == 2;
            if (v0) bad |= x0 > x1 || x1 > x2;
            int s0, s1;
            find2(x0, x1, s0, s1);
            record(v0, s0, x0, y0, e0, d.tf == 0);
            record(v1, s1, x1, ra.tp[u].y, rb.eu[u][1], d.tf == 0);
        }
    };
    auto take = [&]() -> u32 {
        u32 j = 0;
        if (lane == 0) j = atomicAdd(&s_next, 1u);
        return (u32)__builtin_amdgcn_readfirstlane((int)j);
    };
    struct Meta { u64 beg, end, len, f, tf, cte; };
    auto fetch = [&](u32 j) -> Meta {
        Meta m = {0, 0, 0, 0, 0, 0};
        if (j < S1) {
            m.beg = sload_u64(&a.cuts[(u64)r * S1 + j]);
            m.end = sload_u64(&a.cuts[(u64)(r + 1) * S1 + j]);
            m.len = sload_u64(&a.lens[j]);
            m.f = sload_u64((const u64 *)&a.files[j]);
            m.tf = sload_u64((const u64 *)&a.tfiles[j]);
            if (a.cte) m.cte = sload_u64(&a.cte[j]);
        }
        return m;
    };
    // the wave's sequence of steps: slices are taken from the workgroup's counter, the cut points of the slice after
    // the current one are already on their way
    u32 j = take();
    Meta cur = fetch(j);
    u32 jn = take();
    Meta nxt = fetch(jn);
    u64 pos = cur.beg;
    auto next_desc = [&]() -> Desc {
        for (;;) {
            if (j >= S1) return Desc{0, 0, 0, 0, 0, 0u, 0u, false};
            const u64 end = cur.end < cur.beg ? cur.beg : cur.end;
            const u32 fct = cur.tf ? 0u : (u32)cur.cte, fce = cur.tf ? 0u : (u32)(cur.cte >> 32);
            if (cur.len >= 2 && pos < end) {
                const Desc d = {cur.f, cur.tf, pos, end, cur.len, fct, fce, true};
                pos += (u64)U * 128;
                return d;
            }
            if (cur.len < 2 && end > cur.beg) {  // a one-record file (no 16-byte load fits): done on the spot
                const auto f = as_global((const u64 *)(uintptr_t)cur.f);
                const u64 x = f[0];
                const u32 t = cur.tf ? as_global((const u32 *)(uintptr_t)cur.tf)[0] : fct;
                bad_t |= t == PT_UNSET;
                u32 e = cur.tf ? T.euler[t < T.size ? t : 0u] : fce;
                if (cm && cur.tf && e) e |= (u32)T.clade8[t] << 24;
                record(lane == 0, lane == 0 ? find_from(x, pt_hash(x)) : -1, x, t, e, true);
            }
            j = jn;
            cur = nxt;
            jn = take();
            nxt = fetch(jn);
            pos = cur.beg;
        }
    };
    {
        Desc d0 = next_desc(), d1 = next_desc();
        RegA a0, a1, a2;
        RegB b0, b1;
        issue_a(d0, a0);
        issue_a(d1, a1);
        issue_b(d0, a0, b0);
        while (d0.valid) {
            const Desc d2 = next_desc();
            issue_a(d2, a2);
            issue_b(d1, a1, b1);
            process(d0, a0, b0);
            d0 = d1; a0 = a1; b0 = b1;
            d1 = d2; a1 = a2;
        }
    }
    close_chunk();
    if (bad) atomicOr((unsigned long long *)&a.ctl[1], (unsigned long long)PU_FLAG_UNSORTED);
    if (bad_t) atomicOr((unsigned long long *)&a.ctl[1], (unsigned long long)PU_FLAG_TAXID);
    if (bad_raw) atomicOr((unsigned long long *)&a.ctl[1], (unsigned long long)PU_FLAG_RAW);
    __syncthreads();
    // ---- the folds: one table LCA per entry that met a different TaxId -------------------------------------------------
    auto settle = [&](int slot) -> u32 {
        const uint4 st = s_st[slot];
        const u32 mn = st.y, mx = ~st.z;
        if (mn == mx && (st.w & 1u) == 0u) return st.x;  // every record carried t0
        if (mn == 0u) return 0u;                  // TaxId 0 / an unknown id among records that differ
        if (cm) {
            if ((mn >> 24) != (mx >> 24)) return lca_clade_pair(T, mn >> 24, mx >> 24);
            return lca_dev(T, T.node_at[mn & 0xFFFFFFu], T.node_at[mx & 0xFFFFFFu]);
        }
        return lca_dev(T, T.node_at[mn], T.node_at[mx]);
    };
    if (!COUNT) {
#pragma unroll
        for (int i = 0; i < PER; i++) {
            if (ent[i] == PU_EMPTY) continue;
            const int slot = find_from(ent[i], pt_hash(ent[i]));
            const u32 res = settle(slot);
            if (a.base_tax && res != et[i]) a.base_tax[b0 + (u32)tid + (u32)i * PT_NT] = res;
            s_st[slot].w = 2u;  // (this entry is done)
        }
        __syncthreads();
    }
    // what is left in the table are the new codes of this range (COUNT: every code that reached the threshold)
    auto leaves = [&](int sl) -> bool {
        if (sl >= PT_SLOTS || s_tab[sl] == PU_EMPTY) return false;
        const u32 w = s_st[sl].w;
        return COUNT ? (w >> 2) >= a.threshold : w != 2u;
    };
    constexpr int SPT = (PT_SLOTS + PT_NT - 1) / PT_NT;
    u32 mine = 0;
#pragma unroll
    for (int i = 0; i < SPT; i++) {
        const int sl = tid * SPT + i;
        if (leaves(sl)) mine++;
    }
    u32 tot;
    u32 at_l = block_excl_scan_u32<PT_NT>(mine, s_scan, &tot);
    if (tot == 0) return;
    if (tid == 0) {
        const u64 at = atomicAdd((unsigned long long *)&a.ctl[0], (unsigned long long)tot);
        if (at + tot > a.miss_cap) atomicOr((unsigned long long *)&a.ctl[1], (unsigned long long)PU_FLAG_OVERFLOW);
        s_flush_at = at;
    }
    __syncthreads();
    const u64 at = s_flush_at;
    if (at + tot > a.miss_cap) return;
#pragma unroll
    for (int i = 0; i < SPT; i++) {
        const int sl = tid * SPT + i;
        if (leaves(sl)) {
            a.miss[at + at_l] = s_tab[sl];
            if (a.miss_tax) a.miss_tax[at + at_l] = settle(sl);
            at_l++;
        }
    }
}


// Base entries per range of the TaxId / counting pass: PT_RANGE, or less when that leaves only a few rounds of workgroups
// (one per CU) with the last one partly empty -- 1e6 base entries: 651 ranges are 2.54 rounds of 256, 768 ranges of 1302
// entries are three full ones.
u32 pt_range_for(const ukm_ctx *c, u64 n0) {
    const u64 cus = (u64)std::max(1, c->num_cu);
    const u64 r_full = (n0 + PT_RANGE - 1) / PT_RANGE;
    if (r_full >= 16 * cus) return (u32)PT_RANGE;
    const u64 rounds = (r_full + cus - 1) / cus;
    const u64 range = (n0 + rounds * cus - 1) / (rounds * cus);
    return (u32)std::min<u64>(PT_RANGE, std::max<u64>(range, 64));
}

}  // namespace

// one attempt with a base set of k0 files; *low_hit: the later files share too little with it (the caller may try more files)
static int probe_union_k0(ukm_ctx *c, const UkmStreams &in, int k0, const UkmOut &o, bool *declined, bool *low_hit, double *hit_rate) {
    *declined = true;
    *o.n = 0;
    *low_hit = false;
    int S = in.S;
    const bool tax = in.tax;
    if (S < k0 + 1) return UKM_OK;
    bool ready = true;
    if (tax) UKM_TRY(ukm_pu_tax_ready(c, o.taxids, "union", &ready));
    if (!ready) return UKM_OK;
    // The base set is built from the k0 LARGEST files, in their order; the later files follow in theirs.
    std::vector<char> in_base;
    ukm_pu_largest(in.lens, S, k0, &in_base);
    std::vector<const u64 *> keys_v((size_t)S);
    std::vector<const u32 *> tax_v((size_t)S, nullptr);
    std::vector<u64> lens_v((size_t)S);
    std::vector<u32> ct_v((size_t)S, 0u);
    for (int j = 0, b = 0, l = k0; j < S; j++) {
        const size_t at = in_base[(size_t)j] ? b++ : l++;
        keys_v[at] = in.keys[j];
        lens_v[at] = in.lens[j];
        if (tax && in.taxids) tax_v[at] = in.taxids[j];
        ct_v[at] = in.file_taxid(j);
    }
    PuLap lap{c, "[punion]"};
    // 1. the base set
    u64 later = 0;
    for (int j = k0; j < S; j++) later += lens_v[(size_t)j];
    u64 *base = nullptr, n0 = 0;
    u32 *base_tax = nullptr;
    UKM_TRY(ukm_pu_base_union(c, UkmStreams{keys_v.data(), tax_v.data(), ct_v.data(), lens_v.data(), k0, tax}, &base, &base_tax, &n0));
    if (n0 == 0) return UKM_OK;
    lap("base");

    // The plain pass (pu2_probe_kernel) loads 16-byte pairs: every file it probes has at least two records.  A later file
    // of one record goes on the list of new codes from the host -- which is what the list is: records the final union
    // adds --, an empty one is left out.  (pr_probe_kernel guards len < 2 itself.)
    const bool claiming = tax || ukm_env(c, "UKM_PUNION_CLAIM") != nullptr;
    std::vector<const u64 *> tiny;
    if (!claiming) {
        int w = k0;
        for (int j = k0; j < S; j++) {
            if (lens_v[(size_t)j] == 1) tiny.push_back(keys_v[(size_t)j]);
            if (lens_v[(size_t)j] < 2) continue;
            keys_v[(size_t)w] = keys_v[(size_t)j];
            lens_v[(size_t)w] = lens_v[(size_t)j];
            w++;
        }
        S = std::max(w, k0 + 1);
        if (w == k0) {  // (nothing left to probe: the base set and the listed records are everything)
            keys_v[(size_t)k0] = nullptr;
            lens_v[(size_t)k0] = 0;
        }
    }
    // device tables of the later files; their file taxids become taxid | its number << 32 (pu_cte_kernel)
    const int S1all = S - k0;
    bool any_ct = false;
    for (int j = k0; j < S; j++) any_ct = any_ct || ct_v[(size_t)j] != 0;
    StreamTab tab;
    u64 *ctl = nullptr;
    UKM_TRY(ukm_stream_tab(c, UkmStreams{keys_v.data(), tax_v.data(), ct_v.data(), lens_v.data(), S, tax}.from(k0), &tab));
    UKM_TRY(ws_alloc_t(c, 8, &ctl));
    UKM_HIP(hipMemsetAsync(ctl, 0, 8 * sizeof(u64), c->stream));
    if (any_ct) UKM_TRY(ukm_pu_cte(c, tab.file_taxids(), (u32)S1all));

    PuArgs a;
    memset(&a, 0, sizeof(a));
    a.base = base;
    a.n0 = n0;
    a.ctl = ctl;
    a.base_tax = base_tax;
    if (tax) a.tax = ukm_taxdev(c);
    a.files = tab.keys();
    a.lens = tab.lens();
    a.tfiles = tab.taxids();  // (the sample also looks at the taxids: clade_mode)
    a.cte = any_ct ? tab.file_taxids() : nullptr;
    a.S1 = (u32)S1all;

    // 2. do the later files look like the base set?
    u64 h[8];
    UKM_TRY(ukm_pu_hit_sample(c, a, h));
    if (h[3] == 0) return UKM_OK;
    const double miss_rate = 1.0 - (double)h[2] / (double)h[3];
    a.clade_mode = ukm_pu_clade_mode(c, a.tax, tax, h[2], h[6], h[7]);
    if (a.clade_mode && any_ct) UKM_TRY(ukm_pu_cte(c, tab.file_taxids(), (u32)S1all, 1u));  // (the numbers with their clade codes)
    if (lap.on) fprintf(stderr, "[punion] sample: %llu of %llu later records in the base set (n0 = %llu); %llu of them in the entry's clade with another taxid: clade mode %u\n",
                        (unsigned long long)h[2], (unsigned long long)h[3], (unsigned long long)n0, (unsigned long long)h[6], a.clade_mode);
    *hit_rate = 1.0 - miss_rate;
    bool too_many = false;
    UKM_TRY(ukm_pu_hit_guard(c, a, miss_rate, tax ? PT_MIN_HIT : PU_MIN_HIT, later, low_hit, &too_many));
    if (*low_hit || too_many) return UKM_OK;
    lap("sample");
    // (Plain files stay with the plain kernel down to the same hit rate: its tables claim new codes too -- 2048 per range,
    //  512 of them listed from LDS, the rest in chunks -- and a record costs half of what it costs in the tables of the
    //  TaxId pass even without TaxIds: 1000 files x 1e6, a fifth / an eighth of a universe each: 4.1 / 5.9 ms against
    //  5.9 / 7.7.  UKM_PUNION_CLAIM=1: plain files through the TaxId pass's tables all the same, an experiment.)
    a.range = claiming ? pt_range_for(c, n0) : (u32)PU_RANGE;
    const u64 R64 = (n0 + a.range - 1) / a.range;
    if (R64 > 0x7FFFFFFEull) return UKM_OK;
    a.R = (u32)R64;

    // 3. probe pass
    // (+ one partly used chunk of 64 per wave of the grid)
    u64 miss_cap = (u64)((double)later * std::min(1.0, 2.0 * miss_rate + 0.01)) + (1u << 20);
    miss_cap = std::min(miss_cap, later) + 64ull * (std::max(PU2_NT, PT_NT) / 64) * R64 * (u64)((S1all + PU_MAXS - 1) / PU_MAXS) + later / 32;
    miss_cap += tiny.size();
    UKM_TRY(ws_alloc_t(c, miss_cap + 1, &a.miss));
    if (tax) UKM_TRY(ws_alloc_t(c, miss_cap + 1, &a.miss_tax));
    a.miss_cap = miss_cap;
    if (!tiny.empty()) {  // (ctl[0] = records on the list)
        for (size_t i = 0; i < tiny.size(); i++)
            UKM_HIP(hipMemcpyAsync(a.miss + i, tiny[i], sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
        const u64 nt = tiny.size();
        UKM_HIP(hipMemcpyAsync(ctl, &nt, sizeof(u64), hipMemcpyHostToDevice, c->stream));
        UKM_HIP(hipStreamSynchronize(c->stream));  // (`nt` is an object of this frame)
    }
    bool heavy = false;
    UKM_TRY(ukm_pu_probe_batches(c, a, S1all, lens_v.data() + k0, lap, lap.on, &heavy, [&](const PuArgs &b) {
        if (claiming && b.clade_mode) hipLaunchKernelGGL((pt_probe_kernel<false, true>), dim3(b.R), dim3(PT_NT), 0, c->stream, b);
        else if (claiming) hipLaunchKernelGGL((pt_probe_kernel<false, false>), dim3(b.R), dim3(PT_NT), 0, c->stream, b);
        else hipLaunchKernelGGL(pu2_probe_kernel, dim3(b.R), dim3(PU2_NT), 0, c->stream, b);
    }));
    if (heavy) return UKM_OK;
    UKM_TRY(ukm_read_u64(c, ctl, h, 2));
    c->stat_punion_flags = h[1];
    if (lap.on) fprintf(stderr, "[punion] S=%d n0=%llu R=%u later=%llu misses=%llu (cap %llu) flags=%llu\n", S, (unsigned long long)n0,
                        a.R, (unsigned long long)later, (unsigned long long)h[0], (unsigned long long)miss_cap, (unsigned long long)h[1]);
    if (h[1] != 0) return UKM_OK;  // unsorted input / overflow: the general route reports or handles it

    // 4. base ∪ misses (with TaxIds: new codes arrive once per range and batch with their fold, unclaimed records one by one)
    return ukm_pu_finish(c, a, h[0], base, base_tax, n0, o, lap, "miss sort", declined);
}

int ukm_dev_probe_union(ukm_ctx *c, const UkmStreams &in, bool overlap_known, const UkmOut &o, bool *declined) {
    // files of the base set: eight, with TaxIds four (the base union pays an LCA per shared code: 8 files of config 3's
    // shape took as long as a third of the probe pass; the codes the later files add are claimed in the tables anyway).
    // When the later files share too little with it, ONE more attempt with four times as many files (ukm_pu_attempts).
    // (1000 files x 1e6, a tenth / a twentieth of a collection each: with taxids 20.7 / 25.7 ms against 35.2 / 36.1 through
    // the single-pass merge, plain 7.1 / 7.7 against 10.8 / 13.2; a fiftieth each would need 64 files with taxids -- their
    // union with its LCAs alone is 15 ms -- and is left to the merges: 46.4 against 38.3.)
    int k0 = in.tax ? PT_K0 : PU_K0;
    if (ukm_env(c, "UKM_PUNION_K0")) k0 = std::max(3, std::min(64, atoi(ukm_env(c, "UKM_PUNION_K0"))));  // developer knob
    *declined = true;
    *o.n = 0;
    if (ukm_punion_mode(c) < 1 && in.S >= 2 && !overlap_known) {  // (overlap_known: the caller has just taken this sample itself)
        // files that share next to nothing (a record of one is in another with less than 3 % probability: even 32 of them
        // would cover too little): one small kernel says so before a base set is built
        double share = 0.0;
        UKM_TRY(ukm_pu_overlap_share(c, in, &share));
        if (share < 0.03) return UKM_OK;
    }
    // every file carries ONE taxid: the ranked pass (its base set is a plain union: eight files)
    bool ranked = in.tax && in.file_taxids != nullptr && !ukm_env_is(c, "UKM_PUNION_RANKED", '0');
    for (int j = 0; j < in.S && ranked; j++) ranked = !(in.taxids && in.taxids[j]);
    if (ranked && !ukm_env(c, "UKM_PUNION_K0")) k0 = PU_K0;
    bool low_hit = false;
    return ukm_pu_attempts(c, k0, in.S, in.tax ? PT_MIN_HIT : PU_MIN_HIT, &low_hit, [&](int k, bool *low, double *hit) {
        return ranked ? ukm_probe_union_ranked(c, in, k, o, declined, low, hit) : probe_union_k0(c, in, k, o, declined, low, hit);
    });
}

// `common` with a threshold below the number of files by the counting tables of pt_probe_kernel<true>.  first_once: keys[0]
// is the first file as a sorted, duplicate-free set (ukm_common makes it one: every code of the first file counts once,
// common.go:232,244); every record of every other file counts (common.go:262-266).  !first_once: every record of every
// file counts (`merge -d` in its final round = the codes with at least two records, util-sort.go:519-530).  It declines (few
// or small files, more than PU_MAXS of them, later files that share too little with the first, an unsorted file, a record
// no table could count): nothing that matters was written and the caller's counting merge answers.
int ukm_dev_probe_common(ukm_ctx *c, const UkmStreams &in, u32 threshold, bool first_once, const UkmOut &o, bool *declined) {
    const int S = in.S;
    const bool tax = in.tax;
    *declined = true;
    *o.n = 0;
    const int mode = ukm_punion_mode(c);
    c->stat_punion_flags = 0;  // (as ukm_pu_attempts does for the union: the flags of THIS call's probe pass, or none)
    if (mode == 0 || S < 3 || S > PU_MAXS || in.lens[0] == 0) return UKM_OK;
    u64 later = 0;
    for (int j = 1; j < S; j++) later += in.lens[j];
    if (mode < 1 && (S < 24 || later < (1ull << 26))) return UKM_OK;
    bool ready = true;
    if (tax) UKM_TRY(ukm_pu_tax_ready(c, o.taxids, "common", &ready));
    if (!ready) return UKM_OK;
    const bool dbg = ukm_env(c, "UKM_PUNION_DEBUG") != nullptr;
    if (mode < 1) {
        double share = 0.0;
        UKM_TRY(ukm_pu_overlap_share(c, in, &share));
        if (share < 0.03) return UKM_OK;  // (files that share next to nothing: see ukm_dev_probe_union)
    }
    // device tables of ALL files; their file taxids become taxid | its number << 32 (pu_cte_kernel)
    bool any_ct = false;
    for (int j = 0; j < S; j++) any_ct = any_ct || in.file_taxid(j) != 0;
    StreamTab tab;
    u64 *ctl = nullptr;
    UKM_TRY(ukm_stream_tab(c, in, &tab));
    UKM_TRY(ws_alloc_t(c, 8, &ctl));
    UKM_HIP(hipMemsetAsync(ctl, 0, 8 * sizeof(u64), c->stream));
    if (any_ct) UKM_TRY(ukm_pu_cte(c, tab.file_taxids(), (u32)S));
    PuArgs a;
    memset(&a, 0, sizeof(a));
    a.ctl = ctl;
    a.threshold = threshold;
    if (tax) a.tax = ukm_taxdev(c);
    auto probe_from = [&](int j0) {  // the files probed: j0 .. S - 1
        a.files = tab.keys() + j0;
        a.lens = tab.lens() + j0;
        a.tfiles = tab.taxids() + j0;
        a.cte = any_ct ? tab.file_taxids() + j0 : nullptr;
        a.S1 = (u32)(S - j0);
    };
    // (the last sample in front of the launch decides the clade mode; ctl is cleared on both sides of it)
    auto hit_rate = [&](double *rate) -> int {
        u64 h[8];
        UKM_HIP(hipMemsetAsync(ctl, 0, 8 * sizeof(u64), c->stream));
        UKM_TRY(ukm_pu_hit_sample(c, a, h));
        *rate = h[3] ? (double)h[2] / (double)h[3] : 0.0;
        a.clade_mode = ukm_pu_clade_mode(c, a.tax, tax, h[2], h[6], h[7]);
        if (dbg) fprintf(stderr, "[pcommon] sample: %llu of %llu records of the probed files in the base set (n0 = %llu); clade mode %u\n", (unsigned long long)h[2],
                         (unsigned long long)h[3], (unsigned long long)a.n0, a.clade_mode);
        UKM_HIP(hipMemsetAsync(ctl, 0, 8 * sizeof(u64), c->stream));
        return UKM_OK;
    };
    // BASE = the first file, its codes counted once, the other files probed -- when they share enough with it.  Else
    // BASE = the union of the first four files (the TaxIds folded; folding them once more is harmless: LCA(x, x) = x)
    // with no record counted yet, and EVERY file is probed.
    a.base = in.keys[0];
    a.base_tax = (tax && in.taxids) ? const_cast<u32 *>(in.taxids[0]) : nullptr;  // (read only in this mode)
    a.base_ct = in.file_taxid(0);
    a.n0 = in.lens[0];
    a.count0 = 1;
    probe_from(1);
    double rate = 0.0;
    if (first_once) UKM_TRY(hit_rate(&rate));
    if (!first_once || (mode != 2 && rate < PT_MIN_HIT)) {
        // (four files, or -- when their sample promises enough -- sixteen)
        bool low_hit = false;
        UKM_TRY(ukm_pu_attempts(c, std::min(S, PT_K0), S, PT_MIN_HIT, &low_hit, [&](int k0, bool *low, double *hit) -> int {
            u64 *base = nullptr, n0 = 0;
            u32 *base_tax = nullptr;
            UKM_TRY(ukm_pu_base_union(c, UkmStreams{in.keys, in.taxids, in.file_taxids, in.lens, k0, tax}, &base, &base_tax, &n0));
            a.n0 = n0;
            if (n0 == 0) return UKM_OK;
            a.base = base;
            a.base_tax = base_tax;
            a.base_ct = 0;
            a.count0 = 0;
            probe_from(0);
            UKM_TRY(hit_rate(hit));
            *low = mode != 2 && *hit < PT_MIN_HIT;
            return UKM_OK;
        }));
        if (low_hit || a.n0 == 0) return UKM_OK;
        later += in.lens[0];
    }
    const u64 n0 = a.n0;
    const int S1 = (int)a.S1;
    a.range = pt_range_for(c, n0);
    const u64 R64 = (n0 + a.range - 1) / a.range;
    if (R64 > 0x7FFFFFFEull) return UKM_OK;
    a.R = (u32)R64;
    // every code leaves at most once: the first file's codes and what the tables claim (as many again at most)
    const u64 list_cap = 2 * n0 + 64 * R64 + 64;
    UKM_TRY(ws_alloc_t(c, list_cap + 1, &a.miss));
    if (tax) UKM_TRY(ws_alloc_t(c, list_cap + 1, &a.miss_tax));
    a.miss_cap = list_cap;
    UKM_TRY(ws_alloc_t(c, ((size_t)a.R + 1) * S1, &a.cuts));
    UKM_TRY(pu_launch_cuts(c, a));
    bool heavy = false;
    UKM_TRY(ukm_pu_range_load(c, a, later, false, &heavy));
    if (heavy) return UKM_OK;  // (one workgroup would stream most of the input)
    if (a.clade_mode && a.cte) UKM_TRY(ukm_pu_cte(c, const_cast<u64 *>(a.cte), (u32)S1, 1u));  // (the numbers with their clade codes)
    (void)hipEventRecord(c->ev_k0, c->stream);
    if (a.clade_mode) hipLaunchKernelGGL((pt_probe_kernel<true, true>), dim3(a.R), dim3(PT_NT), 0, c->stream, a);
    else hipLaunchKernelGGL((pt_probe_kernel<true, false>), dim3(a.R), dim3(PT_NT), 0, c->stream, a);
    (void)hipEventRecord(c->ev_k1, c->stream);
    c->evk_valid = true;
    UKM_HIP(hipGetLastError());
    u64 h[2] = {0, 0};
    UKM_TRY(ukm_read_u64(c, ctl, h, 2));
    c->stat_punion_flags = h[1];
    if (dbg) fprintf(stderr, "[pcommon] S=%d n0=%llu R=%u later=%llu threshold=%u out=%llu flags=%llu\n", S, (unsigned long long)n0, a.R,
                     (unsigned long long)later, threshold, (unsigned long long)h[0], (unsigned long long)h[1]);
    if (h[1] != 0) return UKM_OK;
    const u64 nm = h[0];
    *declined = false;
    *o.n = nm;
    if (nm > o.cap)
        UKM_FAIL(UKM_ERR_CAPACITY, "common: output needs %llu records, capacity is %llu", (unsigned long long)nm, (unsigned long long)o.cap);
    if (nm == 0) return UKM_OK;
    // the ranges wrote their codes in the order they finished: one sort puts them in code order (every code is in the
    // list once)
    UKM_TRY(ukm_dev_sort(c, a.miss, tax ? a.miss_tax : nullptr, nm, 64));
    UKM_HIP(hipMemcpyAsync(o.keys, a.miss, nm * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
    if (tax) UKM_HIP(hipMemcpyAsync(o.taxids, a.miss_tax, nm * sizeof(u32), hipMemcpyDeviceToDevice, c->stream));
    return UKM_OK;
}
