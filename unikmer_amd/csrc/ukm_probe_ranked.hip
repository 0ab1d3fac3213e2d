// ukm_probe_ranked.hip — the probe union of files that carry ONE taxid each (the .unik header's global taxid): the ranked
// pass (pr_probe_kernel) and its route ukm_probe_union_ranked, which ukm_dev_probe_union picks for such files.
#include <algorithm>
#include <vector>

#include "ukm_probe.h"

namespace {


// ---- every file carries ONE taxid (round 5: the .unik header's global taxid, `count -t`) ---------------------------------
// union.go:195-201 then folds, for every code, the taxids of the FILES that hold it.  The distinct taxid values of a call
// are few (at most one per file), so the host RANKS them: sorted by (pre-order number, taxid value), rank 1 .. D.  The LCA
// of a set of nodes is the LCA of its members with the smallest and the largest pre-order number, and ranks order the
// values by that number -- so all an entry has to keep is the smallest and the largest RANK among the files that hold its
// code: one 32-bit word per slot ([15:0] smallest rank, [31:16] the complement of the largest; 0xFFFFFFFF = no file yet).
// A record costs its hash probe (the plain kernel's: one 32-byte bucket read) and ONE more 4-byte LDS read; the rank of
// its file is a wave-uniform scalar, and the word only changes while the file's rank lies outside the entry's interval --
// the host hands the files over in the order lowest rank, highest, second lowest, second highest ..., so after an entry's
// first two or three files hardly any does (a CAS loop then; no atomic otherwise).  No taxid is loaded, no pre-order
// number looked up, no LCA evaluated while the files stream.
// BASE is the PLAIN union of the largest files (no LCA in its k-way union) and EVERY file is probed, the base files
// included: their ranks are folded like anybody's.  The entries' words live in base_st[] between launches (more files than
// one launch takes: the next batch starts from them); pr_settle_kernel turns them into taxids at the end -- one rank: that
// taxid itself (LCA(x, x) = x, also for an unknown id); else 0 when the smallest number is 0 (taxid 0 / unknown ids among
// files that differ); else LCA(node_at[smallest number], node_at[largest]) -- the left fold of lca_dev, as in ukm_pfold.hip.
// New codes are claimed in the table as in the other kernels and leave with their settled taxid when the range is done;
// what cannot be claimed (all-ones codes, a table that has doubled) is listed record by record with the file's taxid and
// the final sort + unique + 2-way union folds it (associativity is all that is used).
constexpr u32 PR_NONE = 0xFFFFFFFFu; // no file yet
constexpr u32 PR_MAX_RANK = 0xFFFEu;

struct PrTables {
    const u32 *tax_of_rank;  // [D + 1]
    const u32 *eul_of_rank;  // [D + 1]: the pre-order number of the rank's taxid (non-decreasing in the rank)
    u32 *base_st;            // [n0] in / out: the rank interval of every base entry
    // the settled taxid of every (smallest rank, largest rank) pair, [D + 1][D + 1], when the call has at most PR_PAIR_MAX
    // distinct taxids (pr_pairs_kernel): 2e8 entries then settle with one cached read instead of an LCA each
    u32 *pair;
    u32 D;
};
constexpr u32 PR_PAIR_MAX = 1024;

__device__ __forceinline__ u32 pr_settle_pair(const PrTables &t, const TaxDev &T, u32 mn, u32 mx) {
    if (mn == mx) return t.tax_of_rank[mn];
    const u32 en = t.eul_of_rank[mn], ex = t.eul_of_rank[mx];
    if (en == 0u) return 0u;
    return lca_dev(T, T.node_at[en], T.node_at[ex]);
}

__device__ __forceinline__ u32 pr_settle(const PrTables &t, const TaxDev &T, u32 w) {
    const u32 mn = w & 0xFFFFu, mx = 0xFFFFu - (w >> 16);
    if (w == PR_NONE || mn > mx || mx > t.D) return 0u;  // (no file held the code: cannot happen for an entry that is in the table)
    if (t.pair) return t.pair[(size_t)mn * (t.D + 1) + mx];
    return pr_settle_pair(t, T, mn, mx);
}

__global__ void pr_pairs_kernel(PrTables t, TaxDev T) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 W = t.D + 1;
    if (i >= W * W) return;
    const u32 mn = i / W, mx = i % W;
    t.pair[i] = (mn >= 1 && mn <= mx) ? pr_settle_pair(t, T, mn, mx) : 0u;
}

__global__ void pr_settle_kernel(PrTables t, TaxDev T, u64 n0, u32 *base_tax) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n0) base_tax[i] = pr_settle(t, T, t.base_st[i]);
}

// Table layout: round 5 kept 4-byte TAGS per slot beside the codes (a record read 16 bytes of tags, then the code and rank
// word of the slot whose tag matched); round 6 reads the codes themselves, P pair first (see the kernel): 12 bytes per slot.
#ifndef PR_TNT_N
#define PR_TNT_N 1024
#endif
#ifndef PR_TBUCKETS_N
#define PR_TBUCKETS_N 1536
#endif
#ifndef PR_TWAVES
#define PR_TWAVES 8
#endif
// (measured on config 3's shape at half size, probe pass: 2304 buckets x 1024 threads, one workgroup per CU = 4 waves per SIMD
//  14.3 ms; 1152 x 512 x 2 workgroups 14.9; 768 x 512 x 3 = 6 waves 12.6; 1152 x 1024 x 2 = 8 waves per SIMD 12.55)
constexpr int PR_TNT = PR_TNT_N;               // threads of a workgroup
constexpr int PR_TBUCKETS = PR_TBUCKETS_N;     // x 4 slots x (8 + 4) bytes = 72 KB of LDS: two workgroups of 16 waves per CU
constexpr int PR_TSLOTS = 4 * PR_TBUCKETS;
// ONE multiplicative hash per code (v_mul_lo_u32 runs at a quarter of the VALU rate: the two products + the mul_hi of
// the first version were a fifth of the kernel's vector work): its top bits pick the bucket, the word itself (odd: never
// 0) is the tag -- inside a bucket the tags still differ in 21 bits, and a false positive only costs the exact look-up.
__device__ __forceinline__ u32 prt_hash(u64 x) {
    const u32 lo = (u32)x, hi = (u32)(x >> 32);
    return (lo ^ __builtin_rotateleft32(hi, 15) ^ (hi >> 3)) * 0x9E3779B1u;
}
__device__ __forceinline__ u32 prt_bucket_of(u32 h) {
    if ((PR_TBUCKETS & (PR_TBUCKETS - 1)) == 0) return h >> (32 - __builtin_ctz((unsigned)PR_TBUCKETS));
    return (u32)(((u64)h * (u64)PR_TBUCKETS) >> 32);
}
__device__ __forceinline__ u32 prt_bucket(u64 x) { return prt_bucket_of(prt_hash(x)); }

__global__ __launch_bounds__(PR_TNT) __attribute__((amdgpu_waves_per_eu(PR_TWAVES, PR_TWAVES))) void pr_probe_kernel(PuArgs a, PrTables t) {
    // (round 6: no tag words any more -- the codes in two halves as in pu2_probe_kernel: slots 0 and 1 of every bucket in the
    //  first half (P), slots 2 and 3 behind them (Q); a record reads its bucket's P pair, and only a lane that does not find
    //  it there and sees slot 1 taken reads the Q pair; then the rank word of the slot that matched.  Four tag compares, a
    //  select chain and the dependent code read per record are gone, and the table shrinks from 16 to 12 bytes per slot.)
    __shared__ __attribute__((aligned(16))) u64 s_key[PR_TSLOTS];
    __shared__ u32 s_st[PR_TSLOTS];
    auto sidx = [](u32 h, int q) -> int { return (q >> 1) * (PR_TSLOTS / 2) + (int)(2 * h) + (q & 1); };
    __shared__ u32 s_next, s_nins;
    __shared__ u32 s_scan[PR_TNT / 64 + 1];
    __shared__ u64 s_flush_at;
    const int tid = (int)threadIdx.x, lane = lane_id();
    const u32 r = blockIdx.x, S1 = a.S1;
    for (int i = tid; i < PR_TSLOTS; i += PR_TNT) {
        s_key[i] = PU_EMPTY;
        s_st[i] = PR_NONE;
    }
    if (tid == 0) { s_next = 0; s_nins = 0; }
    __syncthreads();
    auto next_bucket = [](u32 h) -> u32 { return h + 1 == (u32)PR_TBUCKETS ? 0u : h + 1; };
    // first free slot of the first bucket of the probe sequence that is not full, or the slot that already holds x
    auto insert = [&](u64 x, bool &fresh) -> int {
        u32 h = prt_bucket(x);
        for (;; h = next_bucket(h)) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const u64 old = atomicCAS((unsigned long long *)&s_key[sidx(h, k)], (unsigned long long)PU_EMPTY, (unsigned long long)x);
                if (old == PU_EMPTY || old == x) {
                    fresh = old == PU_EMPTY;
                    return sidx(h, k);
                }
            }
        }
    };
    // (the slow, exact way: walk the codes of x's probe sequence)
    auto find_codes = [&](u64 x) -> int {
        if (x == PU_EMPTY) return -1;
        u32 h = prt_bucket(x);
        for (;; h = next_bucket(h)) {
            const ulonglong2 p = *reinterpret_cast<const ulonglong2 *>(&s_key[sidx(h, 0)]), q = *reinterpret_cast<const ulonglong2 *>(&s_key[sidx(h, 2)]);
            const int k = p.x == x ? 0 : (p.y == x ? 1 : (q.x == x ? 2 : (q.y == x ? 3 : -1)));
            if (k >= 0) return sidx(h, k);
            if (q.y == PU_EMPTY) return -1;
        }
    };
    const u64 b0 = (u64)r * a.range;
    const u32 nb = (u32)((a.n0 - b0 < (u64)a.range) ? (a.n0 - b0) : (u64)a.range);
    constexpr int PER = (PR_TBUCKETS + PR_TNT - 1) / PR_TNT;
    u64 ent[PER];
    u32 est[PER];
    int eslot[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const u32 idx = (u32)tid + (u32)i * PR_TNT;
        ent[i] = a.base[b0 + (idx < nb ? idx : 0)];
        est[i] = t.base_st[b0 + (idx < nb ? idx : 0)];
        if (idx >= nb) ent[i] = PU_EMPTY;
    }
#pragma unroll
    for (int i = 0; i < PER; i++) {
        eslot[i] = -1;
        if (ent[i] == PU_EMPTY) continue;  // (an all-ones code: its records are listed, the final union folds them)
        bool fresh;
        eslot[i] = insert(ent[i], fresh);
        s_st[eslot[i]] = est[i];
    }
    __syncthreads();
    const u64 lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    u64 chunk_at = 0, fill = 0;  // wave-uniform
    u32 fill_t = 0;
    u32 chunk_cap = 0, chunk_used = 0;
    auto close_chunk = [&]() {
        if ((u32)lane < chunk_cap - chunk_used) {
            a.miss[chunk_at + chunk_used + (u32)lane] = fill;
            a.miss_tax[chunk_at + chunk_used + (u32)lane] = fill_t;
        }
        chunk_cap = chunk_used = 0;
    };
    auto append_global = [&](bool m, u64 x, u32 tx) {
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
        fill_t = tx;  // (wave-uniform: the file's taxid)
        if (m) {
            const u64 at = chunk_at + chunk_used + (u32)__popcll(mask & lt);
            a.miss[at] = x;
            a.miss_tax[at] = tx;
        }
        chunk_used += n;
    };
    // widen the interval of `slot` by a file of rank rk (crk = its complement)
    auto widen = [&](int slot, u32 rk, u32 crk) {
        u32 *w = &s_st[slot];
        u32 old = *w;
        for (;;) {
            const u32 mn = old & 0xFFFFu, cmx = old >> 16;
            const u32 nw = (mn < rk ? mn : rk) | ((cmx < crk ? cmx : crk) << 16);
            if (nw == old) break;
            const u32 prev = atomicCAS(w, old, nw);
            if (prev == old) break;
            old = prev;
        }
    };
    // the rare part of a record: the tags did not settle it (slot < 0: look the codes up, claim a slot or list the record), or
    // its file's rank lies outside the entry's interval
    auto rare = [&](bool valid, int slot, u64 x, u32 rk, u32 crk, u32 ftax) {
        bool raw = false;
        if (valid) {
            if (slot < 0) slot = find_codes(x);
            if (slot < 0) {
                if (x == PU_EMPTY || s_nins >= (u32)PR_TBUCKETS) raw = true;
                else {
                    bool fresh;
                    slot = insert(x, fresh);
                    if (fresh) atomicAdd(&s_nins, 1u);
                }
            }
            if (!raw) widen(slot, rk, crk);
        }
        append_global(raw, x, ftax);
    };
    bool bad = false, raw_slice = false;
    // N records of one file of rank rk, from registers: the P pairs of ALL of them are read; one masked region reads the Q
    // pairs of the lanes that need them; then the rank words of the slots that matched; then every record is judged.
    auto judge = [&](auto NN, const u64 *x, const bool *v, u32 rk, u32 crk, u32 ftax) {
        constexpr int N = decltype(NN)::value;
        ulonglong2 pp[N];
        u32 hh[N];
#pragma unroll
        for (int i = 0; i < N; i++) {
            hh[i] = prt_bucket(x[i]);
            pp[i] = *reinterpret_cast<const ulonglong2 *>(&s_key[sidx(hh[i], 0)]);
        }
        int sl[N];
        bool needq = false;
#pragma unroll
        for (int i = 0; i < N; i++) {
            sl[i] = pp[i].x == x[i] ? sidx(hh[i], 0) : (pp[i].y == x[i] ? sidx(hh[i], 1) : -1);
            needq = needq || (sl[i] < 0 && pp[i].y != PU_EMPTY);
        }
        if (needq) {
#pragma unroll
            for (int i = 0; i < N; i++) {
                const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(&s_key[sidx(hh[i], 2)]);
                if (sl[i] < 0) sl[i] = q.x == x[i] ? sidx(hh[i], 2) : (q.y == x[i] ? sidx(hh[i], 3) : -1);
            }
        }
        u32 ww[N];
#pragma unroll
        for (int i = 0; i < N; i++) ww[i] = s_st[sl[i] < 0 ? 0 : sl[i]];
        bool more[N];
        bool any = false;
#pragma unroll
        for (int i = 0; i < N; i++) {
            const bool hit = sl[i] >= 0 && x[i] != PU_EMPTY;
            const bool outside = rk < (ww[i] & 0xFFFFu) || crk < (ww[i] >> 16);
            if (!hit) sl[i] = -1;  // (not in the bucket's four slots, or a full bucket: the codes of the probe sequence decide)
            more[i] = v[i] && (!hit || outside);
            any = any || more[i];
        }
        if (__ballot(any) == 0ull) return;
#pragma unroll
        for (int i = 0; i < N; i++) {
            if (__ballot(more[i]) == 0ull) continue;
            rare(more[i], sl[i], x[i], rk, crk, ftax);
        }
    };
    auto take = [&]() -> u32 {
        u32 j = 0;
        if (lane == 0) j = atomicAdd(&s_next, 1u);
        return (u32)__builtin_amdgcn_readfirstlane((int)j);
    };
    struct Meta { u64 beg, end, len, f, cte; };
    auto fetch = [&](u32 j) -> Meta {
        Meta m = {0, 0, 0, 0, 0};
        if (j < S1) {
            m.beg = sload_u64(&a.cuts[(u64)r * S1 + j]);
            m.end = sload_u64(&a.cuts[(u64)(r + 1) * S1 + j]);
            m.len = sload_u64(&a.lens[j]);
            m.f = sload_u64((const u64 *)&a.files[j]);
            m.cte = sload_u64(&a.cte[j]);  // [31:0] the file's taxid, [63:32] its rank
        }
        return m;
    };
    // The streaming skeleton of pu2_probe_kernel (round 6): a slice = one general first step (it starts one record early when
    // the slice does not begin its file: the boundary pair is checked inside lane 0), batches of full steps without
    // validity masks, general steps for what is left; the order check takes a pair's predecessor from the neighbouring
    // lane (DPP wave_shr:1) instead of a third load per lane.
    const u32 l2 = 2u * (u32)lane;
    u64 run_carry = 0, ptr = 0;
    u32 rem = 0, rk = 0, crk = 0, ftax = 0;
    auto order = [&](u64 x0, u64 x1, bool cross) {
        const u64 prev = pu2_shr1(x1, run_carry);
        bad |= (cross && prev > x0) || x0 > x1;
        run_carry = ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(x1 >> 32), 63) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)x1, 63);
    };
    auto general_step = [&](u32 lo, bool first) {
        const u32 cnt = rem < 128u ? rem : 128u;
        // one record: at the start of its file the pair (0, 1) -- the file has two records --, else the pair (-1, 0)
        const u32 back = (cnt == 1u && !first) ? 1u : 0u;
        const u32 slo = back ? 1u : lo, shi = cnt + back;
        const u32 pmax = shi > 2u ? shi - 2u : 0u;
        const u32 i0 = l2 < pmax ? l2 : pmax;  // the records this lane holds: i0, i0 + 1 (lanes beyond re-read the last pair)
        const pu_pair pr = *(const pu_pair __attribute__((address_space(1))) *)((const char __attribute__((address_space(1))) *)(uintptr_t)(ptr - 8) +
                                                                               (8u - 8u * back + 8u * i0));
        order(pr.x, pr.y, l2 <= pmax);
        const u64 x[2] = {pr.x, pr.y};
        const bool v[2] = {i0 - slo < shi - slo, i0 + 1u - slo < shi - slo};
        judge(std::integral_constant<int, 2>{}, x, v, rk, crk, ftax);
        rem -= cnt;
        ptr += 1024;
    };
    const u32 voff_full = 16u * (u32)lane;
#ifndef PR_U_N
#define PR_U_N 1
#endif
    constexpr int PRU = PR_U_N;
    u32 j = take();
    Meta cur = fetch(j);
    while (j < S1) {
        const u32 jn = take();
        const Meta nxt = fetch(jn);
        const u64 end = cur.end < cur.beg ? cur.beg : cur.end, n = end - cur.beg;
        ftax = (u32)cur.cte;
        rk = (u32)(cur.cte >> 32);
        crk = 0xFFFFu - rk;
        if (n >= 0xFFFFFF00ull) raw_slice = true;  // (a slice of 2^32 records: the caller's other routes)
        else if (cur.len < 2) {  // (a one-record file: no 16-byte load fits)
            if (n) {
                const u64 x = as_global((const u64 *)(uintptr_t)cur.f)[0];
                rare(lane == 0, -1, x, rk, crk, ftax);
            }
        } else if (n) {
            const u32 lo = cur.beg ? 1u : 0u;
            ptr = cur.f + 8ull * (cur.beg - lo);
            rem = (u32)n + lo;
            run_carry = 0;
            general_step(lo, true);
            while (rem >= 128u * PRU) {
                pu_pair pr[PRU];
#pragma unroll
                for (int u = 0; u < PRU; u++)
                    pr[u] = *(const pu_pair __attribute__((address_space(1))) *)((const char __attribute__((address_space(1))) *)(uintptr_t)ptr + (voff_full + 1024u * (u32)u));
                u64 x[2 * PRU];
                bool v[2 * PRU];
#pragma unroll
                for (int u = 0; u < PRU; u++) {
                    order(pr[u].x, pr[u].y, true);
                    x[2 * u] = pr[u].x;
                    x[2 * u + 1] = pr[u].y;
                    v[2 * u] = v[2 * u + 1] = true;
                }
                judge(std::integral_constant<int, 2 * PRU>{}, x, v, rk, crk, ftax);
                rem -= 128u * PRU;
                ptr += 1024ull * PRU;
            }
            while (rem) general_step(0u, false);
        }
        j = jn;
        cur = nxt;
    }
    if (raw_slice && lane == 0) atomicOr((unsigned long long *)&a.ctl[1], (unsigned long long)PU_FLAG_OVERFLOW);
    close_chunk();
    if (bad) atomicOr((unsigned long long *)&a.ctl[1], (unsigned long long)PU_FLAG_UNSORTED);
    __syncthreads();
    // the base entries hand their intervals back (the next batch of files, or pr_settle_kernel, goes on from them) ...
#pragma unroll
    for (int i = 0; i < PER; i++) {
        if (eslot[i] < 0) continue;
        const u32 w = s_st[eslot[i]];
        if (w != est[i]) t.base_st[b0 + (u32)tid + (u32)i * PR_TNT] = w;
        s_key[eslot[i]] = PU_EMPTY;  // (... and leave the table: what is left are the new codes of this range)
    }
    __syncthreads();
    constexpr int SPT = (PR_TSLOTS + PR_TNT - 1) / PR_TNT;
    u32 mine = 0;
#pragma unroll
    for (int i = 0; i < SPT; i++) {
        const int q = tid * SPT + i;
        if (q < PR_TSLOTS && s_key[q] != PU_EMPTY) mine++;
    }
    u32 tot;
    u32 at_l = block_excl_scan_u32<PR_TNT>(mine, s_scan, &tot);
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
        const int q = tid * SPT + i;
        if (q < PR_TSLOTS && s_key[q] != PU_EMPTY) {
            a.miss[at + at_l] = s_key[q];
            a.miss_tax[at + at_l] = pr_settle(t, a.tax, s_st[q]);
            at_l++;
        }
    }
}

// Base entries per range of the ranked pass (pt_range_for's rule with its own table size)
static u32 pr_range_for(const ukm_ctx *c, u64 n0) {
    const u64 slots = (u64)std::max(1, c->num_cu) * (u64)std::max(1, (160 * 1024) / (PR_TSLOTS * 12 + 1024));  // (workgroups resident at once)
    const u64 r_full = (n0 + PR_TBUCKETS - 1) / PR_TBUCKETS;
    if (r_full >= 16 * slots) return (u32)PR_TBUCKETS;
    const u64 rounds = (r_full + slots - 1) / slots;
    const u64 range = (n0 + rounds * slots - 1) / (rounds * slots);
    return (u32)std::min<u64>(PR_TBUCKETS, std::max<u64>(range, 64));
}

}  // namespace

int ukm_probe_union_ranked(ukm_ctx *c, const UkmStreams &in, int k0, const UkmOut &o, bool *declined, bool *low_hit, double *hit_rate) {
    *declined = true;
    *o.n = 0;
    *low_hit = false;
    const int S = in.S;
    const u64 *const *keys_in = in.keys;
    const u64 *lens_in = in.lens;
    const u32 *ctax = in.file_taxids;
    if (S < k0 + 1) return UKM_OK;
    bool ready = true;
    UKM_TRY(ukm_pu_tax_ready(c, o.taxids, "union", &ready));
    if (!ready) return UKM_OK;
    PuLap lap{c, "[punion/ranked]"};
    // 0. the distinct taxid values, ranked by (pre-order number, value)
    std::vector<u32> vals(ctax, ctax + S);
    std::sort(vals.begin(), vals.end());
    vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
    const size_t D = vals.size();
    if (D > (size_t)PR_MAX_RANK) return UKM_OK;
    std::vector<u64> ve(D);
    for (size_t i = 0; i < D; i++) ve[i] = (u64)vals[i];
    u64 *d_ve = nullptr;
    UKM_TRY(ws_alloc_t(c, D, &d_ve));
    UKM_HIP(hipMemcpyAsync(d_ve, ve.data(), D * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    UKM_TRY(ukm_pu_cte(c, d_ve, (u32)D));
    UKM_HIP(hipMemcpyAsync(ve.data(), d_ve, D * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    UKM_HIP(hipStreamSynchronize(c->stream));
    std::vector<size_t> byrank(D);
    for (size_t i = 0; i < D; i++) byrank[i] = i;
    std::sort(byrank.begin(), byrank.end(), [&](size_t x, size_t y) {
        const u32 ex = (u32)(ve[x] >> 32), ey = (u32)(ve[y] >> 32);
        return ex != ey ? ex < ey : vals[x] < vals[y];
    });
    std::vector<u32> rank_of_val(D), tor(D + 1, 0u), eor(D + 1, 0u);
    for (size_t rnk = 0; rnk < D; rnk++) {
        rank_of_val[byrank[rnk]] = (u32)rnk + 1;
        tor[rnk + 1] = vals[byrank[rnk]];
        eor[rnk + 1] = (u32)(ve[byrank[rnk]] >> 32);
    }
    std::vector<u32> rank_of_file((size_t)S);
    for (int j = 0; j < S; j++)
        rank_of_file[(size_t)j] = rank_of_val[(size_t)(std::lower_bound(vals.begin(), vals.end(), ctax[j]) - vals.begin())];
    // 1. the base set: the PLAIN union of the k0 largest files, the largest first
    std::vector<char> in_base;
    const std::vector<int> ord = ukm_pu_largest(lens_in, S, k0, &in_base);
    std::vector<const u64 *> bkeys((size_t)k0);
    std::vector<u64> blens((size_t)k0);
    u64 later = 0, total = 0;
    for (int j = 0; j < k0; j++) {
        bkeys[(size_t)j] = keys_in[ord[(size_t)j]];
        blens[(size_t)j] = lens_in[ord[(size_t)j]];
    }
    for (int j = 0; j < S; j++) {
        total += lens_in[j];
        if (!in_base[(size_t)j]) later += lens_in[j];
    }
    u64 *base = nullptr, n0 = 0;
    u32 *no_tax = nullptr;
    UKM_TRY(ukm_pu_base_union(c, UkmStreams{bkeys.data(), nullptr, nullptr, blens.data(), k0, false}, &base, &no_tax, &n0));
    if (n0 == 0) return UKM_OK;
    lap("base");
    // 2. device tables.  [0, S): every file in the order lowest rank, highest, second lowest, second highest ... (an entry's
    // interval is then final after its first two or three files); [S, 2S): lengths; [2S, 3S): taxid | rank << 32;
    // [3S, 3S + 2 S1): the files outside the base set and their lengths, for the hit-rate sample
    std::vector<int> byr((size_t)S);
    for (int j = 0; j < S; j++) byr[(size_t)j] = j;
    std::stable_sort(byr.begin(), byr.end(), [&](int x, int y) { return rank_of_file[(size_t)x] < rank_of_file[(size_t)y]; });
    std::vector<int> visit;
    visit.reserve((size_t)S);
    for (int lo = 0, hi = S - 1; lo <= hi; lo++, hi--) {
        visit.push_back(byr[(size_t)lo]);
        if (hi != lo) visit.push_back(byr[(size_t)hi]);
    }
    const int S1 = S - k0;
    std::vector<u64> tab((size_t)3 * S + 2 * (size_t)S1);
    for (int q = 0; q < S; q++) {
        const int j = visit[(size_t)q];
        tab[(size_t)q] = (u64)(uintptr_t)keys_in[j];
        tab[(size_t)S + q] = lens_in[j];
        tab[(size_t)2 * S + q] = (u64)ctax[j] | ((u64)rank_of_file[(size_t)j] << 32);
    }
    for (int j = 0, q = 0; j < S; j++)
        if (!in_base[(size_t)j]) {
            tab[(size_t)3 * S + q] = (u64)(uintptr_t)keys_in[j];
            tab[(size_t)3 * S + S1 + q] = lens_in[j];
            q++;
        }
    u64 *d_tab = nullptr, *ctl = nullptr;
    u32 *d_rank = nullptr;
    UKM_TRY(ws_alloc_t(c, tab.size(), &d_tab));
    UKM_TRY(ws_alloc_t(c, 8, &ctl));
    UKM_TRY(ws_alloc_t(c, 2 * (D + 1), &d_rank));
    UKM_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    UKM_HIP(hipMemcpyAsync(d_rank, tor.data(), (D + 1) * sizeof(u32), hipMemcpyHostToDevice, c->stream));
    UKM_HIP(hipMemcpyAsync(d_rank + D + 1, eor.data(), (D + 1) * sizeof(u32), hipMemcpyHostToDevice, c->stream));
    UKM_HIP(hipMemsetAsync(ctl, 0, 8 * sizeof(u64), c->stream));
    UKM_HIP(hipStreamSynchronize(c->stream));  // (pageable host buffers of this frame)
    PuArgs a;
    memset(&a, 0, sizeof(a));
    a.base = base;
    a.n0 = n0;
    a.ctl = ctl;
    a.tax = ukm_taxdev(c);
    // 3. do the other files look like the base set?
    a.files = (const u64 *const *)(d_tab + 3 * (size_t)S);
    a.lens = d_tab + 3 * (size_t)S + S1;
    a.S1 = (u32)S1;
    u64 h[8];
    UKM_TRY(ukm_pu_hit_sample(c, a, h, 4));  // (no per-record taxids, so no clade mode: the hit counts are all it reads)
    if (h[3] == 0) return UKM_OK;
    const double miss_rate = 1.0 - (double)h[2] / (double)h[3];
    bool too_many = false;
    UKM_TRY(ukm_pu_hit_guard(c, a, miss_rate, PT_MIN_HIT, later, low_hit, &too_many));
    if (too_many) return UKM_OK;
    // (the sample line follows the estimate's and is left out when the estimate declines: the [punion/ranked] debug output
    //  is kept as this route has always printed it, and the guard's two checks exclude each other, so nothing else moves)
    if (lap.on) fprintf(stderr, "[punion/ranked] sample: %llu of %llu later records in the base set (n0 = %llu, %zu distinct taxids)\n",
                        (unsigned long long)h[2], (unsigned long long)h[3], (unsigned long long)n0, D);
    *hit_rate = 1.0 - miss_rate;
    if (*low_hit) return UKM_OK;
    UKM_HIP(hipMemsetAsync(ctl, 0, 8 * sizeof(u64), c->stream));
    lap("sample");
    a.range = pr_range_for(c, n0);
    const u64 R64 = (n0 + a.range - 1) / a.range;
    if (R64 > 0x7FFFFFFEull) return UKM_OK;
    a.R = (u32)R64;
    PrTables t;
    t.tax_of_rank = d_rank;
    t.eul_of_rank = d_rank + D + 1;
    t.D = (u32)D;
    t.pair = nullptr;
    if (D <= (size_t)PR_PAIR_MAX) {
        u32 *pair = nullptr;
        UKM_TRY(ws_alloc_t(c, (D + 1) * (D + 1), &pair));
        t.pair = pair;
        hipLaunchKernelGGL(pr_pairs_kernel, dim3((unsigned)(((D + 1) * (D + 1) + 255) / 256)), dim3(256), 0, c->stream, t, a.tax);
        UKM_HIP(hipGetLastError());
    }
    UKM_TRY(ws_alloc_t(c, n0 + 1, &t.base_st));
    UKM_HIP(hipMemsetAsync(t.base_st, 0xFF, (n0 + 1) * sizeof(u32), c->stream));
    // 4. the probe pass over EVERY file
    u64 miss_cap = (u64)((double)later * std::min(1.0, 2.0 * miss_rate + 0.01)) + (1u << 20);
    miss_cap = std::min(miss_cap, total) + 64ull * (PR_TNT / 64) * R64 * (u64)((S + PU_MAXS - 1) / PU_MAXS) + total / 32;
    UKM_TRY(ws_alloc_t(c, miss_cap + 1, &a.miss));
    UKM_TRY(ws_alloc_t(c, miss_cap + 1, &a.miss_tax));
    a.miss_cap = miss_cap;
    a.files = (const u64 *const *)d_tab;
    a.lens = d_tab + S;
    a.cte = d_tab + 2 * (size_t)S;
    bool heavy = false;
    UKM_TRY(ukm_pu_probe_batches(c, a, S, tab.data() + S, lap, false, &heavy, [&](const PuArgs &b) {
        hipLaunchKernelGGL(pr_probe_kernel, dim3(b.R), dim3(PR_TNT), 0, c->stream, b, t);
    }));
    if (heavy) return UKM_OK;
    // (an all-ones code is the tables' empty marker: none of its records was folded into its base entry -- every one of
    //  them is in the list instead --, so the entry, the base set's last, stays out of the final union)
    u64 last = 0;
    UKM_TRY(ukm_read_u64(c, ctl, h, 2));
    c->stat_punion_flags = h[1];
    UKM_TRY(ukm_read_u64(c, base + n0 - 1, &last));
    if (lap.on) fprintf(stderr, "[punion/ranked] S=%d n0=%llu R=%u range=%u records=%llu listed=%llu (cap %llu) flags=%llu\n", S, (unsigned long long)n0,
                        a.R, a.range, (unsigned long long)total, (unsigned long long)h[0], (unsigned long long)miss_cap, (unsigned long long)h[1]);
    if (h[1] != 0) return UKM_OK;  // unsorted input / overflow: the general route reports or handles it
    const u64 n0e = last == PU_EMPTY ? n0 - 1 : n0;
    u32 *base_tax = nullptr;
    UKM_TRY(ws_alloc_t(c, n0 + 1, &base_tax));
    if (n0e) hipLaunchKernelGGL(pr_settle_kernel, dim3((unsigned)((n0e + 255) / 256)), dim3(256), 0, c->stream, t, a.tax, n0e, base_tax);
    UKM_HIP(hipGetLastError());
    lap("settle");
    return ukm_pu_finish(c, a, h[0], base, base_tax, n0e, o, lap, "list sort", declined);
}
