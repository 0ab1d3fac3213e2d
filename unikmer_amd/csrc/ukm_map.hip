// ukm_map.hip — k-mers back to genome coordinates on the GPU:
//   * ukm_locate: every occurrence of every queried code (locate.go:141-289: `m[code] = append(m[code], {seqIdx, Index})`
//     over all windows, then the .unik files in order, `delete(m, code)` after a code's first appearance);
//   * ukm_map: the successive regions covered by k-mers of a set (map.go:116-491 at -x 0 -X 0: a region is a maximal run of
//     windows whose code is in the set and, without -M, occurs once among the windows of its genome).
//
// Both are a JOIN of the genome's windows (run_windows, ukm_encode.hip; its kernels: ukm_win_kernels.h) against a sorted code array, done in genome order:
//   join_kernel   every window looks its code up through a PREFIX DIRECTORY of the sorted array (ukm_dir.h; dir[p] = lower bound of
//                 prefix p, 2^B + 1 words with B = log2(n) - 1: the bucket of a prefix holds 2-4 codes, one 128-byte line
//                 most of the time) -- one directory read and one or two reads of the array per window instead of the
//                 ~log2(n) dependent gathers of a whole binary search (every step of a per-lane search in an array
//                 beyond L2 is 64 scattered rows per wave).  It writes one flag byte per window and/or compacts the
//                 hits, in window order, with the library's look-back.
//   ukm_map       flags -> (without allow_multi: the HITS alone are compacted as (code, window), sorted by code with
//                 ukm_dev_sort, and classify_kernel takes the good bit from every hit whose sorted neighbour carries the same
//                 code in the same genome: all occurrences of a code hit together, so counting among the hits is counting
//                 among all windows; a set that covers little of the genome sorts little) -> mark_rec_kernel raises the
//                 "first window of a record" bit -> runs_kernel finds run starts and ends in one pass (the j-th start and
//                 the j-th end belong together: an end's slot is the number of starts up to it minus one, so ONE look-back
//                 over the start counts orders both) -> emit_kernel keeps the runs of at least min_len bases, compacted in
//                 order.
//   ukm_map_gapped  map.go:298-490 with -x / -X / --circular (definition: include/unikmer_hip.h): the same classes, a
//                 multiple-mapped hit marked F_MULTI; circular records: unroll_kernel writes the class bytes of the L
//                 circular windows out as the 2L - k + 1 positions of the record written twice; runs_kernel<GAPPED> also
//                 counts breaks (multiple-mapped positions, record starts) in its look-back word; chain_kernel joins runs
//                 across small gaps without a break; emit_gapped_kernel emits every group of max_gap_num + 1 runs of a chain.
//   ukm_locate    the queries are sorted stably with their indices (a code's first copy comes first, and the directory's
//                 lower bound finds exactly it); the join emits (index of that query, window) per hit in window order;
//                 a stable sort by query index is then the reference's output order, and expand_kernel turns window
//                 indices into (record, position).
// Against a LARGE sorted array (a set of 2^24 codes, 2^23 queries or more; option "map_sorted" 0 / 1 forces either way) both calls first sort ALL
// (code, window) pairs and look the array up in sorted order -- neighbouring lanes read neighbouring entries -- instead of
// gathering from genome order: ukm_map's sorted_classify_kernel scatters the flags back, ukm_locate's join emits the
// windows' own indices.  The measurements behind the threshold: DESIGN.md 4.14.
#include <algorithm>
#include <vector>

#include "ukm_device.h"
#include "ukm_dir.h"
#include "ukm_map.h"

namespace {

constexpr int NT = 256;
constexpr int VT = 8;            // consecutive windows per thread: their eight flag bytes are one 8-byte word
constexpr int TILE = NT * VT;
enum : u64 { MAP_FLAG_TIMEOUT = 4 };  // result word [1]
// flag byte of a window: good / first window of its record / in the set but multiple-mapped (ukm_map_gapped's class B;
// ukm_map reads F_GOOD alone, so a multiple-mapped hit is a miss to it)
enum : u32 { F_GOOD = 1, F_REC = 2, F_MULTI = 4 };

// first index in [0, n) with a[i] > x
__device__ __forceinline__ u64 upper_bound_u64(const u64 *a, u64 n, u64 x) {
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void iota_u32_kernel(u32 *v, u64 n) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) v[i] = (u32)i;
}

// ---- the join ---------------------------------------------------------------------------------------------------------
struct JoinArgs {
    const u64 *w;   // window values in genome order
    u64 n;
    Dir d;
    u8 *flag;       // (may be null) flag[i] = F_GOOD when w[i] is in d.keys; whole 8-byte words, zero behind n
    const u32 *wi;  // (COMPACT, may be null) w is sorted and wi[i] is the window it came from: emitted instead of i
    const u32 *qi;  // (COMPACT, may be null) the emitted key is qi[lower bound] instead of the code
    u64 *outk;      // COMPACT: hits in window order
    u32 *outv;      //          their window indices
    u64 out_cap;
    u64 *status;
    u32 *ticket;
    u64 *result;    // [0] number of hits, [1] flags
    u64 ntiles;
};

template <bool COMPACT, bool TICKET>
__global__ __launch_bounds__(NT) void join_kernel(JoinArgs p) {
    __shared__ u32 s_scan[NT / 64 + 1];
    __shared__ u64 s_misc[2];
    const int tid = (int)threadIdx.x, lane = lane_id();
    const u64 tile = COMPACT ? lb_tile_id<TICKET>(p.ticket, &s_misc[0]) : (u64)blockIdx.x;
    const u64 i0 = tile * (u64)TILE + (u64)tid * VT;
    u64 x[VT];
    u32 lo[VT];
    u32 valid = 0;
#pragma unroll
    for (int s = 0; s < VT; s++) {
        x[s] = (i0 + s < p.n) ? p.w[i0 + s] : 0;
        valid |= (i0 + s < p.n) ? 1u << s : 0u;
    }
    const u32 hit = dir_search_n<VT>(p.d, x, valid, lo);  // (ukm_dir.h: the eight searches side by side)
    if (p.flag && i0 < p.n) {
        u64 f8 = 0;
#pragma unroll
        for (int s = 0; s < VT; s++) f8 |= (u64)((hit >> s) & 1u) << (8 * s);
        *reinterpret_cast<u64 *>(p.flag + i0) = f8;
    }
    if (COMPACT) {
        u32 tot;
        const u32 excl = block_excl_scan_u32<NT>((u32)__popc(hit), s_scan, &tot);
        const u64 base = lb_tile_base<TICKET>(p.status, tile, (u64)tot, &p.result[1], MAP_FLAG_TIMEOUT, &s_misc[1], tid, lane);
        u64 pos = base + excl;
#pragma unroll
        for (int s = 0; s < VT; s++)
            if ((hit >> s) & 1u) {
                if (pos < p.out_cap) {
                    p.outk[pos] = p.qi ? (u64)p.qi[lo[s]] : x[s];
                    p.outv[pos] = p.wi ? p.wi[i0 + s] : (u32)(i0 + s);
                }
                pos++;
            }
        if (tid == 0 && tile == p.ntiles - 1) p.result[0] = base + tot;
    }
}

// ---- multiple-mapped codes --------------------------------------------------------------------------------------------
// two windows a <= b lie in one genome when no genome starts in (a, b]
struct Genomes {
    const u64 *gwin;  // [n_genome + 1] first window of every genome
    u64 n_genome;
};
__device__ __forceinline__ bool same_genome(const Genomes &g, u32 a, u32 b) {
    if (g.n_genome <= 1) return true;
    return upper_bound_u64(g.gwin, g.n_genome + 1, a) == upper_bound_u64(g.gwin, g.n_genome + 1, b);
}
__global__ void genome_windows_kernel(const u64 *genome_off, const u64 *win_off, u64 n_genome, u64 *gwin) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g <= n_genome) gwin[g] = win_off[genome_off[g]];
}
// (hk, hv) sorted by code, equal codes by window: does a neighbour carry the same code in the same genome?
__device__ __forceinline__ bool multi_mapped(const u64 *hk, const u32 *hv, u64 n, u64 j, const Genomes &g) {
    const u64 code = hk[j];
    const u32 w = hv[j];
    if (j > 0 && hk[j - 1] == code && same_genome(g, hv[j - 1], w)) return true;
    return j + 1 < n && hk[j + 1] == code && same_genome(g, w, hv[j + 1]);
}
// the hits alone, sorted: the multiple-mapped ones are no longer good
__global__ void classify_kernel(const u64 *hk, const u32 *hv, u64 n, Genomes g, u8 *flag) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n && multi_mapped(hk, hv, n, j, g)) flag[hv[j]] = (u8)F_MULTI;
}
// option map_sorted: ALL windows sorted; membership in sorted order, every flag scattered back
__global__ void sorted_classify_kernel(const u64 *hk, const u32 *hv, u64 n, Dir d, Genomes g, int allow_multi, u8 *flag) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const u64 code = hk[j];
    const u32 lb = dir_lower_bound(d, code);
    const bool hit = (u64)lb < d.n && d.keys[lb] == code;
    const bool multi = hit && !allow_multi && multi_mapped(hk, hv, n, j, g);
    flag[hv[j]] = !hit ? (u8)0 : multi ? (u8)F_MULTI : (u8)F_GOOD;
}

__global__ void mark_rec_kernel(const u64 *win_off, u64 n_rec, u8 *flag) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_rec && win_off[r + 1] > win_off[r]) flag[win_off[r]] |= (u8)F_REC;
}

// ---- runs of good windows ---------------------------------------------------------------------------------------------
struct RunArgs {
    const u8 *flag;  // whole 8-byte words, zero behind n
    u64 n;
    u32 *start, *end;  // [cap] first / last window of every run
    u32 *brk;          // (GAPPED) [cap] breaks up to and including every run's first position
    u64 cap;
    u64 *status;
    u32 *ticket;
    u64 *result;  // [0] number of runs, [1] flags
    u64 ntiles;
};

// GAPPED (ukm_map_gapped): the running count of BREAKS -- positions that are multiple-mapped (F_MULTI) or the first of
// their record (F_REC) -- rides in the same look-back word, run starts in bits [30:0], breaks in [61:31] (fewer than
// 2^31 positions per call, so neither field overflows), and every run keeps the count at its first position.  No break
// lies inside a run behind that position (a good window is not multiple-mapped, a record's first window starts a run),
// so the count at a run's end is the same number: two neighbouring runs have a break between them exactly when their
// counts differ, whatever the length of the gap.
template <bool TICKET, bool GAPPED>
__global__ __launch_bounds__(NT) void runs_kernel(RunArgs p) {
    __shared__ u32 s_scan[NT / 64 + 1];
    __shared__ u64 s_misc[2];
    const int tid = (int)threadIdx.x, lane = lane_id();
    const u64 tile = lb_tile_id<TICKET>(p.ticket, &s_misc[0]);
    const u64 i0 = tile * (u64)TILE + (u64)tid * VT;
    const bool in = i0 < p.n;
    const u64 f8 = in ? *reinterpret_cast<const u64 *>(p.flag + i0) : 0;
    u32 prev = (in && i0 > 0) ? p.flag[i0 - 1] : 0;
    const u32 next = (i0 + VT < p.n) ? p.flag[i0 + VT] : 0;
    u32 starts = 0, ends = 0, brks = 0;
#pragma unroll
    for (int s = 0; s < VT; s++) {
        const u32 f = (u32)(f8 >> (8 * s)) & 0xFFu;
        const u32 nf = s + 1 < VT ? (u32)(f8 >> (8 * (s + 1))) & 0xFFu : next;
        const bool good = (f & F_GOOD) != 0;
        if (good && ((f & F_REC) || !(prev & F_GOOD))) starts |= 1u << s;
        if (good && (!(nf & F_GOOD) || (nf & F_REC))) ends |= 1u << s;
        if (GAPPED && (f & (F_MULTI | F_REC))) brks |= 1u << s;
        prev = f;
    }
    // (one block scan for both counts: at most 2048 of either per tile)
    u32 tot;
    const u32 excl = block_excl_scan_u32<NT>((u32)__popc(starts) | (GAPPED ? (u32)__popc(brks) << 16 : 0u), s_scan, &tot);
    const u64 agg = GAPPED ? ((u64)(tot >> 16) << 31) | (u64)(tot & 0xFFFFu) : (u64)tot;
    const u64 base = lb_tile_base<TICKET>(p.status, tile, agg, &p.result[1], MAP_FLAG_TIMEOUT, &s_misc[1], tid, lane);
    u64 slot = (GAPPED ? base & 0x7FFFFFFFull : base) + (GAPPED ? excl & 0xFFFFu : excl);  // runs that started in front of this thread's windows
    u32 nb = GAPPED ? (u32)(base >> 31) + (excl >> 16) : 0u;                                 // breaks in front of them
#pragma unroll
    for (int s = 0; s < VT; s++) {
        if (GAPPED) nb += (brks >> s) & 1u;
        if ((starts >> s) & 1u) {
            if (slot < p.cap) {
                p.start[slot] = (u32)(i0 + s);
                if (GAPPED) p.brk[slot] = nb;
            }
            slot++;
        }
        // an end closes the most recent start: slot - 1 (>= 0: a good window has a start at or in front of it)
        if (((ends >> s) & 1u) && slot >= 1 && slot - 1 < p.cap) p.end[slot - 1] = (u32)(i0 + s);
    }
    if (tid == 0 && tile == p.ntiles - 1) p.result[0] = (GAPPED ? (base + agg) & 0x7FFFFFFFull : base + agg);
}

struct EmitArgs {
    const u32 *start, *end;
    u64 nruns;
    const u64 *win_off;  // [n_rec + 1]
    u64 n_rec;
    int k;
    u64 min_len;
    u32 *out_rec;
    u64 *out_start, *out_end;
    u64 out_cap;
    u64 *status;
    u32 *ticket;
    u64 *result;
    u64 ntiles;
};

// one run per thread: map.go's `lastmatch - start + k >= minLen`, survivors in order
template <bool TICKET>
__global__ __launch_bounds__(NT) void emit_kernel(EmitArgs p) {
    __shared__ u32 s_scan[NT / 64 + 1];
    __shared__ u64 s_misc[2];
    const int tid = (int)threadIdx.x, lane = lane_id();
    const u64 tile = lb_tile_id<TICKET>(p.ticket, &s_misc[0]);
    const u64 j = tile * (u64)NT + (u64)tid;
    u64 s = 0, e = 0;
    bool keep = false;
    if (j < p.nruns) {
        s = p.start[j];
        e = p.end[j];
        keep = e - s + (u64)p.k >= p.min_len;
    }
    u32 tot;
    const u32 excl = block_excl_scan_u32<NT>(keep ? 1u : 0u, s_scan, &tot);
    const u64 base = lb_tile_base<TICKET>(p.status, tile, (u64)tot, &p.result[1], MAP_FLAG_TIMEOUT, &s_misc[1], tid, lane);
    const u64 pos = base + excl;
    if (keep && pos < p.out_cap) {
        const u64 r = upper_bound_u64(p.win_off, p.n_rec + 1, s) - 1;  // (records without windows share their offset with the next one)
        const u64 w0 = p.win_off[r];
        p.out_rec[pos] = (u32)r;
        p.out_start[pos] = s - w0;
        p.out_end[pos] = e - w0 + (u64)p.k;
    }
    if (tid == 0 && tile == p.ntiles - 1) p.result[0] = base + tot;
}

// ---- ukm_map_gapped: the stream of a circular record, chains of runs, regions -------------------------------------------
// A record of L >= k bases has 2L - k + 1 stream positions when circular (the windows of the record written twice,
// map.go:338-340), none when it is shorter than k.
__global__ void stream_count_kernel(const u64 *rec_off, u64 n_rec, int k, u64 *cnt) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rec) return;
    const u64 len = r < n_rec ? rec_off[r + 1] - rec_off[r] : 0;
    cnt[r] = len < (u64)k ? 0 : 2 * len - (u64)k + 1;
}

// Class bytes of the circular windows (cls, L per record at win_off) -> flag bytes of the stream (2L - k + 1 per record
// at soff): position i of a record carries the class of circular window i mod L, position 0 also F_REC.  Eight
// positions = one 8-byte word per thread, zero behind n.
__global__ __launch_bounds__(NT) void unroll_kernel(const u8 *cls, const u64 *win_off, const u64 *soff, u64 n_rec, u64 n, u8 *flag) {
    const u64 p0 = ((u64)blockIdx.x * NT + threadIdx.x) * VT;
    if (p0 >= n) return;
    u64 r = upper_bound_u64(soff, n_rec + 1, p0) - 1;  // (records without positions share their offset with the next one)
    u64 s0 = soff[r], s1 = soff[r + 1], w0 = win_off[r], len = win_off[r + 1] - w0;
    u64 f8 = 0;
#pragma unroll
    for (int s = 0; s < VT; s++) {
        const u64 p = p0 + s;
        if (p >= n) break;
        while (p >= s1) {  // (p < n = soff[n_rec]: ends at a record with positions)
            r++;
            s0 = s1; s1 = soff[r + 1]; w0 = win_off[r]; len = win_off[r + 1] - w0;
        }
        const u64 i = p - s0;
        const u32 f = (u32)cls[w0 + (i >= len ? i - len : i)] | (i == 0 ? (u32)F_REC : 0u);
        f8 |= (u64)f << (8 * s);
    }
    *reinterpret_cast<u64 *>(flag + p0) = f8;
}

// One run per thread.  The separator in front of run j is HARD when j is the first run, when more than max_gap_size
// positions lie between the two runs, or when a break does (a multiple-mapped window, or the start of a record: the
// break counts of the two runs differ).  A chain = a hard run and the soft ones behind it: cid[j] = hard runs up to and
// including j, minus one; heads[c] = first run of chain c, heads[number of chains] = nruns.
struct ChainArgs {
    const u32 *start, *end, *brk;
    u64 nruns;
    u64 max_gap_size;
    u32 *cid;    // [nruns]
    u32 *heads;  // [nruns + 1]
    u64 *status;
    u32 *ticket;
    u64 *result;  // [0] number of chains, [1] flags
    u64 ntiles;
};

template <bool TICKET>
__global__ __launch_bounds__(NT) void chain_kernel(ChainArgs p) {
    __shared__ u32 s_scan[NT / 64 + 1];
    __shared__ u64 s_misc[2];
    const int tid = (int)threadIdx.x, lane = lane_id();
    const u64 tile = lb_tile_id<TICKET>(p.ticket, &s_misc[0]);
    const u64 j = tile * (u64)NT + (u64)tid;
    bool hard = false;
    if (j < p.nruns)
        hard = j == 0 || p.brk[j] != p.brk[j - 1] || (u64)(p.start[j] - p.end[j - 1] - 1u) > p.max_gap_size;
    u32 tot;
    const u32 excl = block_excl_scan_u32<NT>(hard ? 1u : 0u, s_scan, &tot);
    const u64 base = lb_tile_base<TICKET>(p.status, tile, (u64)tot, &p.result[1], MAP_FLAG_TIMEOUT, &s_misc[1], tid, lane);
    if (j < p.nruns) {
        const u64 c = base + excl + (hard ? 1u : 0u) - 1;  // (run 0 is hard: never negative)
        p.cid[j] = (u32)c;
        if (hard) p.heads[c] = (u32)j;
    }
    if (tid == 0 && tile == p.ntiles - 1) {
        p.result[0] = base + tot;
        p.heads[base + tot] = (u32)p.nruns;
    }
}

struct EmitGappedArgs {
    const u32 *start, *end, *cid, *heads;
    u64 nruns;
    const u64 *soff;     // [n_rec + 1] first stream position of every record
    const u64 *rec_off;  // [n_rec + 1]
    u64 n_rec;
    int k, circular;
    u64 min_len;
    u64 max_gap_num;
    u32 *out_rec;
    u64 *out_start, *out_end;
    u64 out_cap;
    u64 *status;
    u32 *ticket;
    u64 *result;
    u64 ntiles;
};

// One run per thread.  Inside a chain the state machine of map.go:362-489 closes a region at the (X + 1)-th small gap,
// X = max_gap_num, and opens the next one at the run behind that gap: the regions are the groups of X + 1 consecutive
// runs counted from the chain's head, the last group cut at the chain's end.  A run that heads a group emits it.
template <bool TICKET>
__global__ __launch_bounds__(NT) void emit_gapped_kernel(EmitGappedArgs p) {
    __shared__ u32 s_scan[NT / 64 + 1];
    __shared__ u64 s_misc[2];
    const int tid = (int)threadIdx.x, lane = lane_id();
    const u64 tile = lb_tile_id<TICKET>(p.ticket, &s_misc[0]);
    const u64 j = tile * (u64)NT + (u64)tid;
    u64 r = 0, s = 0, e = 0;
    bool keep = false;
    if (j < p.nruns) {
        const u32 c = p.cid[j];
        if ((j - (u64)p.heads[c]) % (p.max_gap_num + 1) == 0) {
            const u64 chain_last = (u64)p.heads[c + 1] - 1;
            const u64 last = j + p.max_gap_num < chain_last ? j + p.max_gap_num : chain_last;
            const u64 first_pos = p.start[j];
            const u64 span = (u64)p.end[last] - first_pos + (u64)p.k;  // lastmatch - start + k
            r = upper_bound_u64(p.soff, p.n_rec + 1, first_pos) - 1;
            s = first_pos - p.soff[r];
            e = s + span;
            keep = span >= p.min_len;
            if (p.circular) {
                const u64 len = p.rec_off[r + 1] - p.rec_off[r];
                if (s >= len) keep = false;    // a start in the second copy (map.go:407/423)
                if (span > len) e = s + len;   // longer than the record itself (map.go:381)
            }
        }
    }
    u32 tot;
    const u32 excl = block_excl_scan_u32<NT>(keep ? 1u : 0u, s_scan, &tot);
    const u64 base = lb_tile_base<TICKET>(p.status, tile, (u64)tot, &p.result[1], MAP_FLAG_TIMEOUT, &s_misc[1], tid, lane);
    const u64 pos = base + excl;
    if (keep && pos < p.out_cap) {
        p.out_rec[pos] = (u32)r;
        p.out_start[pos] = s;
        p.out_end[pos] = e;
    }
    if (tid == 0 && tile == p.ntiles - 1) p.result[0] = base + tot;
}

// ukm_locate: hits sorted by query index -> (query, record, position)
__global__ void expand_kernel(const u64 *hk, const u32 *hv, u64 n, const u64 *win_off, u64 n_rec, u64 *out_q, u32 *out_rec,
                              u64 *out_pos) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const u64 w = hv[e];
    const u64 r = upper_bound_u64(win_off, n_rec + 1, w) - 1;
    out_q[e] = hk[e];
    out_rec[e] = (u32)r;
    out_pos[e] = w - win_off[r];
}

// ---- host steps -------------------------------------------------------------------------------------------------------
unsigned blocks_for(u64 n) { return (unsigned)((n + NT - 1) / NT); }

// flag: n rounded up to whole tiles (the kernels read and write 8-byte words)
size_t flag_bytes(u64 n) { return (size_t)((n + TILE - 1) / TILE * TILE + 8); }

int run_join(ukm_ctx *c, const u64 *w, const u32 *wi, u64 n, const Dir &d, u8 *flag, const u32 *qi, bool compact, u64 *outk, u32 *outv,
             u64 out_cap, u64 *n_hits) {
    JoinArgs p;
    memset(&p, 0, sizeof(p));
    p.w = w; p.wi = wi; p.n = n; p.d = d; p.flag = flag; p.qi = qi; p.outk = outk; p.outv = outv; p.out_cap = out_cap;
    p.ntiles = (n + TILE - 1) / TILE;
    *n_hits = 0;
    if (!compact) {
        (void)hipEventRecord(c->ev_k0, c->stream);
        hipLaunchKernelGGL((join_kernel<false, false>), dim3((unsigned)p.ntiles), dim3(NT), 0, c->stream, p);
        (void)hipEventRecord(c->ev_k1, c->stream);
        c->evk_valid = true;
        UKM_HIP(hipGetLastError());
        return UKM_OK;
    }
    LbCtl blk;
    UKM_TRY(ukm_lb_ctl_alloc(c, p.ntiles, 0, &blk));
    p.status = blk.status; p.ticket = blk.ticket; p.result = blk.result;
    u64 res[2] = {0, 0};
    const LbLaunch how = {"window join", "window join kernel", MAP_FLAG_TIMEOUT, true, false, false};
    UKM_TRY(ukm_lb_launch(c, blk, how, [&](bool ticket) {
        if (ticket) hipLaunchKernelGGL((join_kernel<true, true>), dim3((unsigned)p.ntiles), dim3(NT), 0, c->stream, p);
        else hipLaunchKernelGGL((join_kernel<true, false>), dim3((unsigned)p.ntiles), dim3(NT), 0, c->stream, p);
        return UKM_OK;
    }, res));
    *n_hits = res[0];
    return UKM_OK;
}

}  // namespace

// ---- host steps shared with ukm_screen.hip (declared in ukm_map.h) -------------------------------------------------------
// log2 of the codes per prefix of the directory (developer knob; 1 / 2 / 3 measured: DESIGN.md 4.14)
int ukm_map_dir_slack(const ukm_ctx *c) { return ukm_env_int(c, "UKM_MAP_DIR_SLACK", DIR_SLACK_DEFAULT); }

// Route policy: a window's lookup in genome order is a gather into the sorted array.  While the array
// (and its directory) stays near the caches that is the cheapest membership there is; against an array of hundreds of MB
// every lookup is an HBM row, and sorting the (code, window) pairs first -- neighbouring lanes then read neighbouring
// entries -- costs less than the gathers it saves.  Option "map_sorted" 0 / 1 forces either.
// Measured at 1e8 windows: ukm_map 1e7 codes 5.6 (genome order) against 6.1 ms (sorted), 1e8 codes 9.6 against 7.3;
// ukm_locate, whose join also compacts, 1e7 queries 5.7 against 4.9.  (The thresholds: ukm_map.h.)
bool ukm_map_sorted_route(const ukm_ctx *c, u64 n_keys, u64 min_keys) {
    const char *e = ukm_env(c, "UKM_MAP_SORTED");
    if (e && *e) return e[0] == '1';
    return n_keys >= min_keys;
}
// (w, wi) = every window and its index, sorted by code (stably: equal codes by window)
int ukm_dev_sort_windows(ukm_ctx *c, u64 *w, u64 n, int key_bits, u32 **wi) {
    UKM_TRY(ws_alloc_t(c, n, wi));
    hipLaunchKernelGGL(iota_u32_kernel, dim3(std::min(blocks_for(n), (unsigned)c->num_cu * 16u)), dim3(NT), 0, c->stream, *wi, n);
    return ukm_dev_sort(c, w, *wi, n, key_bits);
}

// what every entry point does first: stage the records, produce the windows
int ukm_dev_make_windows(ukm_ctx *c, const char *name, const u8 *bases, const u64 *rec_off, u64 n_rec, int k, int canonical, int circular,
                         int hashed, MapWindows *W) {
    u64 total_bases = 0;
    const u8 *b = nullptr;
    UKM_TRY(ukm_dev_stage_records(c, name, bases, rec_off, n_rec, &W->rec_off, &b, &total_bases));
    UKM_TRY(ws_alloc_t(c, (size_t)total_bases + 1, &W->w));
    UKM_TRY(ukm_dev_windows(c, hashed != 0, b, W->rec_off, n_rec, k, canonical, circular, W->w, total_bases + 1, &W->n, total_bases, &W->win_off));
    if (W->n >= (1ull << 32))
        UKM_FAIL(UKM_ERR_INVALID, "%s: %llu windows in one call; the limit is 2^32 - 1 (window indices are the 32-bit payload of the pair sort): "
                 "split the records over several calls", name, (unsigned long long)W->n);
    return UKM_OK;
}

namespace {

int check_args(const char *name, const void *ctx, const void *n_out, const void *bases, const void *rec_off, u64 n_rec, int k, int hashed) {
    if (!ctx || !n_out || (n_rec && (!rec_off || !bases))) UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
    if (k < 1 || k > (hashed ? 64 : 32)) UKM_FAIL(UKM_ERR_K, "%s: k = %d out of range", name, k);
    return UKM_OK;
}

}  // namespace

extern "C" int ukm_locate(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off, uint64_t n_rec, int k, int circular,
                          int hashed, const uint64_t *q_keys, uint64_t nq, uint64_t *out_q, uint32_t *out_rec,
                          uint64_t *out_pos, uint64_t out_cap, uint64_t *n_out) {
    const char *name = "ukm_locate";
    UKM_TRY(check_args(name, ctx, n_out, bases, rec_off, n_rec, k, hashed));
    if ((nq && !q_keys) || (out_cap && (!out_q || !out_rec || !out_pos))) UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
    if (nq >= (1ull << 32)) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu queries; the limit is 2^32 - 1", name, (unsigned long long)nq);
    *n_out = 0;
    if (n_rec == 0) return UKM_OK;
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        u64 *oq = nullptr, *op = nullptr;
        u32 *orec = nullptr;
        UKM_TRY(ukm_out_t(ctx, out_q, out_cap, &oq));
        UKM_TRY(ukm_out_t(ctx, out_rec, out_cap, &orec));
        UKM_TRY(ukm_out_t(ctx, out_pos, out_cap, &op));
        auto sizes = [&](u64 n) {
            ukm_out_resize(ctx, out_q, n * sizeof(u64));
            ukm_out_resize(ctx, out_rec, n * sizeof(u32));
            ukm_out_resize(ctx, out_pos, n * sizeof(u64));
        };
        const int r = [&]() -> int {
        MapWindows W;
        UKM_TRY(ukm_dev_make_windows(ctx, name, bases, rec_off, n_rec, k, 1, circular, hashed, &W));  // (also without queries: an illegal base is an error)
        if (W.n == 0 || nq == 0) return UKM_OK;
        // the queries, sorted stably with their indices (all 64 bits: they are the caller's, not ours)
        u64 *qs = nullptr;
        u32 *qi = nullptr;
        UKM_TRY(ws_alloc_t(ctx, nq, &qs));
        UKM_TRY(ws_alloc_t(ctx, nq, &qi));
        UKM_HIP(hipMemcpyAsync(qs, q_keys, nq * sizeof(u64), ukm_is_device_ptr(q_keys) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(iota_u32_kernel, dim3(std::min(blocks_for(nq), (unsigned)ctx->num_cu * 16u)), dim3(NT), 0, ctx->stream, qi, nq);
        UKM_TRY(ukm_dev_sort(ctx, qs, qi, nq, 64));
        Dir d;
        UKM_TRY(build_dir(ctx, qs, nq, hashed ? 64 : 2 * k, ukm_map_dir_slack(ctx), &d));
        // hits in window order.  The caller's capacity bounds the first attempt's buffers (a host that asks for a few
        // positions pays for a few); more hits than that: the exact number goes back with UKM_ERR_CAPACITY
        const u64 hcap = std::min<u64>(W.n, out_cap);
        u64 *hk = nullptr;
        u32 *hv = nullptr;
        UKM_TRY(ws_alloc_t(ctx, hcap + 1, &hk));
        UKM_TRY(ws_alloc_t(ctx, hcap + 1, &hv));
        u64 nh = 0;
        u32 *wi = nullptr;  // (sorted route: the hits then come by code, a code's windows ascending; the sort below keeps that)
        if (ukm_map_sorted_route(ctx, nq, LOCATE_SORTED_MIN_KEYS)) UKM_TRY(ukm_dev_sort_windows(ctx, W.w, W.n, hashed ? 64 : 2 * k, &wi));
        UKM_TRY(run_join(ctx, W.w, wi, W.n, d, nullptr, qi, true, hk, hv, hcap, &nh));
        *n_out = nh;
        if (nh > out_cap)
            UKM_FAIL(UKM_ERR_CAPACITY, "%s: output needs %llu entries, capacity is %llu", name, (unsigned long long)nh, (unsigned long long)out_cap);
        if (nh == 0) return UKM_OK;
        int qbits = 1;
        while (qbits < 64 && (nq >> qbits) != 0) qbits++;
        UKM_TRY(ukm_dev_sort(ctx, hk, hv, nh, qbits));  // stable: a query's windows stay ascending
        hipLaunchKernelGGL(expand_kernel, dim3(blocks_for(nh)), dim3(NT), 0, ctx->stream, hk, hv, nh, W.win_off, n_rec, oq, orec, op);
        UKM_HIP(hipGetLastError());
        return UKM_OK;
        }();
        sizes(r == UKM_OK ? *n_out : 0);  // (the copy-back of host outputs: what was written, nothing after an error)
        return r;
    }();
    return ukm_finish(&s, rc);
}

// ---- ukm_map / ukm_map_gapped -------------------------------------------------------------------------------------------
namespace {

// one look-back launch over `ntiles` tiles: control block, the watchdog ladder, result word [0]
template <typename Args, typename Launch>
int lb_pass(ukm_ctx *c, const char *name, const char *kernel_name, Args &p, u64 ntiles, Launch launch, u64 *count) {
    p.ntiles = ntiles;
    LbCtl blk;
    UKM_TRY(ukm_lb_ctl_alloc(c, ntiles, 0, &blk));
    p.status = blk.status; p.ticket = blk.ticket; p.result = blk.result;
    u64 res[2] = {0, 0};
    const LbLaunch how = {name, kernel_name, MAP_FLAG_TIMEOUT, false, false, false};
    UKM_TRY(ukm_lb_launch(c, blk, how, [&](bool ticket) {
        launch(ticket);
        return UKM_OK;
    }, res));
    *count = res[0];
    return UKM_OK;
}

struct MapOpts {
    int circular = 0;
    u64 max_gap_size = 0, max_gap_num = 0;
};

// Everything behind the argument checks.  Without gaps and on linear records a region is a run (runs_kernel, emit_kernel);
// otherwise the runs of the stream are chained and grouped (runs_kernel with break counts, chain_kernel, emit_gapped_kernel).
int map_regions(ukm_ctx *ctx, const char *name, const u8 *bases, const u64 *rec_off, u64 n_rec, const u64 *genome_off, u64 n_genome,
                int k, int hashed, const u64 *set_keys, u64 n_set, int allow_multi, u64 min_len, const MapOpts &o, u32 *orec,
                u64 *ostart, u64 *oend, u64 out_cap, u64 *n_out) {
    // genome_off: checked on the host (it is small), used on the device
    const u64 *goff = nullptr;
    UKM_TRY(ukm_in_t(ctx, genome_off, n_genome + 1, &goff));
    {
        std::vector<u64> gh(n_genome + 1);
        if (ukm_is_device_ptr(genome_off)) {
            UKM_HIP(hipMemcpyAsync(gh.data(), goff, gh.size() * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
            UKM_HIP(hipStreamSynchronize(ctx->stream));
        } else {
            memcpy(gh.data(), genome_off, gh.size() * sizeof(u64));
        }
        bool ok = gh[0] == 0 && gh[n_genome] == n_rec;
        for (u64 g = 0; ok && g < n_genome; g++) ok = gh[g] <= gh[g + 1];
        if (!ok) UKM_FAIL(UKM_ERR_INVALID, "%s: genome_off must rise from 0 to n_rec", name);
    }
    const u64 *set = nullptr;
    UKM_TRY(ukm_in_t(ctx, set_keys, n_set, &set));
    bool sorted = true, strict = true;
    UKM_TRY(ukm_dev_check_sorted(ctx, set, n_set, &sorted, &strict));
    if (!sorted) UKM_FAIL(UKM_ERR_UNSORTED, "%s: the code set is not sorted", name);
    MapWindows W;  // (circular: the L circular windows of every record, the ones map.go:222-226 counts multiplicity among)
    UKM_TRY(ukm_dev_make_windows(ctx, name, bases, rec_off, n_rec, k, 1, o.circular, hashed, &W));
    if (W.n == 0 || n_set == 0) return UKM_OK;
    const bool plain = !o.circular && o.max_gap_size == 0;
    if (!plain && !o.circular && W.n >= (1ull << 31))
        UKM_FAIL(UKM_ERR_INVALID, "%s: %llu stream positions in one call; the limit is 2^31 - 1 (run and break counts share one "
                 "look-back word): split the records over several calls", name, (unsigned long long)W.n);
    const int key_bits = hashed ? 64 : 2 * k;
    Dir d;
    UKM_TRY(build_dir(ctx, set, n_set, key_bits, ukm_map_dir_slack(ctx), &d));
    u8 *flag = nullptr;
    UKM_TRY(ws_alloc_t(ctx, flag_bytes(W.n), &flag));
    Genomes G = {nullptr, n_genome};
    if (!allow_multi && n_genome > 1) {
        u64 *gwin = nullptr;
        UKM_TRY(ws_alloc_t(ctx, n_genome + 1, &gwin));
        hipLaunchKernelGGL(genome_windows_kernel, dim3(blocks_for(n_genome + 1)), dim3(NT), 0, ctx->stream, goff, W.win_off, n_genome, gwin);
        G.gwin = gwin;
    }
    if (ukm_map_sorted_route(ctx, n_set, MAP_SORTED_MIN_KEYS)) {
        // every (code, window) pair sorted, the set looked up in sorted order, the flags scattered back
        u32 *wi = nullptr;
        UKM_TRY(ukm_dev_sort_windows(ctx, W.w, W.n, key_bits, &wi));
        UKM_HIP(hipMemsetAsync(flag, 0, flag_bytes(W.n), ctx->stream));
        (void)hipEventRecord(ctx->ev_k0, ctx->stream);
        hipLaunchKernelGGL(sorted_classify_kernel, dim3(blocks_for(W.n)), dim3(NT), 0, ctx->stream, W.w, wi, W.n, d, G, allow_multi, flag);
        (void)hipEventRecord(ctx->ev_k1, ctx->stream);
        ctx->evk_valid = true;
        UKM_HIP(hipGetLastError());
    } else if (allow_multi) {
        u64 nh = 0;
        UKM_TRY(run_join(ctx, W.w, nullptr, W.n, d, flag, nullptr, false, nullptr, nullptr, 0, &nh));
    } else {
        // the hits, sorted by code: a multiple-mapped code's occurrences are neighbours
        u64 *hk = nullptr;
        u32 *hv = nullptr;
        UKM_TRY(ws_alloc_t(ctx, W.n, &hk));
        UKM_TRY(ws_alloc_t(ctx, W.n, &hv));
        u64 nh = 0;
        UKM_TRY(run_join(ctx, W.w, nullptr, W.n, d, flag, nullptr, true, hk, hv, W.n, &nh));
        if (nh > 1) {
            UKM_TRY(ukm_dev_sort(ctx, hk, hv, nh, key_bits));
            hipLaunchKernelGGL(classify_kernel, dim3(blocks_for(nh)), dim3(NT), 0, ctx->stream, hk, hv, nh, G, flag);
            UKM_HIP(hipGetLastError());
        }
    }
    // the stream the runs are found on: the windows themselves, or every circular record's windows written out twice
    const u64 *soff = W.win_off;
    u64 ns = W.n;
    if (o.circular) {
        u64 *cnt = nullptr, *so = nullptr, *total_dev = nullptr;
        UKM_TRY(ws_alloc_t(ctx, n_rec + 1, &cnt));
        UKM_TRY(ws_alloc_t(ctx, n_rec + 1, &so));
        UKM_TRY(ws_alloc_t(ctx, 1, &total_dev));
        hipLaunchKernelGGL(stream_count_kernel, dim3(blocks_for(n_rec + 1)), dim3(NT), 0, ctx->stream, W.rec_off, n_rec, k, cnt);
        UKM_TRY(ukm_dev_exclusive_scan_u64(ctx, cnt, so, n_rec + 1, total_dev));
        UKM_TRY(ukm_read_u64(ctx, total_dev, &ns));
        if (ns >= (1ull << 31))
            UKM_FAIL(UKM_ERR_INVALID, "%s: %llu stream positions in one call (2L - k + 1 per circular record); the limit is 2^31 - 1 "
                     "(run and break counts share one look-back word): split the records over several calls", name, (unsigned long long)ns);
        u8 *sflag = nullptr;
        UKM_TRY(ws_alloc_t(ctx, flag_bytes(ns), &sflag));
        hipLaunchKernelGGL(unroll_kernel, dim3((unsigned)((ns + TILE - 1) / TILE)), dim3(NT), 0, ctx->stream, flag, W.win_off, so, n_rec, ns, sflag);
        UKM_HIP(hipGetLastError());
        flag = sflag;
        soff = so;
    } else {
        hipLaunchKernelGGL(mark_rec_kernel, dim3(blocks_for(n_rec)), dim3(NT), 0, ctx->stream, W.win_off, n_rec, flag);
        UKM_HIP(hipGetLastError());
    }
    // run starts and ends (records of one good window each: as many runs as positions)
    const u64 rcap = ns;
    u32 *rs = nullptr, *re = nullptr, *rb = nullptr;
    UKM_TRY(ws_alloc_t(ctx, rcap, &rs));
    UKM_TRY(ws_alloc_t(ctx, rcap, &re));
    if (!plain) UKM_TRY(ws_alloc_t(ctx, rcap, &rb));
    u64 nruns = 0;
    {
        RunArgs p;
        memset(&p, 0, sizeof(p));
        p.flag = flag; p.n = ns; p.start = rs; p.end = re; p.brk = rb; p.cap = rcap;
        const unsigned nt = (unsigned)((ns + TILE - 1) / TILE);
        UKM_TRY(lb_pass(ctx, name, "run kernel", p, nt, [&](bool ticket) {
            if (plain) {
                if (ticket) hipLaunchKernelGGL((runs_kernel<true, false>), dim3(nt), dim3(NT), 0, ctx->stream, p);
                else hipLaunchKernelGGL((runs_kernel<false, false>), dim3(nt), dim3(NT), 0, ctx->stream, p);
            } else {
                if (ticket) hipLaunchKernelGGL((runs_kernel<true, true>), dim3(nt), dim3(NT), 0, ctx->stream, p);
                else hipLaunchKernelGGL((runs_kernel<false, true>), dim3(nt), dim3(NT), 0, ctx->stream, p);
            }
        }, &nruns));
    }
    if (nruns == 0) return UKM_OK;
    const unsigned rt = (unsigned)((nruns + NT - 1) / NT);
    if (plain) {
        EmitArgs p;
        memset(&p, 0, sizeof(p));
        p.start = rs; p.end = re; p.nruns = nruns; p.win_off = W.win_off; p.n_rec = n_rec; p.k = k; p.min_len = min_len;
        p.out_rec = orec; p.out_start = ostart; p.out_end = oend; p.out_cap = out_cap;
        UKM_TRY(lb_pass(ctx, name, "region kernel", p, rt, [&](bool ticket) {
            if (ticket) hipLaunchKernelGGL((emit_kernel<true>), dim3(rt), dim3(NT), 0, ctx->stream, p);
            else hipLaunchKernelGGL((emit_kernel<false>), dim3(rt), dim3(NT), 0, ctx->stream, p);
        }, n_out));
    } else {
        u32 *cid = nullptr, *heads = nullptr;
        UKM_TRY(ws_alloc_t(ctx, nruns, &cid));
        UKM_TRY(ws_alloc_t(ctx, nruns + 1, &heads));
        u64 nchains = 0;
        {
            ChainArgs p;
            memset(&p, 0, sizeof(p));
            p.start = rs; p.end = re; p.brk = rb; p.nruns = nruns; p.max_gap_size = o.max_gap_size; p.cid = cid; p.heads = heads;
            UKM_TRY(lb_pass(ctx, name, "chain kernel", p, rt, [&](bool ticket) {
                if (ticket) hipLaunchKernelGGL((chain_kernel<true>), dim3(rt), dim3(NT), 0, ctx->stream, p);
                else hipLaunchKernelGGL((chain_kernel<false>), dim3(rt), dim3(NT), 0, ctx->stream, p);
            }, &nchains));
        }
        EmitGappedArgs p;
        memset(&p, 0, sizeof(p));
        p.start = rs; p.end = re; p.cid = cid; p.heads = heads; p.nruns = nruns; p.soff = soff; p.rec_off = W.rec_off; p.n_rec = n_rec;
        p.k = k; p.circular = o.circular; p.min_len = min_len; p.max_gap_num = o.max_gap_size ? o.max_gap_num : 0;
        p.out_rec = orec; p.out_start = ostart; p.out_end = oend; p.out_cap = out_cap;
        UKM_TRY(lb_pass(ctx, name, "gapped region kernel", p, rt, [&](bool ticket) {
            if (ticket) hipLaunchKernelGGL((emit_gapped_kernel<true>), dim3(rt), dim3(NT), 0, ctx->stream, p);
            else hipLaunchKernelGGL((emit_gapped_kernel<false>), dim3(rt), dim3(NT), 0, ctx->stream, p);
        }, n_out));
    }
    if (*n_out > out_cap)
        UKM_FAIL(UKM_ERR_CAPACITY, "%s: output needs %llu regions, capacity is %llu", name, (unsigned long long)*n_out, (unsigned long long)out_cap);
    return UKM_OK;
}

int map_entry(const char *name, ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off, uint64_t n_rec, const uint64_t *genome_off,
              uint64_t n_genome, int k, int hashed, const uint64_t *set_keys, uint64_t n_set, int allow_multi, uint64_t min_len,
              const MapOpts &o, uint32_t *out_rec, uint64_t *out_start, uint64_t *out_end, uint64_t out_cap, uint64_t *n_out) {
    UKM_TRY(check_args(name, ctx, n_out, bases, rec_off, n_rec, k, hashed));
    if ((n_set && !set_keys) || (out_cap && (!out_rec || !out_start || !out_end)) || (n_rec && !genome_off))
        UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
    if (min_len < 1) UKM_FAIL(UKM_ERR_INVALID, "%s: min_len must be at least 1", name);
    if (n_set >= (1ull << 32)) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu codes in the set; the limit is 2^32 - 1", name, (unsigned long long)n_set);
    if (o.max_gap_size > 0x7FFFFFFFull || o.max_gap_num > 0x7FFFFFFFull)
        UKM_FAIL(UKM_ERR_INVALID, "%s: max_gap_size and max_gap_num must be below 2^31", name);
    if (o.max_gap_size > 0 && o.max_gap_num == 0)
        UKM_FAIL(UKM_ERR_INVALID, "%s: max_gap_num must be above 0 when max_gap_size is (map.go:112)", name);
    *n_out = 0;
    if (n_rec == 0) return UKM_OK;
    if (n_genome == 0) UKM_FAIL(UKM_ERR_INVALID, "%s: records need at least one genome", name);
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        u32 *orec = nullptr;
        u64 *ostart = nullptr, *oend = nullptr;
        UKM_TRY(ukm_out_t(ctx, out_rec, out_cap, &orec));
        UKM_TRY(ukm_out_t(ctx, out_start, out_cap, &ostart));
        UKM_TRY(ukm_out_t(ctx, out_end, out_cap, &oend));
        const int r = map_regions(ctx, name, bases, rec_off, n_rec, genome_off, n_genome, k, hashed, set_keys, n_set, allow_multi, min_len, o,
                                  orec, ostart, oend, out_cap, n_out);
        const u64 n = r == UKM_OK ? *n_out : 0;  // (the copy-back of host outputs: what was written, nothing after an error)
        ukm_out_resize(ctx, out_rec, n * sizeof(u32));
        ukm_out_resize(ctx, out_start, n * sizeof(u64));
        ukm_out_resize(ctx, out_end, n * sizeof(u64));
        return r;
    }();
    return ukm_finish(&s, rc);
}

}  // namespace

extern "C" int ukm_map(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off, uint64_t n_rec, const uint64_t *genome_off,
                       uint64_t n_genome, int k, int hashed, const uint64_t *set_keys, uint64_t n_set, int allow_multi,
                       uint64_t min_len, uint32_t *out_rec, uint64_t *out_start, uint64_t *out_end, uint64_t out_cap,
                       uint64_t *n_out) {
    return map_entry("ukm_map", ctx, bases, rec_off, n_rec, genome_off, n_genome, k, hashed, set_keys, n_set, allow_multi, min_len, MapOpts(),
                     out_rec, out_start, out_end, out_cap, n_out);
}

extern "C" int ukm_map_gapped(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off, uint64_t n_rec, const uint64_t *genome_off,
                              uint64_t n_genome, int k, int hashed, int circular, const uint64_t *set_keys, uint64_t n_set,
                              int allow_multi, uint64_t min_len, uint64_t max_gap_size, uint64_t max_gap_num, uint32_t *out_rec,
                              uint64_t *out_start, uint64_t *out_end, uint64_t out_cap, uint64_t *n_out) {
    MapOpts o;
    o.circular = circular != 0;
    o.max_gap_size = max_gap_size;
    o.max_gap_num = max_gap_num;
    return map_entry("ukm_map_gapped", ctx, bases, rec_off, n_rec, genome_off, n_genome, k, hashed, set_keys, n_set, allow_multi, min_len, o,
                     out_rec, out_start, out_end, out_cap, n_out);
}
