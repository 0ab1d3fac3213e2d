// ukm_probe.h — internal: the hash-probe routes of the n-way operations, `union` / `common` of many heavily overlapping
// sorted sets and the placement merge.  One file per kernel family with the host code that launches it:
//   ukm_probe_union.hip   the plain pass (pu2_probe_kernel), the TaxId and counting tables (pt_probe_kernel), the routes
//   ukm_probe_ranked.hip  the ranked pass for files with one taxid each (pr_*)
//   ukm_place.hip         the placement merge (pl_merge_kernel)
//   ukm_probe.hip         the samplers and the host steps the routes share
// The build has no relocatable device code: a kernel is launched from its own file only, so a shared step that runs a
// family's kernel takes that launch as a callable.
#pragma once
#include <chrono>
#include <functional>
#include <vector>

#include "ukm_device.h"
#include "ukm_route.h"

// developer / test knob UKM_PUNION: 0 = never, 1 = whenever the shape allows it (size thresholds ignored),
// 2 = as 1 and without the hit-rate guard.  Unset: the library's own choice.
int ukm_punion_mode(const ukm_ctx *c);
// UKM_PUNION_TAX=0: records with TaxIds never take this path
int ukm_punion_tax_mode(const ukm_ctx *c);
// The three entries keep the route contract of ukm_route.h.  A stream whose in.taxids[j] is null and whose
// in.file_taxids[j] is set carries that ONE taxid (the .unik header's global taxid): it loads no taxid and looks no
// pre-order number up.
// Union; declines low overlap, an unsorted stream, a miss buffer overflow (the caller's k-way merge answers).  The
// result's TaxId is the LCA over every record of a code.  overlap_known: the caller has just sampled the overlap itself.
int ukm_dev_probe_union(ukm_ctx *c, const UkmStreams &in, bool overlap_known, const UkmOut &o, bool *declined);
// `common` below the number of files through the same tables with a record count per entry; in.keys[0] = the first file
// as a sorted duplicate-free set (first_once), or -- !first_once -- every record of every file counts (`merge -d`).
int ukm_dev_probe_common(ukm_ctx *c, const UkmStreams &in, u32 threshold, bool first_once, const UkmOut &o, bool *declined);
// Keep-everything merge of many files that share most of their codes, by placement (pl_merge_kernel):
// developer knob UKM_PLACE: 0 = never, 1 = whenever the shape allows it.
int ukm_place_mode(const ukm_ctx *c);
int ukm_dev_place_merge(ukm_ctx *c, const UkmStreams &in, const UkmOut &o, bool *declined);

#ifndef PU_K0_N
#define PU_K0_N 8
#endif
constexpr int PU_K0 = PU_K0_N;    // files merged into the base set
#ifndef PU_WAVES
#define PU_WAVES 4
#endif
constexpr int PU_RANGE = 2048;    // base entries per range
constexpr int PU_BUCKET_BITS = 11;  // 2048 buckets x 4 slots x 8 B = 64 KB of LDS: two workgroups per CU
constexpr int PU_BUCKETS = 1 << PU_BUCKET_BITS;
constexpr int PU_SLOTS = 4 * PU_BUCKETS;
constexpr int PU_MAXS = 4096;     // later files per launch
constexpr int PU_LMISS = 512;     // new codes a range keeps in LDS before they go out in one piece
constexpr u32 PU_CHUNK = 32;      // slots of the miss list a wave reserves at a time
constexpr u64 PU_EMPTY = ~0ull;
constexpr double PU_MIN_HIT = 0.55;  // (a table takes as many new codes as it has base entries: see PT_MIN_HIT)
enum { PU_FLAG_UNSORTED = 1, PU_FLAG_OVERFLOW = 2, PU_FLAG_TAXID = 4, PU_FLAG_RAW = 8 };
// New codes are claimed in the tables with their fold, and a table takes as many of them as it has base entries: the pass
// works as long as the later files bring fewer new codes than the base set holds, i.e. from a hit rate of one half on.
// (1000 files x 1e6 with taxids, a fifth of a universe each: 59 % hits, 18.8 ms against 34 ms through the single-pass
// merge; a tenth each: 34 % hits, the tables fill up and every further record is listed: 179 ms.)
constexpr double PT_MIN_HIT = 0.55;

struct PuArgs {
    const u64 *const *files;  // [S1] later files (device table of device pointers)
    const u64 *lens;          // [S1]
    u32 S1;
    const u64 *base;          // sorted, duplicate-free
    u64 n0;
    u32 R;                    // ranges = ceil(n0 / PU_RANGE)
    u64 *cuts;                // [R + 1][S1]
    u64 *miss;
    u64 miss_cap;
    u64 *ctl;                 // [0] misses, [1] flags, [2] sample hits, [3] samples
    u32 range;                // base entries per range (PU_RANGE; with TaxIds PT_RANGE)
    // with TaxIds (pt_probe_kernel)
    const u32 *const *tfiles; // [S1] TaxIds of the later files (an entry may be null: all 0)
    u32 *base_tax;            // [n0] in: the fold over the base files, out: over every file
    u32 *miss_tax;            // beside `miss`
    unsigned short *rec_idx;  // placement merge: [all records, file by file] the record's code as an index into its range
    const u64 *rec_off;       // [S1]: where file j's records begin in rec_idx
    u32 threshold;            // COUNT (`common`): a code leaves when at least this many records carried it
    u32 count0;               // COUNT: records a base entry starts with (1: the base set is the first file; 0: every file is probed)
    // files with ONE taxid each (round 5; the .unik header's global taxid): tfiles[j] is null and cte[j] = taxid | its
    // pre-order number << 32 (pu_cte_kernel) -- a slice of such a file loads no taxids and looks no number up
    const u64 *cte;           // [S1], or null: files without per-record taxids have taxid 0
    u32 base_ct;              // COUNT with the first file as the base set and no base_tax: its file taxid
    // Round 5, pt_probe_kernel: the taxids of the later records look UNRELATED to the entries' (the sample: ctl[6]): a record
    // brings the one-byte CLADE code of its taxid instead of the 4-byte pre-order number (see the kernel's fold)
    u32 clade_mode;
    TaxDev tax;
};


typedef u64 pu_u64x2 __attribute__((ext_vector_type(2)));
typedef pu_u64x2 __attribute__((aligned(8))) pu_pair;  // 16 bytes at 8-byte alignment

namespace {
__device__ __forceinline__ u64 pu2_shr1(u64 v, u64 carry) {  // lane l gets v of lane l - 1, lane 0 gets `carry`
    const u32 lo = (u32)__builtin_amdgcn_update_dpp((int)(u32)carry, (int)(u32)v, 0x138, 0xF, 0xF, false);          // wave_shr:1
    const u32 hi = (u32)__builtin_amdgcn_update_dpp((int)(u32)(carry >> 32), (int)(u32)(v >> 32), 0x138, 0xF, 0xF, false);
    return ((u64)hi << 32) | lo;
}
}  // namespace

static inline int pu_launch_cuts(ukm_ctx *c, const PuArgs &a) {  // cuts[r][j] = lower bound of base[r range] in later file j
    return ukm_launch_range_cuts(c, RangeCuts{a.files, a.lens, a.S1, a.R, a.base, a.range, a.cuts});
}

// ---- host steps of the probe routes (ukm_probe.hip) ----
// Debug stage timer of a route (UKM_PUNION_DEBUG): "<tag> <stage> <ms since the last lap>", after a sync.
struct PuLap {
    ukm_ctx *c;
    const char *tag;
    bool on = ukm_env(c, "UKM_PUNION_DEBUG") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char *what) {
        if (!on) return;
        (void)hipStreamSynchronize(c->stream);
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "%s %-10s %8.3f ms\n", tag, what, std::chrono::duration<double, std::milli>(t - t0).count());
        t0 = std::chrono::steady_clock::now();
    }
};
// Records with taxids need the output's taxids and a loaded taxonomy (errors; `op` names the operation in the message);
// *ready = false: the taxonomy has no pre-order tables and the route declines.
int ukm_pu_tax_ready(ukm_ctx *c, const u32 *tout, const char *op, bool *ready);
// Files by size, the largest first (files of one size keep their order); in_base[j]: file j is one of the k0 largest.
std::vector<int> ukm_pu_largest(const u64 *lens, int S, int k0, std::vector<char> *in_base);
// BASE = the k-way union of the streams b, their TaxIds folded (a stream with ONE taxid gets its array first: the k-way
// union reads a taxid per record).  *n0 = 0: the k-way merge declined.
int ukm_pu_base_union(ukm_ctx *c, const UkmStreams &b, u64 **base, u32 **base_tax, u64 *n0);
// The base set's attempts: k0 files, then ONE more with four times as many when the first share too little with the
// later files (*low_hit) but promise enough -- files that each hold a share p of a collection hit a base set of k of them
// with probability 1 - (1 - p)^k, so the next set is expected at 1 - (1 - hit)^4.  stat_punion_attempts counts them.
// An attempt with a low hit gives its workspace back; *low_hit on return: the ladder gave up.
int ukm_pu_attempts(ukm_ctx *c, int k0, int S, double min_hit, bool *low_hit, const std::function<int(int k0, bool *low_hit, double *hit)> &attempt);
// The hit-rate sample (pu_sample_kernel): 2^16 records of a.files [0, a.S1) looked up in the base set.  h[2] of h[3] were
// found (h[3] = 0: nothing to sample); h[6], h[7] feed ukm_pu_clade_mode (words = 4: only the hit counts are read back).
int ukm_pu_hit_sample(ukm_ctx *c, const PuArgs &a, u64 h[8], int words = 8);
u32 ukm_pu_clade_mode(const ukm_ctx *c, const TaxDev &T, bool tax, u64 hits, u64 same, u64 runs);
// The guards behind the sample: *low_hit when fewer than min_hit of the sampled records are in the base set (more files
// in it may help); else *too_many when the new codes of the later files would overflow the tables (pu_new_codes: more
// files in the base set would not help, the new codes are the files' own).
int ukm_pu_hit_guard(ukm_ctx *c, const PuArgs &a, double miss_rate, double min_hit, u64 later, bool *low_hit, bool *too_many);
// cte[j]: the file taxid in its low word gets its pre-order number in the high word (pu_cte_kernel; with the clade code)
int ukm_pu_cte(ukm_ctx *c, u64 *cte, u32 n, u32 clade_mode = 0);
// the share of sampled records that are found in another file (pu_overlap_kernel): h[2] of h[3], into a.ctl
int ukm_pu_overlap_sample(ukm_ctx *c, const PuArgs &a, u64 h[4]);
int ukm_pu_overlap_share(ukm_ctx *c, const UkmStreams &in, double *share);
// The range-load guard: one workgroup streams everything that falls into its range, so later files whose records crowd
// into a few ranges (codes beyond the base set's last entry, a dense cluster the base set does not have) would leave the
// pass to a handful of CUs.  *heavy: more than 64 x the average load (`records` over a.R ranges) in one range.
int ukm_pu_range_load(ukm_ctx *c, const PuArgs &a, u64 records, bool say, bool *heavy);
// The probe pass over files [0, S1) of the tables in a, PU_MAXS at a time: cut points, the range-load guard (`say`: print
// its line), probe(a) between ev_k0 and ev_k1.  hlens: the files' lengths on the host.  *heavy: a batch declined (one that
// already ran only produced list entries).
int ukm_pu_probe_batches(ukm_ctx *c, PuArgs &a, int S1, const u64 *hlens, PuLap &lap, bool say, bool *heavy,
                     const std::function<void(const PuArgs &)> &probe);
// The end of the union routes: BASE [0, n0) ∪ the sorted, duplicate-free list a.miss [0, nm) -- with TaxIds the LCA over
// equal codes of the list and over the codes it shares with BASE finishes the fold --, an empty list: BASE itself.
int ukm_pu_finish(ukm_ctx *c, const PuArgs &a, u64 nm, const u64 *base, const u32 *base_tax, u64 n0, const UkmOut &o, PuLap &lap,
              const char *sort_stage, bool *declined);
// The probe union of files with ONE taxid each (ukm_probe_ranked.hip): one attempt of ukm_dev_probe_union, the contract
// of probe_union_k0 in ukm_probe_union.hip.
int ukm_probe_union_ranked(ukm_ctx *c, const UkmStreams &in, int k0, const UkmOut &o, bool *declined, bool *low_hit, double *hit_rate);
