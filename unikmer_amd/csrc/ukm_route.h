// ukm_route.h — internal: what the device routes of the n-way operations share (ukm_probe_union.hip, ukm_srmerge.hip,
// ukm_kway.hip, ukm_pfold.hip, ukm_fold.hip; their caller is ukm_nway.hip)
//
// The route contract.  Every route entry ukm_dev_*(c, in, [its own arguments,] out, &declined):
//   * sets *declined = true and *out.n = 0 on entry;
//   * clears *declined only when the answer is in the output, out.keys / out.taxids [0, *out.n);
//   * declines for inputs that are not its own (a shape it does not fit, a duplicate or unsorted stream, ...): *out.n
//     is then 0, the output's contents are undefined, and the caller's next route answers;
//   * returns an error as an error, never as a decline (UKM_ERR_UNSORTED of the range fold, capacity, no taxonomy).
// All stream and output pointers are device pointers.
#pragma once
#include <atomic>
#include <cstdio>
#include <utility>
#include <vector>

#include "ukm_internal.h"

struct UkmStreams {
    const u64 *const *keys;    // [S]
    const u32 *const *taxids;  // [S] per-record taxids (an entry may be null), or null: none
    const u32 *file_taxids;    // [S] the ONE taxid of a file whose taxids[j] is null (the .unik header's), or null
    const u64 *lens;           // [S]
    int S;
    bool tax;                  // the records carry taxids
    UkmStreams from(int j0) const {  // streams j0 .. S - 1
        return UkmStreams{keys + j0, taxids ? taxids + j0 : nullptr, file_taxids ? file_taxids + j0 : nullptr, lens + j0, S - j0, tax};
    }
    u32 file_taxid(int j) const { return (tax && file_taxids && !(taxids && taxids[j])) ? file_taxids[j] : 0u; }
};

struct UkmOut {
    u64 *keys;
    u32 *taxids;
    u64 cap;
    u64 *n;
};

// One device table of a route's streams: [keys S][taxids S][lens S][file taxids S], then the u64 columns a route appends
// (sample bases, segment bases, record offsets).  Kernels read it through these accessors.
struct StreamTab {
    u64 *d;
    u32 S;
    __host__ __device__ const u64 *const *keys() const { return (const u64 *const *)d; }
    __host__ __device__ const u32 *const *taxids() const { return (const u32 *const *)(d + S); }
    __host__ __device__ const u64 *lens() const { return d + 2 * (size_t)S; }
    __host__ __device__ u64 *file_taxids() const { return d + 3 * (size_t)S; }
    __host__ __device__ u64 *extra() const { return d + 4 * (size_t)S; }
};
// one H2D copy of the table (+ `nextra` extra words) and a sync: the host copy is pageable
int ukm_stream_tab(ukm_ctx *c, const UkmStreams &in, StreamTab *t, const u64 *extra = nullptr, size_t nextra = 0);

// Developer output of a route (UKM_*_DEBUG): device time between named points of the stream.  print() after a sync.
struct PhaseMarks {
    bool on;
    hipStream_t st;
    std::vector<std::pair<const char *, hipEvent_t>> m;
    PhaseMarks(bool on_, hipStream_t st_) : on(on_), st(st_) {}
    ~PhaseMarks() {
        for (auto &x : m) (void)hipEventDestroy(x.second);
    }
    void mark(const char *name) {
        hipEvent_t e;
        if (on && hipEventCreate(&e) == hipSuccess) {
            (void)hipEventRecord(e, st);
            m.emplace_back(name, e);
        }
    }
    void print() const {  // " name=ms" per phase, on stderr
        for (size_t i = 1; i < m.size(); i++) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, m[i - 1].second, m[i].second);
            fprintf(stderr, " %s=%.3fms", m[i].first, ms);
        }
    }
};

// Workgroups of `kernel` (nt threads) resident on the device at once, worked out once per `cache` slot.  The range folds
// size their ranges so that all of them run in one round.
template <typename K>
u64 ukm_resident_slots(ukm_ctx *c, std::atomic<int> &cache, K kernel, int nt) {
    if (!cache.load(std::memory_order_relaxed)) {  // (racing first calls compute the same value)
        int per_cu = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, nt, 0);
        if (e != hipSuccess || per_cu <= 0) per_cu = 2;
        cache.store(per_cu * c->num_cu, std::memory_order_relaxed);
    }
    return (u64)cache.load(std::memory_order_relaxed);
}

// One cut kernel for the routes whose splitters are every L-th record of a base stream (probe fold, probe union; the range
// fold keeps its paired layout):
// cuts[r][j] = lower bound of base[r L] in file j, r = 0 .. R (row 0: 0, row R: the file's length).  A range reads rows r
// and r + 1.  A block holds 16 ranges x 16 files: 16 neighbouring lanes store one range's cuts in 16 consecutive files.
struct RangeCuts {
    const u64 *const *files;  // [S1]
    const u64 *lens;          // [S1]
    u32 S1, R;
    const u64 *base;
    u64 L;
    u64 *cuts;                // [R + 1][S1]
};
int ukm_launch_range_cuts(ukm_ctx *c, const RangeCuts &a);

// The end of a range-partitioned route.  Range r's cnt[r] records start at src + (slot ? slot[r] : r * stride); an
// exclusive scan of cnt (ctl[0] = total) places them in the output, `parts` workgroups per range copy them (a range that
// does not fit is not written; a route whose ranges may give up without writing their count zeroes cnt first).  Without
// cnt only the read-back runs: h = ctl[0..1] (total, flags).
struct RangeGather {
    const u64 *src_k = nullptr;
    const u32 *src_t = nullptr;
    const u64 *slot = nullptr;
    u64 stride = 0;
    const u64 *cnt = nullptr;
    u32 R = 0;
    int parts = 1;
};
int ukm_range_finish(ukm_ctx *c, const RangeGather &g, u64 *ctl, const UkmOut &o, u64 h[2]);
// a route's answer of n records: *o.n = n, UKM_ERR_CAPACITY when they do not fit, else *declined = false
int ukm_route_answer(u64 n, const UkmOut &o, bool *declined);
