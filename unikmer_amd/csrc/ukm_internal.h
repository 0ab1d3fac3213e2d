// ukm_internal.h — shared host-side plumbing of libunikmer_hip.so (context, workspace arena,
// host/device pointer staging, error reporting).  gfx950 only; no portability layer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/unikmer_hip.h"
#include "ukm_sort_state.h"

typedef uint64_t u64;
typedef uint32_t u32;
typedef uint8_t u8;

// ---- error reporting (thread-local message, never exit) -------------------------------------
void ukm_set_error(const char *fmt, ...);

#define UKM_FAIL(code, ...)        \
    do {                           \
        ukm_set_error(__VA_ARGS__); \
        return (code);             \
    } while (0)

#define UKM_HIP(expr)                                                                    \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            ukm_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                          __LINE__);                                                     \
            return _e == hipErrorOutOfMemory ? UKM_ERR_NOMEM : UKM_ERR_HIP;              \
        }                                                                                \
    } while (0)

#define UKM_TRY(expr)            \
    do {                         \
        int _rc = (expr);        \
        if (_rc != UKM_OK) return _rc; \
    } while (0)

// ---- device taxonomy ------------------------------------------------------------------------
struct TaxDev {
    const u32 *parent;  // dense [size]; 0 = absent; root: parent[r] == r
    const u8 *depth;    // dense [size]; root depth 0
    const u32 *merged;  // dense [size] or nullptr; 0 = not merged
    u32 size;
    // (the rank column of ukm_taxonomy_set_ranks, dense u8 [size], lives beside these in the context -- ukm_ctx::tax_rank --
    //  and is handed to the one kernel that reads it, ukm_tax.hip's rank_keep_kernel, as an argument of its own)
    // root-path table (round 3): anc[c * size + t] = the ancestors of t at depths 4c .. 4c+3 (t itself at its own
    // depth, 0 beyond it; all 0 for an absent taxid).  Always present when a taxonomy is loaded: ukm_taxonomy_load builds
    // every table or none (it refuses dumps whose dense tables do not fit the device).
    const uint4 *anc;
    u32 nchunks;
    // pre-order numbers (round 3, ukm_pfold.hip): euler[t] = 1 + the position of t (merged ids: of their target) in a
    // depth-first walk of the forest, 0 for taxid 0 / absent / unknown ids; node_at[e] = the taxid with number e.
    // The LCA of a SET of nodes is the LCA of its members with the smallest and the largest number.
    const u32 *euler;
    const u32 *node_at;
    // clade codes (round 5): clade[t] = 1 + the index of t's ancestor at depth min(depth(t), D) among the nodes of depth <= D
    // (D <= 3, the deepest level whose nodes fit 16 bits; 0: absent / merged id, or no table), top[k] = the root path
    // (depths 0..3, as a row of anc[0]) of clade node k.  Two taxids with DIFFERENT codes have the LCA of their clade nodes:
    // two 2-byte reads of a table that mostly sits in L2 and two rows of a table of a few KB settle every pair that
    // diverges within D levels of the root, instead of two random 16-byte rows of the 16 B x ids root-path table.
    const unsigned short *clade;
    const uint4 *top;
    // the same codes in ONE byte per id when the nodes of depth <= 2 (or 1, or 0) are at most 255: a table a quarter the size
    // of a 4-byte column stays in L2 beside the streams (2.4 MB for 2.4 M ids); `clade` is null then
    const unsigned char *clade8;
    // beside clade8: pair[ca * kp + cb] = the LCA of clade nodes ca and cb (0 on the diagonal and in row / column 0: same
    // clade or no code -> the root paths answer); at most 256 x 256 words, one read instead of two rows of `top`
    const u32 *pair;
    u32 kp;
    // behind the pair table, in the same allocation (round 6): what a workgroup copies into LDS so that an unrelated pair
    // costs NO third gather.  cpath[c] = 16 bytes: byte d = the code of clade node c's ancestor at depth d (c itself at its
    // own depth, 0 below it; the first 16 levels of a deeper node), 256 rows; cnode[c] = the taxid of clade node c, 256
    // words.  Two different codes whose rows differ have the LCA cnode[the last byte their rows share] (no shared byte:
    // different trees, 0); rows that agree in all 16 bytes (both nodes 16 or more levels down one chain) ask `pair`.
    const uint4 *cpath;
    const u32 *cnode;
};
constexpr u32 TAX_CPATH_ROWS = 256;

// ---- workspace arena: chunked bump allocator on the ctx's device ------------------------------
struct WsBlock {
    char *base;
    size_t cap;
    size_t used;
};

struct ukm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;  // whole call
    bool ev_valid = false;
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr;  // dominant kernel of the call
    bool evk_valid = false;
    // transfer stream (ukm_copy_async): created on first use
    hipStream_t xfer = nullptr;
    hipEvent_t ev_xfer = nullptr, ev_comp = nullptr;
    bool xfer_pending = false;
    // RCCL communicator of the multi-GPU exchange (ukm_comm.hip); nullptr until ukm_comm_init
    void *comm = nullptr;
    int comm_size = 0, comm_rank = 0;
    int depth = 0;  // nesting depth of API calls (n-way ops call 2-way ops)
    int last_route = 0;  // ukm_last_route(): which n-way route answered last

    std::vector<WsBlock> blocks;
    size_t ws_high = 0;  // high-water mark of one top-level call, for consolidation
    // test aid (option "ws_poison"): the byte every arena block is filled with before a top-level call and when it is
    // created; -1 = off, and nothing is enqueued.  stat_ws_poisoned: the bytes filled since the most recent top-level call
    // began (the blocks it created, the block ws_reset_top merged them into and a later ukm_ctx_reserve included)
    int ws_poison = -1;
    u64 stat_ws_poisoned = 0;

    // pending host copy-backs of the current top-level call
    struct CopyBack {
        void *host;
        const void *dev;
        size_t bytes;
    };
    std::vector<CopyBack> copybacks;

    // taxonomy (device arrays owned by the ctx)
    u32 *tax_parent = nullptr;
    u8 *tax_depth = nullptr;
    u32 *tax_merged = nullptr;
    u8 *tax_rank = nullptr;  // rank id of every node (ukm_taxonomy_set_ranks): dense [tax_size], 0 = no known rank; null until set
    uint4 *tax_anc = nullptr;  // root-path table, see TaxDev
    u32 *tax_euler = nullptr, *tax_node_at = nullptr;  // pre-order numbers, see TaxDev
    unsigned short *tax_clade = nullptr;                // clade codes, see TaxDev (tax_clade8: the one-byte form)
    unsigned char *tax_clade8 = nullptr;
    u32 *tax_pair = nullptr;
    u32 tax_kp = 0;
    uint4 *tax_top = nullptr;
    u32 tax_top_n = 0;  // entries of tax_top
    u32 tax_nchunks = 0;
    u32 tax_size = 0;
    u32 tax_max = 0;

    // pinned host scratch for small D2H results
    u64 *h_scratch = nullptr;  // 64 x u64

    int num_cu = 256;

    // Route policy and developer knobs (round 5): the UKM_* variables of the environment are read ONCE, when the context is
    // created (knobs), and ukm_ctx_set_option overrides them per context (opts: "punion" <-> UKM_PUNION ...).  No compute
    // call reads the environment -- unless the context was created under UKM_ENV_LIVE=1 (the test suite, whose cases flip
    // knobs between calls on one context).
    std::map<std::string, std::string> knobs, opts;
    bool env_live = false;
    // statistics a host or a test may ask for (ukm_ctx_get_stat)
    u64 stat_inflate_cp_walk_us = 0;  // of the last ukm_inflate: device time of the second walk (inf_cp_kernel), microseconds
    u64 stat_inflate_candidates = 0, stat_inflate_segments = 0;  // of the last ukm_inflate: offsets behind a marker (and 0); segments on the chain
    u64 stat_grep_route = 0;  // membership shape of the last ukm_grep: 1 queries in LDS, 2 sorted queries behind a prefix directory, 3 taxid bitmap, 0 no kernel
    u64 stat_window_route = 0;  // kernel that wrote the windows of the last call through run_windows: 1 window_kernel, 2 stripwin_kernel, 3 nthash_strip_kernel, 0 no launch
    u64 stat_window_strip_declined = 0;  // strip kernel launches of this context that set ENC_FLAG_OVERFLOW (record table / candidate list): the general kernel answered
    u64 stat_punion_attempts = 0;  // base sets the last probe union / counting probes built (2: the retry with 4 x the files ran)
    u64 stat_punion_flags = 0;     // the flag word (ctl[1], PU_FLAG_*) the most recent probe pass of this context left
    u64 stat_count_window_retries = 0;  // ukm_count calls that repeated the window pass: its estimated buffer was too small
    u64 stat_setop_part_hits = 0;   // 2-way set operations that took their merge-path table from the partition cache (verified, see below)
    u64 stat_setop_part_stale = 0;  // ... whose cached table failed the verification: the partition ran after all
    u64 stat_setop_offs_hits = 0;   // ... of the hits: plain-key passes that took their tiles' output offsets from the cached match counts
    u64 stat_setop_offs_stale = 0;  // ... whose tiles counted otherwise (contents changed in place, partition intact): the pass ran again with the look-back
    u64 stat_setop_multi_fused = 0;  // ukm_setop2_multi calls answered by the one fused pass
    u64 stat_setop_multi_split = 0;  // ... by one ordinary pass per operation (taxids, one operation, duplicate codes)
    // of the last ukm_pair_counts (ukm_pairs.hip): distinct codes over all streams, column blocks walked, and the device time,
    // in microseconds, of its three steps: records sorted and ranked, bits set (zeroing included), pair kernel launches
    u64 stat_pair_columns = 0, stat_pair_blocks = 0;
    u64 stat_pair_sort_us = 0, stat_pair_bits_us = 0, stat_pair_kernel_us = 0;
    // ukm_last_kernel_ms of a call whose dominant kernel ran as several launches: their summed time (kernel_ms_sum_valid;
    // cleared when a top-level call begins), which one ev_k0 / ev_k1 bracket cannot hold
    float kernel_ms_sum = 0.f;
    bool kernel_ms_sum_valid = false;

    // Partition cache of the public 2-way set operation (ukm_setops.hip: run_setop_pass).  The merge-path table depends on
    // (A, B, |A|, |B|, tile size) only -- union, inter and diff of one pair share it -- so the context keeps the table of the
    // most recent call in ONE slot of device memory of its own (never the arena: that is poisoned by tests and reused by
    // every call) and the next call on the same key VERIFIES it against the inputs as they are now instead of searching
    // again.  buf[0] = the verification's stale word (zero whenever `valid`), buf[PC_HEAD ...] = the table.
    // Behind the table's ntiles + 1 words a second column of ntiles + 1: MP[t] = how many matched pairs of (A, B) have their A
    // record in front of boundary t.  Every plain-key operation's tile offsets follow from it (ukm_setop_part.h:
    // setop_partition_verify_kernel), so a pass that finds it valid runs without the look-back.  Same key, same slot: it is
    // dropped wherever the table is; `counts_valid` is set only behind a pass that came back without any flag.
    struct PartCache {
        static constexpr size_t PC_HEAD = 8;  // u64 words in front of the table: a 64-byte line
        struct Key {
            const u64 *a = nullptr, *b = nullptr;
            u64 na = 0, nb = 0, tile_items = 0;
            bool operator==(const Key &o) const { return a == o.a && b == o.b && na == o.na && nb == o.nb && tile_items == o.tile_items; }
        };
        u64 *buf = nullptr;
        size_t cap_words = 0;
        Key key;
        bool valid = false;
        int stale_run = 0;  // stale hits in a row
        bool off = false;   // two in a row (a caller that refills fixed buffers with same-sized batches): no more attempts
        bool counts_valid = false;
        int offs_stale_run = 0;  // passes in a row whose tiles contradicted the counts
        bool offs_off = false;   // two in a row: no more attempts (the partition cache itself goes on)

        u64 *stale_word() const { return buf; }
        u64 *table() const { return buf + PC_HEAD; }
        u64 *counts(u64 ntiles) const { return table() + ntiles + 1; }
        // Room for a table and a count column of ntiles + 1 words each.  Grown on demand: the slot's contents go with the old
        // buffer.  false = no memory for a cache: the call goes on without one.
        bool reserve(u64 ntiles) {
            const size_t need = PC_HEAD + 2 * ((size_t)ntiles + 1);
            if (cap_words >= need) return true;
            if (buf) (void)hipFree(buf);
            buf = nullptr;
            cap_words = 0;
            valid = counts_valid = false;
            void *nbuf = nullptr;
            if (hipMalloc(&nbuf, need * sizeof(u64)) != hipSuccess) {
                (void)hipGetLastError();
                return false;
            }
            buf = (u64 *)nbuf;
            cap_words = need;
            return true;
        }
        // A pass on key k begins: is the slot's table k's, and are its counts usable?  The slot holds NOTHING until commit(): an
        // error on the way leaves no key behind.
        struct Opened { bool hit, counts; };
        Opened open(const Key &k) {
            const Opened o = {valid && key == k, valid && key == k && counts_valid};
            valid = counts_valid = false;
            return o;
        }
        // the pass has come back: the table in the slot belongs to k's inputs as they were a moment ago
        void commit(const Key &k, bool counts) {
            key = k;
            valid = true;
            counts_valid = counts;
        }
        // the verdicts of the passes that tried: two bad ones in a row end the attempts for the context's lifetime
        void note_table(bool stale) { if (!stale) stale_run = 0; else if (++stale_run >= 2) off = true; }
        void note_counts(bool stale) { if (!stale) offs_stale_run = 0; else if (++offs_stale_run >= 2) offs_off = true; }
    } part_cache;

    // set once the blockIdx-ordered set-op kernel hit its watchdog on this device
    bool setop_force_ticket = false;  // = ticket_latched || option "force_ticket"
    bool ticket_latched = false;      // the look-back watchdog fired on this device (ukm_switch_to_tickets): stays set
    unsigned long long stat_lb_watchdogs = 0;  // times ukm_switch_to_tickets ran: a launch ladder's retry, or a chained fold's fallback

    // The radix sort (ukm_sort.hip): what it keeps from one sort to the next and its statistics (SortPolicy, ukm_sort_state.h),
    // and the device resources it creates on first use and ukm_ctx_destroy releases.
    struct SortState : SortPolicy {
        // buckets of the last bucket-route sort that fell back from the counting step to the digit passes: bumped by
        // ls_sort_kernel, fetched and cleared by the next sort's classify kernel (SortPolicy::note_fallbacks)
        u64 *stat_dev = nullptr;
        // two more streams for launches that do not depend on each other (the bucket kernel's size classes): forked from and
        // joined to the call's stream by events inside one call
        hipStream_t side[2] = {nullptr, nullptr};
        hipEvent_t ev_fork = nullptr, ev_side[2] = {nullptr, nullptr};

        int stat_word(hipStream_t stream, u64 **out) {
            if (!stat_dev) {
                UKM_HIP(hipMalloc((void **)&stat_dev, 64));
                UKM_HIP(hipMemsetAsync(stat_dev, 0, 64, stream));
            }
            *out = stat_dev;
            return UKM_OK;
        }
        int side_streams() {
            if (ev_fork) return UKM_OK;
            UKM_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
            for (int i = 0; i < 2; i++) {
                UKM_HIP(hipStreamCreateWithFlags(&side[i], hipStreamNonBlocking));
                UKM_HIP(hipEventCreateWithFlags(&ev_side[i], hipEventDisableTiming));
            }
            return UKM_OK;
        }
        void release() {
            if (stat_dev) (void)hipFree(stat_dev);
            for (int i = 0; i < 2; i++) {
                if (side[i]) { (void)hipStreamSynchronize(side[i]); (void)hipStreamDestroy(side[i]); }
                if (ev_side[i]) (void)hipEventDestroy(ev_side[i]);
            }
            if (ev_fork) (void)hipEventDestroy(ev_fork);
        }
    } sort;
};

// The value of knob UKM_<NAME> for this context (see ukm_ctx::knobs): nullptr when it is not set.  The pointer stays valid
// until the next ukm_ctx_set_option on the context.
const char *ukm_env(const ukm_ctx *c, const char *name);
static inline bool ukm_env_is(const ukm_ctx *c, const char *name, char v) {
    const char *e = ukm_env(c, name);
    return e && e[0] == v;
}
static inline int ukm_env_int(const ukm_ctx *c, const char *name, int unset) {
    const char *e = ukm_env(c, name);
    return (e && *e) ? atoi(e) : unset;
}

// Arena API.  Pointers stay valid until the enclosing top-level call returns.
int ws_alloc(ukm_ctx *c, size_t bytes, void **out);
template <typename T>
static inline int ws_alloc_t(ukm_ctx *c, size_t n, T **out) {
    void *p = nullptr;
    int rc = ws_alloc(c, n * sizeof(T), &p);
    *out = (T *)p;
    return rc;
}
struct WsMark {
    size_t nblocks;
    size_t used_last;
};
WsMark ws_mark(ukm_ctx *c);
void ws_release(ukm_ctx *c, WsMark m);  // frees allocations made after the mark (LIFO)

// true if p is a device pointer usable by kernels on this ctx's device
bool ukm_is_device_ptr(const void *p);

// Input staging: returns p itself for device pointers, else an arena copy (H2D on the stream).
int ukm_in(ukm_ctx *c, const void *p, size_t bytes, const void **dev);
template <typename T>
static inline int ukm_in_t(ukm_ctx *c, const T *p, size_t n, const T **dev) {
    const void *d = nullptr;
    if (p == nullptr || n == 0) {
        *dev = p;
        if (p == nullptr) return UKM_OK;
    }
    int rc = ukm_in(c, p, n * sizeof(T), &d);
    *dev = (const T *)d;
    return rc;
}
// Output staging: device pointers pass through; host pointers get an arena buffer whose
// first `bytes` are copied back by ukm_finish() (use ukm_out_resize to shrink the copy).
int ukm_out(ukm_ctx *c, void *p, size_t bytes, void **dev);
template <typename T>
static inline int ukm_out_t(ukm_ctx *c, T *p, size_t n, T **dev) {
    void *d = nullptr;
    if (p == nullptr) {
        *dev = nullptr;
        return UKM_OK;
    }
    int rc = ukm_out(c, p, n * sizeof(T), &d);
    *dev = (T *)d;
    return rc;
}
// Output array of an entry point that answers a size query (include/unikmer_hip.h: with out_cap == 0 every output pointer
// may be NULL): the routes get one workspace word in place of a NULL array -- nothing is copied back -- so none of them
// ever holds a null output pointer, whatever it does about the capacity.
template <typename T>
static inline int ukm_out_query_t(ukm_ctx *c, T *p, size_t n, T **dev) {
    if (p != nullptr || n != 0) return ukm_out_t(c, p, n, dev);
    return ws_alloc_t(c, 1, dev);
}
void ukm_out_resize(ukm_ctx *c, void *host, size_t bytes);
// In-place staging (sort): host array copied in, and copied back at finish.
int ukm_inout(ukm_ctx *c, void *p, size_t bytes, void **dev);

// Call bracket.  ukm_begin at the top of every compute entry; ukm_finish before returning:
// performs copy-backs, stream sync, arena reset (top level only).  Nested calls are cheap.
struct CallScope {
    ukm_ctx *c;
    bool top;
    WsMark mark;
};
int ukm_begin(ukm_ctx *c, CallScope *s);
int ukm_finish(CallScope *s, int rc);

// read one u64 (or several) from device memory to host, synchronising the stream
int ukm_read_u64(ukm_ctx *c, const u64 *dev, u64 *host, int n = 1);

static inline TaxDev ukm_taxdev(const ukm_ctx *c) {
    TaxDev t;
    t.parent = c->tax_parent;
    t.depth = c->tax_depth;
    t.merged = c->tax_merged;
    t.anc = c->tax_anc;
    t.euler = c->tax_euler;
    t.node_at = c->tax_node_at;
    t.clade = c->tax_clade;
    t.clade8 = c->tax_clade8;
    t.pair = c->tax_pair;
    t.kp = c->tax_kp;
    {   // [pair kp x kp | pad to 16 bytes | cpath 256 x 16 B | cnode 256 x 4 B]
        const size_t off = (((size_t)c->tax_kp * c->tax_kp) + 3) & ~(size_t)3;
        t.cpath = c->tax_pair ? reinterpret_cast<const uint4 *>(c->tax_pair + off) : nullptr;
        t.cnode = c->tax_pair ? c->tax_pair + off + 4 * TAX_CPATH_ROWS : nullptr;
    }
    t.top = c->tax_top;
    t.nchunks = c->tax_nchunks;
    t.size = c->tax_size;
    return t;
}

// ---- launch protocol of the kernels that compact with the decoupled look-back (ukm_device.h) --------------------
#ifndef LB_STRIDE
#define LB_STRIDE 8  /* u64 words per tile's status word: a 64-byte line of its own */
#endif
static inline size_t lb_status_words(u64 ntiles) { return (size_t)ntiles * LB_STRIDE; }

// The control block of one launch: [0] count, [1] flags, [2] ticket counter, [3..7] the launch's own words, then one
// status line per tile.  Head and status lines must be zero before the kernel starts; `tail` words behind them are
// the launch's own and are never zeroed (the set operation's partition points).
struct LbCtl {
    static constexpr size_t HEAD = 8;
    u64 *result = nullptr;
    u32 *ticket = nullptr;
    u64 *status = nullptr;
    u64 *tail = nullptr;
    u64 *zero_from = nullptr;  // what must be zero before a launch ...
    size_t zero_words = 0;     // ... the head too, unless it is the caller's
};
// ntiles = 0: a launch without look-back (head only).  `head` != null: HEAD zeroed words the caller owns (a chained fold
// reads them after the arena is gone); status lines and tail still come from the arena.
int ukm_lb_ctl_alloc(ukm_ctx *c, u64 ntiles, size_t tail, LbCtl *b, u64 *head = nullptr);
int ukm_lb_ctl_zero(ukm_ctx *c, const LbCtl &b);

// a look-back watchdog fired in a blockIdx-ordered kernel: from now on this context uses the ticketed
// instantiations (one warning on stderr per context, so that an operator sees the slower mode)
void ukm_switch_to_tickets(ukm_ctx *c, const char *where);

// The watchdog ladder.  The first attempt takes tile ids from blockIdx -- unless the context is on tickets already or
// `ticket_first` says that a second attempt could not repair the first (output over input).  If the kernel then reports
// its watchdog bit in result word [1], the context switches to tickets for good and the launch is repeated ticketed;
// a watchdog in the ticketed form is an error.  launch(ticket) enqueues the kernel(s) on c->stream.
struct LbLaunch {
    const char *err_name;   // what the error of a watchdog in the ticketed form starts with ("setop", "ukm_unique")
    const char *warn_name;  // what the warning of ukm_switch_to_tickets calls the kernel
    u64 watchdog;           // the kernel's watchdog bit (0: this launch has no look-back)
    bool bracket;           // ev_k0 / ev_k1 around the launch: it is the dominant kernel of the call
    bool ticket_first;
    bool first_zeroed;      // an earlier kernel of the stream has zeroed the block for the first attempt
};
int ukm_lb_launch(ukm_ctx *c, const LbCtl &b, const LbLaunch &how, const std::function<int(bool ticket)> &launch, u64 res[2]);

// ---- internal device-pointer entry points (all pointers are device pointers) ------------------
// internal fourth 2-way operation: merge keeping every record (k-way merge tree of ukm_merge_k)
#define UKM_OP_MERGE_INTERNAL 3
int ukm_dev_setop2(ukm_ctx *c, int op, const u64 *a, const u32 *ta, u64 na, const u64 *b,
                   const u32 *tb, u64 nb, u32 flags, u64 *out, u32 *tout, u64 out_cap,
                   u64 *n_out);
// (cta, ctb): the taxid of every record of a stream whose per-record pointer is null -- the file's global taxid
// (round 5; 0 = none).  Both constant: the plain-key kernel with a taxid epilogue.
int ukm_dev_setop2_ct(ukm_ctx *c, int op, const u64 *a, const u32 *ta, u32 cta, u64 na, const u64 *b,
                      const u32 *tb, u32 ctb, u64 nb, u32 flags, u64 *out, u32 *tout, u64 out_cap,
                      u64 *n_out);
// two or three operations of one pair (ops: 1 << UKM_OP_x each; the arrays are indexed by UKM_OP_x); flags may carry
// UKM_F_INTERNAL_PART_CACHE for the passes of the split route
int ukm_dev_setop2_multi(ukm_ctx *c, u32 ops, const u64 *a, const u32 *ta, u32 cta, u64 na, const u64 *b, const u32 *tb, u32 ctb,
                         u64 nb, u32 flags, u64 *const out[3], u32 *const tout[3], const u64 out_cap[3], u64 n_out[3]);
int ukm_dev_setop2_link(ukm_ctx *c, int op, const u64 *a, const u32 *ta, u64 na_max, const u64 *na_dev, const u64 *b,
                        const u32 *tb, u64 nb, u32 flags, u64 *out, u32 *tout, u64 out_cap, u64 *ctl, u32 cta = 0, u32 ctb = 0);
// fill n words with one value on the context's stream (file taxids; ukm_scan.hip)
int ukm_dev_fill_u32(ukm_ctx *c, u32 *dst, u64 n, u32 value);
// decisions over per-file taxids on the device (ukm_tax.hip): plan[0] = inter's left LCA fold, plan[2 + j] = diff -t keeps
int ukm_dev_ct_plan(ukm_ctx *c, const u32 *ct_host, int n, bool mix, u32 **plan);
// the keep bitmap of a rank filter (ukm_tax.hip): bit t = a record with taxid t passes, t = 0 .. tax_size - 1, in an even number
// of workspace words every one of which the kernel writes.  UKM_ERR_NO_TAXONOMY without a taxonomy or without ranks.
int ukm_dev_rank_bitmap(ukm_ctx *c, const char *name, const ukm_rank_filter *f, u32 **bits);
int ukm_dev_fill_u32_from(ukm_ctx *c, u32 *dst, u64 n, u32 value, const u32 *value_dev);  // value_dev != null: the value is read there
// internal flag of ukm_dev_setop2 / _ct (op DIFF, first stream with duplicate codes): the survivors are NOT collapsed to one
// record per code -- the caller is in the middle of an n-file fold (diff.go:437: mc1 = mc2 keeps every record; the map of
// diff.go:449-453 only shapes the final result) and collapses once at the end
#define UKM_F_INTERNAL_KEEP_DUPS 0x10000u
// internal flag of ukm_dev_setop2_ct, set by the public 2-way entry alone: both key streams are the CALLER's device memory
// (not arena copies, not an n-way route's intermediate), so the call may use the context's partition cache
#define UKM_F_INTERNAL_PART_CACHE 0x20000u
// flag bits of the set-op result word [1]
enum { UKM_SETOP_FLAG_DUP = 1, UKM_SETOP_FLAG_UNSORTED = 2, UKM_SETOP_FLAG_TIMEOUT = 4, UKM_SETOP_FLAG_STALE = 8 };
int ukm_dev_sort(ukm_ctx *c, u64 *keys, u32 *vals, u64 n, int key_bits);
// the same with the first scatter pass's digit histogram already counted by the producer of the keys (ukm_count)
int ukm_dev_sort_hist(ukm_ctx *c, u64 *keys, u32 *vals, u64 n, int key_bits, const u64 *first_hist, int first_shift);
int ukm_sort_first_shift(const ukm_ctx *c, u64 n, int key_bits);
int ukm_dev_unique(ukm_ctx *c, const u64 *keys, const u32 *taxids, u64 n, int mode, u64 *out,
                   u32 *tout, u64 out_cap, u64 *n_out);
// mode 5 = UNIQUE_LAST (last record of each run), 6 = COMMON (run length >= threshold)
int ukm_dev_unique_ex(ukm_ctx *c, const u64 *keys, const u32 *taxids, u64 n, int mode, u32 threshold,
                      u64 *out, u32 *tout, u64 out_cap, u64 *n_out);
int ukm_dev_check_sorted(ukm_ctx *c, const u64 *keys, u64 n, bool *sorted, bool *strict);
int ukm_dev_exclusive_scan_u64(ukm_ctx *c, const u64 *in, u64 *out, u64 n, u64 *total_dev);
