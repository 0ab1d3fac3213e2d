// ukm_sort_plan.h — what the radix sort decides on the host, as plain C++ (no HIP: tests/sort_plan_units.cpp compiles it
// with g++): the build knobs and thresholds, the bucket route's plan and admission test, the choice among the four routes,
// the size classes of the bucket kernel and the verdicts of the skew guard.  The kernels are in ukm_sort_kernels.h and
// ukm_sort_buckets.h, the host side that runs what is decided here in ukm_sort.hip, which alone includes this file; what a
// context keeps from one sort to the next is ukm_sort_state.h (SortPolicy, in ukm_ctx through ukm_internal.h).
#pragma once

#include <stdint.h>

typedef uint64_t u64;
typedef uint32_t u32;

// ---- build knobs, with their defaults ------------------------------------------------------------------------------------
// onesweep tile shapes (threads x keys per thread), measured on MI355X at 1e8 keys (profiles/r01_notes.md, r02_notes.md):
// keys only 1024x14 with the fused next-digit histogram (3.67 ms; round 1 without it: 512x14 4.15, 512x12 4.3,
// 512x15 5.3, 256x24 4.6, 768x10 4.9, 1024x7 5.1), key + taxid 1024x11 (5.1 ms; 768x14 5.1, 512x20 5.4, 512x12 6.4)
#ifndef SORT_NT_KEYS
#define SORT_NT_KEYS 1024
#endif
#ifndef SORT_VT_KEYS
#define SORT_VT_KEYS 14
#endif
#ifndef SORT_NT_PAIRS
#define SORT_NT_PAIRS 1024
#endif
#ifndef SORT_VT_PAIRS
#define SORT_VT_PAIRS 11
#endif
#ifndef SORT_LB_W
#define SORT_LB_W 4  /* tiles per hop of the scatter pass's look-back */
#endif
// (SORT_WAVES_PER_EU: no default; when given, the scatter pass is compiled for exactly that many waves per SIMD)
#ifndef LS_WALK_MAX
#define LS_WALK_MAX 4u  /* keys read by the walks, per key of the bucket, beyond which the bucket takes the digit passes (1.75 on evenly spread keys) */
#endif
#ifndef SORT_FUSED_MIN
#define SORT_FUSED_MIN (1ull << 24)
#endif
#ifndef SORT_LOCAL_MIN
#define SORT_LOCAL_MIN (1ull << 23)  // (measured: 1.2e7 keys 0.62 -> 0.50 ms, 6.7e6 equal, 1.5e6 slower)
#endif

constexpr int RB = 8;  // digit width: 8 passes for 57..64 bits.  (9 bits -- 7 passes for k = 31 codes -- measured slower in round 1)
constexpr u64 SORT_CHUNK_MIN = 1ull << 32;  // the scatter pass's tile / status arithmetic is 32-bit: from here chunks of 2^31, merged

// ---- the bucket route: the top `topb` bits by scatter passes, then every bucket inside LDS --------------------------------
constexpr int LS_NT = 256;                       // threads of the bucket kernel
constexpr int LS_TOP_MIN = 12, LS_TOP_MAX = 22;  // bucket = the top `topb` bits: 2^topb buckets of ~1400 keys
constexpr int LS_BUCKET_AVG = 1400;
constexpr int LS_MAX_BIG = 8192;  // buckets beyond 4096 keys, gathered side by side and sorted together by the general route
constexpr int LS_NCLASS = 12;
constexpr int LS_CLASS_KPT[LS_NCLASS] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16};  // keys per thread of the size classes: 256 ... 4096 keys
constexpr u32 LS_NSAMP = 1u << 20;  // keys the skew guard looks at

// Size class of a bucket of m keys: -1 none (empty), k < LS_NCLASS the smallest class that holds it, LS_NCLASS beyond every
// class (oversized).  (A bucket of one key still has a class: it has to reach the caller's array when the
// sorted-by-top-bits copy is the scratch.)
constexpr int ls_class_of(u64 m) {
    int k = -1;
    if (m > 0) {
        k = 0;
        while (k < LS_NCLASS && m > (u64)LS_NT * LS_CLASS_KPT[k]) k++;
    }
    return k;
}

// topb / npass for n keys: 2^topb ~ n / 1400.  Up to 1.3e8 keys the array is sorted by its top 16 bits at most (two scatter
// passes: a third costs more than larger buckets), beyond that by up to 22 (three passes).
static inline void ls_plan(u64 n, int *topb_out, int *npass_out) {
    int topb;
    if ((n >> 16) <= 2048) {
        topb = LS_TOP_MIN;
        while (topb < 16 && (n >> topb) > (u64)LS_BUCKET_AVG) topb++;
    } else {
        topb = 17;
        while (topb < LS_TOP_MAX && (n >> topb) > (u64)LS_BUCKET_AVG) topb++;
    }
    *topb_out = topb;
    *npass_out = topb <= 16 ? 2 : 3;
}

// The bucket route's admission test, stated once.  `enter`: a sort of n keys declared key_bits wide tries the route (it may
// still hand the call back: keys narrower than declared, crowded keys).  first_shift: the shift of the digit whose histogram
// the route builds first when the keys are as wide as declared, -1 when it does not enter or declines on the declared width.
struct BucketPlan {
    bool enter;
    int topb, npass;
    int min_bits;     // the top passes' digits + two digits for the buckets' own passes: narrower keys are declined
    int first_shift;
};
static inline BucketPlan bucket_plan(u64 n, int key_bits, bool local_enabled, bool general_only) {
    BucketPlan p;
    ls_plan(n, &p.topb, &p.npass);
    p.min_bits = RB * p.npass + 16;
    p.enter = n >= SORT_LOCAL_MIN && n < SORT_CHUNK_MIN && key_bits >= 32 && key_bits <= 64 && local_enabled && !general_only;
    p.first_shift = (p.enter && key_bits >= p.min_bits) ? key_bits - RB * p.npass : -1;
    return p;
}
// ... as a producer of the keys asks (ukm_sort_first_shift): a declared width of 64 makes the route read the OR of all keys
// before it settles its shift, so no histogram can be handed over
static inline int sort_first_shift(u64 n, int key_bits, bool local_enabled, bool general_only) {
    if (key_bits <= 0 || key_bits >= 64) return -1;
    return bucket_plan(n, key_bits, local_enabled, general_only).first_shift;
}

// ---- the route choice --------------------------------------------------------------------------------------------------
enum class SortRoute : int {  // the values of the statistic "sort_route"
    HOST_HIST = 1,  // every digit's histogram read back, constant digits dropped
    FUSED = 2,      // the first histogram by a pre-pass, every later one by the scatter pass before it
    BUCKETS = 3,    // top bits by scatter passes, then every bucket inside LDS
    CHUNKED = 4,    // chunks of 2^31 records, merged
};
// what sorts n keys when the bucket route is not taken, or hands the call back
static inline SortRoute sort_general_route(u64 n) { return n >= SORT_FUSED_MIN ? SortRoute::FUSED : SortRoute::HOST_HIST; }
static inline SortRoute sort_route(u64 n, int key_bits, bool local_enabled, bool general_only) {
    if (n >= SORT_CHUNK_MIN) return SortRoute::CHUNKED;
    if (bucket_plan(n, key_bits, local_enabled, general_only).enter) return SortRoute::BUCKETS;
    return sort_general_route(n);
}

// Skew guard: a bucket of 4096 keys holds 4096 * nsamp / n of nsamp evenly drawn samples on average; 25 % above that to let
// borderline buckets pass.
static inline u32 ls_sample_threshold(u64 n, u32 nsamp) {
    return (u32)((double)(LS_NT * LS_CLASS_KPT[LS_NCLASS - 1]) * 1.25 * (double)nsamp / (double)n) + 4;
}
// The verdict, from the sample (heavy buckets, samples in them, of nsamp) and from the real bucket sizes (oversized buckets,
// keys in them, of n) alike: the oversized buckets are gathered and sorted by ONE call of the general route, which is worth
// it for a few of them holding a minor share of the keys; else the general passes sort everything.
static inline bool ls_too_crowded(u64 big_buckets, u64 in_them, u64 of) { return big_buckets > (u64)LS_MAX_BIG || in_them > of / 4; }
