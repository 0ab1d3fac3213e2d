// ukm_sort_state.h — what a context keeps from one radix sort to the next (ukm_sort.hip), as plain C++ (no HIP:
// tests/sort_plan_units.cpp compiles it with g++): the skew memory, the policy of the buckets' counting step, the sort's
// statistics.  ukm_internal.h includes it: ukm_ctx::SortState adds the device resources the sort creates on first use.
#pragma once

#include <stdint.h>

typedef uint64_t u64;

struct SortPolicy {
    // set once a sort found its keys crowded into few buckets: later sorts look at a sample before they spend scatter passes
    bool skew_seen = false;
    void note_skew() { skew_seen = true; }
    // set around the sort of the gathered oversized buckets: those keys are crowded by construction, the general passes take them
    bool general_only = false;
    int depth = 0;  // sorts inside sorts (the chunks, the gathered buckets): only the outermost one records its route

    // The buckets' counting step.  A bucket whose keys crowd into few bins falls back to the digit passes and bumps a device
    // word; the NEXT bucket-route sort's classify kernel fetches it, so that it rides on that call's read-back.  Keys with many
    // copies each (k-mers of reads at coverage) make every bucket fall back: after a sort in which more than half did, the
    // next LS_COUNTING_SKIP sorts do not try.  knob: option "sort_counting" (-1 unset; 1 tries whatever happened; 0 never).
    static constexpr int LS_COUNTING_SKIP = 15;
    bool last_counting = false;  // the last bucket-route sort tried the counting step ...
    u64 last_buckets = 0;        // ... in this many buckets
    int counting_skip = 0;
    void note_fallbacks(u64 prev_fallbacks) { if (last_counting && prev_fallbacks * 2 > last_buckets) counting_skip = LS_COUNTING_SKIP; }
    bool want_counting(int knob) {
        if (knob == 0) return false;
        if (counting_skip > 0 && knob != 1) {
            counting_skip--;
            return false;
        }
        return true;
    }
    void note_launch(bool counting, u64 buckets) {
        last_counting = counting;
        last_buckets = buckets;
    }

    // statistics (ukm_ctx_get_stat)
    u64 stat_route = 0;                      // "sort_route": the route (SortRoute, ukm_sort_plan.h) that completed the last outermost sort
    u64 stat_bucket_declined = 0;            // "sort_bucket_declined": times the bucket route was entered and handed the call back
    u64 stat_oversized_buckets = 0;          // "sort_oversized_buckets": buckets the last outermost bucket-route sort gathered
    unsigned long long stat_fused_hist = 0;  // "sort_fused_hist": sorts that took their first histogram from the producer of the keys (ukm_count)
};
