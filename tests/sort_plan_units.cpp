// The radix sort's host decisions (unikmer_amd/csrc/ukm_sort_plan.h, ukm_sort_state.h) as a stand-alone program: plain C++, built by
// tests/test_sort_plan_cpu.py with g++ under the address and undefined-behaviour sanitizers.  Prints "OK" or the first
// property that does not hold.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ukm_sort_plan.h"
#include "ukm_sort_state.h"

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
            exit(1);                                      \
        }                                                 \
    } while (0)

// every power of two from 2^23 to 2^31 and 2^32 - 1, +-1 around each, and around 2048 * 2^16 where the plan changes its branch
static std::vector<u64> sizes() {
    std::vector<u64> v;
    for (int e = 23; e <= 31; e++)
        for (int d = -1; d <= 1; d++) v.push_back((1ull << e) + d);
    v.push_back((1ull << 32) - 2);
    v.push_back((1ull << 32) - 1);
    for (int d = -1; d <= 1; d++) v.push_back((2048ull << 16) + d);
    for (int d = -1; d <= 1; d++) v.push_back((2049ull << 16) + d);
    return v;
}

static void test_plan() {
    for (u64 n : sizes()) {
        int topb = 0, npass = 0;
        ls_plan(n, &topb, &npass);
        CHECK(topb >= LS_TOP_MIN && topb <= LS_TOP_MAX, "n %llu topb %d", (unsigned long long)n, topb);
        CHECK(topb >= 12 && topb <= 22, "n %llu topb %d", (unsigned long long)n, topb);
        CHECK(npass == (topb <= 16 ? 2 : 3), "n %llu topb %d npass %d", (unsigned long long)n, topb, npass);
        // (the caps: 16 inside the two-pass branch, 22 overall)
        const int cap = (n >> 16) <= 2048 ? 16 : 22;
        if (topb < cap) CHECK((n >> topb) <= 1400, "n %llu topb %d", (unsigned long long)n, topb);
        if (topb > 12 && topb != 17) CHECK((n >> (topb - 1)) > 1400, "n %llu: topb %d is not the smallest", (unsigned long long)n, topb);
    }
}

// the admission test, stated independently of bucket_plan, against what ukm_sort_first_shift hands the producer of the keys
static void test_admission() {
    std::vector<u64> ns = sizes();
    ns.push_back((1ull << 23) - 2);
    ns.push_back(1ull << 32);
    ns.push_back((1ull << 32) + 1);
    for (u64 n : ns)
        for (int bits = 1; bits <= 64; bits++)
            for (int local = 0; local <= 1; local++)
                for (int general = 0; general <= 1; general++) {
                    int topb = 0, npass = 0;
                    ls_plan(n, &topb, &npass);
                    const BucketPlan p = bucket_plan(n, bits, local != 0, general != 0);
                    const bool enter = n >= (1ull << 23) && n < (1ull << 32) && bits >= 32 && local && !general;
                    CHECK(p.enter == enter, "n %llu bits %d local %d general %d", (unsigned long long)n, bits, local, general);
                    CHECK(p.topb == topb && p.npass == npass && p.min_bits == 8 * npass + 16, "n %llu", (unsigned long long)n);
                    CHECK(p.first_shift == -1 || p.first_shift == bits - 8 * npass, "n %llu bits %d shift %d", (unsigned long long)n, bits, p.first_shift);
                    CHECK((p.first_shift >= 0) == (enter && bits >= p.min_bits), "n %llu bits %d", (unsigned long long)n, bits);
                    const int fs = sort_first_shift(n, bits, local != 0, general != 0);
                    CHECK(fs == (bits < 64 ? p.first_shift : -1), "n %llu bits %d: %d against %d", (unsigned long long)n, bits, fs, p.first_shift);
                    CHECK(fs == -1 || (fs == bits - 8 * npass && fs >= 16), "n %llu bits %d shift %d", (unsigned long long)n, bits, fs);
                    // the route choice enters the bucket route exactly where the predicate says
                    CHECK((sort_route(n, bits, local != 0, general != 0) == SortRoute::BUCKETS) == enter, "n %llu bits %d", (unsigned long long)n, bits);
                }
}

static void test_classes() {
    int prev = -1;
    for (u64 m = 0; m <= 4097; m++) {
        const int k = ls_class_of(m);
        CHECK(k >= prev, "size %llu: class %d after %d", (unsigned long long)m, k, prev);
        if (m == 0) CHECK(k == -1, "an empty bucket has class %d", k);
        else CHECK(k >= 0 && k <= LS_NCLASS, "size %llu class %d", (unsigned long long)m, k);
        if (k >= 0 && k < LS_NCLASS) {
            CHECK(m <= 256ull * LS_CLASS_KPT[k], "size %llu does not fit class %d", (unsigned long long)m, k);
            if (k > 0) CHECK(m > 256ull * LS_CLASS_KPT[k - 1], "size %llu fits class %d", (unsigned long long)m, k - 1);
        }
        prev = k;
    }
    CHECK(ls_class_of(4096) == LS_NCLASS - 1 && ls_class_of(4097) == LS_NCLASS, "the largest class ends at 4096 keys");
    for (int k = 1; k < LS_NCLASS; k++) CHECK(LS_CLASS_KPT[k] > LS_CLASS_KPT[k - 1], "class %d", k);
}

static void test_routes() {
    const u64 L = SORT_LOCAL_MIN, F = SORT_FUSED_MIN;
    CHECK(L <= F, "the thresholds' order");
    struct { u64 n; SortRoute wide, knob_off; } rows[] = {
        {L - 1, SortRoute::HOST_HIST, SortRoute::HOST_HIST}, {L, SortRoute::BUCKETS, SortRoute::HOST_HIST},
        {F - 1, SortRoute::BUCKETS, SortRoute::HOST_HIST},   {F, SortRoute::BUCKETS, SortRoute::FUSED},
        {(1ull << 32) - 1, SortRoute::BUCKETS, SortRoute::FUSED}, {1ull << 32, SortRoute::CHUNKED, SortRoute::CHUNKED},
    };
    for (auto &r : rows) {
        CHECK(sort_route(r.n, 62, true, false) == r.wide, "n %llu", (unsigned long long)r.n);
        CHECK(sort_route(r.n, 64, true, false) == r.wide, "n %llu", (unsigned long long)r.n);
        CHECK(sort_route(r.n, 62, false, false) == r.knob_off, "n %llu, UKM_SORT_LOCAL=0", (unsigned long long)r.n);
        CHECK(sort_route(r.n, 62, true, true) == r.knob_off, "n %llu, the gathered buckets' sort", (unsigned long long)r.n);
        CHECK(sort_route(r.n, 31, true, false) == r.knob_off, "n %llu, 31-bit keys", (unsigned long long)r.n);
        if (r.n < (1ull << 32)) CHECK(sort_general_route(r.n) == r.knob_off, "n %llu", (unsigned long long)r.n);
    }
    CHECK((int)SortRoute::HOST_HIST == 1 && (int)SortRoute::FUSED == 2 && (int)SortRoute::BUCKETS == 3 && (int)SortRoute::CHUNKED == 4,
          "the values of the statistic sort_route");
    // the sample threshold: the samples a bucket of 4096 keys holds on average, a quarter more, plus 4
    CHECK(ls_sample_threshold(1ull << 23, 1u << 20) == 644, "%u", ls_sample_threshold(1ull << 23, 1u << 20));
    CHECK(ls_sample_threshold(1ull << 20, 1u << 20) == 5124, "%u", ls_sample_threshold(1ull << 20, 1u << 20));
}

// one bucket-route sort as sort_buckets drives the policy: the previous sort's fall-backs arrive, then the decision
static bool one_sort(SortPolicy &s, int knob, u64 prev_fallbacks, u64 buckets) {
    s.note_fallbacks(prev_fallbacks);
    const bool counting = s.want_counting(knob);
    s.note_launch(counting, buckets);
    return counting;
}

static void test_counting_policy() {
    const u64 B = 1000;
    {   // more than half fell back: exactly the next 15 sorts skip
        SortPolicy s;
        CHECK(one_sort(s, -1, 0, B), "the first sort tries");
        CHECK(one_sort(s, -1, B / 2, B), "half is not more than half");            // (reports sort 1's fall-backs: exactly half)
        CHECK(!one_sort(s, -1, B / 2 + 1, B), "more than half: this sort skips");  // (sort 2's: more than half) skip 1
        for (int i = 2; i <= 15; i++) CHECK(!one_sort(s, -1, 0, B), "skip %d", i);
        CHECK(one_sort(s, -1, 0, B), "the 16th tries again");
        CHECK(one_sort(s, -1, 0, B), "and goes on");
    }
    {   // fall-backs reported behind a sort that did not try do not re-arm the skip
        SortPolicy s;
        one_sort(s, -1, 0, B);
        CHECK(!one_sort(s, -1, B, B), "skip 1");
        for (int i = 2; i <= 15; i++) CHECK(!one_sort(s, -1, B, B), "skip %d", i);
        CHECK(one_sort(s, -1, B, B), "the skipped sorts' reports count for nothing");
    }
    {   // sort_counting = 1 overrides the skip (and does not use it up); 0 always wins
        SortPolicy s;
        one_sort(s, -1, 0, B);
        CHECK(!one_sort(s, -1, B, B), "skip 1");
        CHECK(one_sort(s, 1, 0, B), "sort_counting = 1 tries whatever happened");
        CHECK(s.counting_skip == 14, "%d", s.counting_skip);
        CHECK(!one_sort(s, 0, 0, B), "sort_counting = 0 never tries");
        CHECK(s.counting_skip == 14, "0 does not use the skip up: %d", s.counting_skip);
        SortPolicy t;
        for (int i = 0; i < 40; i++) CHECK(!one_sort(t, 0, 0, B), "sort_counting = 0, sort %d", i);
        for (int i = 0; i < 40; i++) CHECK(one_sort(t, 1, B, B), "sort_counting = 1, sort %d", i);
    }
    SortPolicy s;
    CHECK(!s.skew_seen, "a new context has met no crowded keys");
    s.note_skew();
    CHECK(s.skew_seen, "note_skew");
}

int main() {
    test_plan();
    test_admission();
    test_classes();
    test_routes();
    test_counting_policy();
    printf("OK\n");
    return 0;
}
