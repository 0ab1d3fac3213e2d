// ukm_probe.hip — the samplers of the hash-probe routes (hit rate, overlap, range load, new codes) and the host steps the
// routes share (ukm_probe.h).  The routes themselves: ukm_probe_union.hip, ukm_probe_ranked.hip, ukm_place.hip.
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "ukm_kway.h"
#include "ukm_probe.h"

namespace {

__device__ __forceinline__ u64 pu_splitmix(u64 x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// heaviest range: records of all later files inside one range (ctl[4] = max over the ranges)
__global__ void pu_load_kernel(PuArgs a) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.R) return;
    u64 sum = 0;
    for (u32 j = 0; j < a.S1; j++) {
        const u64 b = a.cuts[(u64)r * a.S1 + j], e = a.cuts[(u64)(r + 1) * a.S1 + j];
        sum += e > b ? e - b : 0;
    }
    atomicMax((unsigned long long *)&a.ctl[4], (unsigned long long)sum);
}

// hit rate of a sample of later records in the base set
__global__ void pu_sample_kernel(PuArgs a, u32 nsamp, u32 nfiles_s) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    bool tested = false, hit = false, same = false, run = false;
    if (i < nsamp) {
        const u32 j = (u32)(((u64)(i % nfiles_s) * a.S1) / nfiles_s);
        const u64 len = a.lens[j];
        if (len) {
            // sample t of its file sits in the t-th of spf equal strides, at a hashed place inside it: no record is drawn
            // twice (pu_new_codes counts EQUAL sampled records; drawing with replacement showed it pairs that are one record)
            const u64 spf = (nsamp + nfiles_s - 1) / nfiles_s, t = i / nfiles_s;
            const u64 lo_p = (u64)(((unsigned __int128)t * len) / spf), hi_p = (u64)(((unsigned __int128)(t + 1) * len) / spf);
            const u64 key = as_global(a.files[j])[hi_p > lo_p ? lo_p + pu_splitmix(i) % (hi_p - lo_p) : (lo_p < len ? lo_p : len - 1)];
            u64 lo = 0, hi = a.n0;
            while (lo < hi) {
                const u64 mid = (lo + hi) >> 1;
                if (a.base[mid] < key) lo = mid + 1; else hi = mid;
            }
            tested = true;
            hit = lo < a.n0 && a.base[lo] == key;
            // (records with taxids: does the record's taxid differ from the entry's and lie in the entry's clade?  Those are
            //  the records that need their exact pre-order number in the fold: PuArgs::clade_mode)
            if (hit && a.tax.clade8 && a.tfiles && (a.base_tax || a.base_ct)) {
                const u32 *tf = a.tfiles[j];
                const u64 at = hi_p > lo_p ? lo_p + pu_splitmix(i) % (hi_p - lo_p) : (lo_p < len ? lo_p : len - 1);
                const u32 t = tf ? tf[at] : (a.cte ? (u32)a.cte[j] : 0u);
                const u32 bt = a.base_tax ? a.base_tax[lo] : a.base_ct;
                same = t != bt && t < a.tax.size && bt < a.tax.size && a.tax.clade8[t] == a.tax.clade8[bt];
                // (and does the file's NEXT record carry the same taxid?  Files whose neighbouring records share their taxid -- one
                //  taxid per genome, taxids assigned by clade -- read the 4-byte numbers from lines they have just used)
                run = !tf || (at + 1 < len && tf[at + 1] == t);
            }
            // (the sampled records the base set lacks are kept: how many DISTINCT new codes the files bring is read off
            //  the equal pairs among them, pu_new_codes)
            if (!hit && a.miss) {
                const u64 at = atomicAdd((unsigned long long *)&a.ctl[5], 1ull);
                if (at < a.miss_cap) a.miss[at] = key;
            }
        }
    }
    const u64 mh = __ballot(hit), mt = __ballot(tested), ms = __ballot(same), mr = __ballot(run);
    if (lane_id() == 0 && mt) {
        atomicAdd((unsigned long long *)&a.ctl[2], (unsigned long long)__popcll(mh));
        atomicAdd((unsigned long long *)&a.ctl[3], (unsigned long long)__popcll(mt));
        if (ms) atomicAdd((unsigned long long *)&a.ctl[6], (unsigned long long)__popcll(ms));
        if (mr) atomicAdd((unsigned long long *)&a.ctl[7], (unsigned long long)__popcll(mr));
    }
}

// cte[j]: the file taxid in the low word (host) gets its pre-order number in the high word
__global__ void pu_cte_kernel(u64 *cte, u32 n, TaxDev T, u32 clade_mode = 0) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const u32 t = (u32)cte[j];
    u32 e = T.euler ? T.euler[t < T.size ? t : 0u] : 0u;
    if (clade_mode && e) e |= (u32)T.clade8[t] << 24;  // (PuArgs::clade_mode: the numbers carry their clade code)
    cte[j] = (u64)t | ((u64)e << 32);
}


// Do the files share codes at all?  Records drawn from random files are looked up in ONE other random file each: the
// share that is found estimates how much of a collection a file holds.  (The chunk files of an out-of-core sort share
// nothing: without this look the placement merge below would build a base set and sample it before it declines.)
__global__ void pu_overlap_kernel(PuArgs a, u32 nsamp) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    bool tested = false, hit = false;
    if (i < nsamp && a.S1 >= 2) {
        const u64 h = pu_splitmix(i);
        const u32 fa = (u32)(h % a.S1), fb = (fa + 1 + (u32)((h >> 20) % (a.S1 - 1))) % a.S1;
        const u64 la = a.lens[fa], lb = a.lens[fb];
        if (la && lb) {
            const u64 key = as_global(a.files[fa])[pu_splitmix(h) % la];
            const auto f = as_global(a.files[fb]);
            u64 lo = 0, hi = lb;
            while (lo < hi) {
                const u64 mid = (lo + hi) >> 1;
                if (f[mid] < key) lo = mid + 1; else hi = mid;
            }
            tested = true;
            hit = lo < lb && f[lo] == key;
        }
    }
    const u64 mh = __ballot(hit), mt = __ballot(tested);
    if (lane_id() == 0 && mt) {
        atomicAdd((unsigned long long *)&a.ctl[2], (unsigned long long)__popcll(mh));
        atomicAdd((unsigned long long *)&a.ctl[3], (unsigned long long)__popcll(mt));
    }
}

}  // namespace

int ukm_punion_mode(const ukm_ctx *c) { return ukm_env_int(c, "UKM_PUNION", -1); }

int ukm_punion_tax_mode(const ukm_ctx *c) { return ukm_env_int(c, "UKM_PUNION_TAX", -1); }

// PuArgs::clade_mode from the sample (hits: sampled later records found in the base set, same: those of them whose taxid
// differs from the entry's and lies in the entry's clade -- the records whose exact number the fold would have to fetch on
// the spot).  Unrelated taxa: next to none.  Related taxa (one species' strains): most -- the numbers are then read for
// every record in the pipeline's second stage, as in rounds 4-5.  UKM_PUNION_CLADE=0 / 1: never / always.
// runs: hits whose file's next record carries the same taxid: with most of them the numbers come from lines the wave has just
// used and the plain fold is the faster one (config 3's files with one taxid each as arrays: probe pass 27.5 ms against 34.0 in
// clade mode; uniformly random taxids: 67.8 against 41.7).
u32 ukm_pu_clade_mode(const ukm_ctx *c, const TaxDev &T, bool tax, u64 hits, u64 same, u64 runs) {
    if (!tax || T.clade8 == nullptr || T.pair == nullptr || T.euler == nullptr) return 0u;
    const int k = ukm_env_int(c, "UKM_PUNION_CLADE", -1);
    if (k == 0) return 0u;
    if (k == 1) return 1u;
    return (hits > 0 && same * 16 < hits && runs * 2 < hits) ? 1u : 0u;
}

// equal neighbours in a sorted array
__global__ void pu_eqpairs_kernel(const u64 *k, u64 n, u64 *out) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const bool eq = g > 0 && g < n && k[g] == k[g - 1];
    const u64 m = __ballot(eq);
    if (m && lane_id() == 0) atomicAdd((unsigned long long *)out, (unsigned long long)__popcll(m));
}

// How many DISTINCT codes do the later files add to the base set?  `smiss` holds the m sampled records the base set lacks
// (pu_sample_kernel).  Two records drawn from the files' new records carry the same code with probability 1 / (distinct new
// codes), so m (m - 1) / 2 pairs show about that many equal pairs: distinct ~ m (m - 1) / (2 pairs) (solved exactly below,
// for samples that see a code several times), and at least the number that would show ONE pair when none is seen (the sample is sized so that a count that just fills the tables'
// room would show about four).  The tables of a range take as many new codes as the range has base
// entries; what comes beyond is listed record by record through global atomics (100 strains that each bring 3 % PRIVATE
// k-mers: 13.5 M new codes on a base set of 5.6 M -- the probe pass took 4.9 ms where the k-way merge finishes the whole
// union in 3.4).  Only looked at when the files' new RECORDS outnumber the room at all.  *too_many: the estimate exceeds it.
static int pu_new_codes(ukm_ctx *c, PuArgs a, u32 nf, double miss_rate, u64 later, bool *too_many) {
    *too_many = false;
    const double expected_misses = (double)later * miss_rate, room = 1.25 * (double)a.n0;
    if (expected_misses <= room || miss_rate <= 0.0) return UKM_OK;
    // enough sampled new records to see ~4 equal pairs if the distinct new codes just filled the tables' room
    const double want = std::sqrt(8.0 * room);
    const u64 nsamp = (u64)std::min(4194304.0, std::max(65536.0, want / miss_rate));
    WsMark mk = ws_mark(c);
    u64 *smiss = nullptr;
    UKM_TRY(ws_alloc_t(c, (size_t)nsamp, &smiss));
    UKM_HIP(hipMemsetAsync(a.ctl, 0, 8 * sizeof(u64), c->stream));
    a.miss = smiss;
    a.miss_cap = nsamp;
    hipLaunchKernelGGL(pu_sample_kernel, dim3((unsigned)((nsamp + 255) / 256)), dim3(256), 0, c->stream, a, (u32)nsamp, nf);
    UKM_HIP(hipGetLastError());
    u64 m = 0;
    UKM_TRY(ukm_read_u64(c, a.ctl + 5, &m));
    m = std::min<u64>(m, nsamp);
    u64 pairs = 0;
    if (m >= 2) {
        UKM_TRY(ukm_dev_sort(c, smiss, nullptr, m, 64));
        hipLaunchKernelGGL(pu_eqpairs_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, smiss, m, a.ctl + 6);
        UKM_HIP(hipGetLastError());
        UKM_TRY(ukm_read_u64(c, a.ctl + 6, &pairs));
    }
    UKM_HIP(hipMemsetAsync(a.ctl, 0, 8 * sizeof(u64), c->stream));
    ws_release(c, mk);
    // `pairs` = equal NEIGHBOURS of the sorted sample, so m - pairs distinct codes were seen; m draws from D equally likely
    // codes show D (1 - exp(-m / D)) distinct ones: solved for D (few pairs: D ~ m^2 / (2 pairs); a sample that has seen most
    // codes several times: D ~ the codes seen).  No pair at all: at least what would have shown one.
    double distinct = expected_misses;
    if (m >= 2) {
        const double seen = (double)(m - std::min<u64>(std::max<u64>(pairs, 1), m - 1)), ratio = seen / (double)m;
        double lo = 1e-12, hi = 64.0;  // x = m / D; (1 - exp(-x)) / x falls from 1 to 0
        for (int it = 0; it < 80; it++) {
            const double x = 0.5 * (lo + hi);
            if (-std::expm1(-x) / x > ratio) lo = x; else hi = x;
        }
        distinct = std::min(expected_misses, (double)m / (0.5 * (lo + hi)));
    }
    *too_many = distinct > room;
    if (ukm_env(c, "UKM_PUNION_DEBUG"))
        fprintf(stderr, "[punion] %llu sampled new records, %llu equal pairs: ~%.3g distinct new codes among %.3g new records, base set %llu%s\n",
                (unsigned long long)m, (unsigned long long)pairs, distinct, expected_misses, (unsigned long long)a.n0, *too_many ? " -> not this route" : "");
    return UKM_OK;
}

int ukm_pu_overlap_sample(ukm_ctx *c, const PuArgs &a, u64 h[4]) {
    const u32 nsamp = 1u << 14;
    hipLaunchKernelGGL(pu_overlap_kernel, dim3(nsamp / 256), dim3(256), 0, c->stream, a, nsamp);
    UKM_HIP(hipGetLastError());
    return ukm_read_u64(c, a.ctl, h, 4);
}

// the share of sampled records that are found in another file; the workspace it takes is given back
int ukm_pu_overlap_share(ukm_ctx *c, const UkmStreams &in, double *share) {
    *share = 0.0;
    WsMark m = ws_mark(c);
    StreamTab tab;
    u64 *ctl = nullptr;
    UKM_TRY(ukm_stream_tab(c, in, &tab));
    UKM_TRY(ws_alloc_t(c, 8, &ctl));
    UKM_HIP(hipMemsetAsync(ctl, 0, 8 * sizeof(u64), c->stream));
    PuArgs a;
    memset(&a, 0, sizeof(a));
    a.files = tab.keys();
    a.lens = tab.lens();
    a.S1 = (u32)in.S;
    a.ctl = ctl;
    u64 h[4] = {0, 0, 0, 0};
    UKM_TRY(ukm_pu_overlap_sample(c, a, h));
    ws_release(c, m);
    if (h[3]) *share = (double)h[2] / (double)h[3];
    return UKM_OK;
}

int ukm_pu_tax_ready(ukm_ctx *c, const u32 *tout, const char *op, bool *ready) {
    if (!tout) UKM_FAIL(UKM_ERR_INVALID, "%s: taxids given but out_taxids is NULL", op);
    if (c->tax_parent == nullptr) UKM_FAIL(UKM_ERR_NO_TAXONOMY, "%s: records carry taxids but no taxonomy is loaded", op);
    *ready = c->tax_euler != nullptr && c->tax_node_at != nullptr;
    return UKM_OK;
}

// (a small first file -- a plasmid in front of the genomes -- would leave the tables nearly empty and every later record
//  a new code; a union does not depend on the order of its files, and neither does the TaxId fold)
std::vector<int> ukm_pu_largest(const u64 *lens, int S, int k0, std::vector<char> *in_base) {
    std::vector<int> ord((size_t)S);
    for (int j = 0; j < S; j++) ord[(size_t)j] = j;
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return lens[x] > lens[y]; });
    in_base->assign((size_t)S, 0);
    for (int j = 0; j < k0; j++) (*in_base)[(size_t)ord[(size_t)j]] = 1;
    return ord;
}

int ukm_pu_base_union(ukm_ctx *c, const UkmStreams &b, u64 **base, u32 **base_tax, u64 *n0) {
    u64 cap0 = 0;
    std::vector<const u32 *> bt((size_t)b.S, nullptr);
    for (int j = 0; j < b.S; j++) {
        cap0 += b.lens[j];
        if (!b.tax) continue;
        bt[(size_t)j] = b.taxids ? b.taxids[j] : nullptr;
        if (!bt[(size_t)j] && b.file_taxid(j) != 0 && b.lens[j]) {
            u32 *t = nullptr;
            UKM_TRY(ws_alloc_t(c, b.lens[j], &t));
            UKM_TRY(ukm_dev_fill_u32(c, t, b.lens[j], b.file_taxid(j)));
            bt[(size_t)j] = t;
        }
    }
    *base_tax = nullptr;
    UKM_TRY(ws_alloc_t(c, cap0 + 1, base));
    if (b.tax) UKM_TRY(ws_alloc_t(c, cap0 + 1, base_tax));
    bool kw_declined = true;
    UKM_TRY(ukm_dev_kway(c, UkmStreams{b.keys, b.tax ? bt.data() : nullptr, nullptr, b.lens, b.S, b.tax}, UKM_KWAY_UNION,
                         UkmOut{*base, *base_tax, cap0, n0}, &kw_declined));
    if (kw_declined) *n0 = 0;
    return UKM_OK;
}

int ukm_pu_attempts(ukm_ctx *c, int k0, int S, double min_hit, bool *low_hit, const std::function<int(int, bool *, double *)> &attempt) {
    c->stat_punion_attempts = 0;
    c->stat_punion_flags = 0;  // (an attempt that declines in front of its probe pass leaves no earlier call's flags behind)
    for (int n = 0;; n++) {
        const WsMark m = ws_mark(c);
        c->stat_punion_attempts++;
        double hit = 0.0;
        *low_hit = false;
        UKM_TRY(attempt(k0, low_hit, &hit));
        if (!*low_hit) return UKM_OK;
        ws_release(c, m);  // (a low hit gives its workspace back, whether or not another attempt follows)
        const double miss4 = (1.0 - hit) * (1.0 - hit) * (1.0 - hit) * (1.0 - hit);
        k0 *= 4;
        if (n > 0 || 1.0 - miss4 < min_hit || k0 > S / 4) return UKM_OK;
    }
}

int ukm_pu_hit_sample(ukm_ctx *c, const PuArgs &a, u64 h[8], int words) {
    const u32 nsamp = 1u << 16, nf = std::min(a.S1, 16u);
    hipLaunchKernelGGL(pu_sample_kernel, dim3(nsamp / 256), dim3(256), 0, c->stream, a, nsamp, nf);
    UKM_HIP(hipGetLastError());
    for (int i = 0; i < 8; i++) h[i] = 0;
    return ukm_read_u64(c, a.ctl, h, words);
}

int ukm_pu_hit_guard(ukm_ctx *c, const PuArgs &a, double miss_rate, double min_hit, u64 later, bool *low_hit, bool *too_many) {
    const int mode = ukm_punion_mode(c);
    *low_hit = mode != 2 && 1.0 - miss_rate < min_hit;
    *too_many = false;
    if (mode != 2 && !*low_hit) UKM_TRY(pu_new_codes(c, a, std::min(a.S1, 16u), miss_rate, later, too_many));
    return UKM_OK;
}

int ukm_pu_cte(ukm_ctx *c, u64 *cte, u32 n, u32 clade_mode) {
    hipLaunchKernelGGL(pu_cte_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, cte, n, ukm_taxdev(c), clade_mode);
    UKM_HIP(hipGetLastError());
    return UKM_OK;
}

int ukm_pu_range_load(ukm_ctx *c, const PuArgs &a, u64 records, bool say, bool *heavy) {
    hipLaunchKernelGGL(pu_load_kernel, dim3((a.R + 255) / 256), dim3(256), 0, c->stream, a);
    UKM_HIP(hipGetLastError());
    u64 heaviest = 0;
    UKM_TRY(ukm_read_u64(c, a.ctl + 4, &heaviest));
    const u64 avg = records / a.R + 1;
    if (say) fprintf(stderr, "[punion] heaviest range %llu records, average %llu\n", (unsigned long long)heaviest, (unsigned long long)avg);
    *heavy = ukm_punion_mode(c) != 2 && heaviest > 64 * avg + 65536;
    return UKM_OK;
}

int ukm_pu_probe_batches(ukm_ctx *c, PuArgs &a, int S1, const u64 *hlens, PuLap &lap, bool say, bool *heavy,
                     const std::function<void(const PuArgs &)> &probe) {
    const PuArgs all = a;
    for (int s0 = 0; s0 < S1; s0 += PU_MAXS) {
        const int s1 = std::min(PU_MAXS, S1 - s0);
        a.files = all.files + s0;
        a.lens = all.lens + s0;
        a.tfiles = all.tfiles ? all.tfiles + s0 : nullptr;
        a.cte = all.cte ? all.cte + s0 : nullptr;
        a.S1 = (u32)s1;
        WsMark mark = ws_mark(c);
        UKM_TRY(ws_alloc_t(c, ((size_t)a.R + 1) * s1, &a.cuts));
        UKM_TRY(pu_launch_cuts(c, a));
        lap("cuts");
        u64 records = 0;
        for (int j = 0; j < s1; j++) records += hlens[s0 + j];
        UKM_TRY(ukm_pu_range_load(c, a, records, say, heavy));
        if (*heavy) {
            ws_release(c, mark);
            return UKM_OK;
        }
        UKM_HIP(hipMemsetAsync(a.ctl + 4, 0, sizeof(u64), c->stream));
        (void)hipEventRecord(c->ev_k0, c->stream);
        probe(a);
        (void)hipEventRecord(c->ev_k1, c->stream);
        c->evk_valid = true;
        UKM_HIP(hipGetLastError());
        lap("probe");
        ws_release(c, mark);  // (the stream orders the next batch's cuts behind this probe)
    }
    return UKM_OK;
}

int ukm_pu_finish(ukm_ctx *c, const PuArgs &a, u64 nm, const u64 *base, const u32 *base_tax, u64 n0, const UkmOut &o, PuLap &lap,
              const char *sort_stage, bool *declined) {
    const bool tax = base_tax != nullptr;
    if (nm == 0) {
        UKM_TRY(ukm_route_answer(n0, o, declined));
        UKM_HIP(hipMemcpyAsync(o.keys, base, n0 * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
        if (tax) UKM_HIP(hipMemcpyAsync(o.taxids, base_tax, n0 * sizeof(u32), hipMemcpyDeviceToDevice, c->stream));
        return UKM_OK;
    }
    UKM_TRY(ukm_dev_sort(c, a.miss, a.miss_tax, nm, 64));
    u64 *mu = nullptr;
    u32 *mut = nullptr;
    UKM_TRY(ws_alloc_t(c, nm + 1, &mu));
    if (tax) UKM_TRY(ws_alloc_t(c, nm + 1, &mut));
    u64 nmu = 0;
    UKM_TRY(ukm_dev_unique(c, a.miss, a.miss_tax, nm, UKM_UNIQUE, mu, mut, nm, &nmu));
    lap(sort_stage);
    // (capacity: the 2-way kernel reports the size it needs)
    UKM_TRY(ukm_dev_setop2(c, UKM_OP_UNION, base, base_tax, n0, mu, mut, nmu, 0, o.keys, o.taxids, o.cap, o.n));
    lap("final");
    *declined = false;
    return UKM_OK;
}
