// ukm_select.hip — order-preserving record selection: ukm_grep (grep.go:617-676), ukm_filter (filter.go:181-221),
// ukm_sample (sample.go:134-148) and ukm_rfilter (rfilter.go:280-304).  On the device grep, filter and rfilter are ONE
// operation: a predicate per record, the survivors written in input order with their own taxids (copied, never folded: no
// sorted input, every duplicate kept; only rfilter's bitmap is built from a taxonomy).
//
// select_kernel<PRED, TAX, TICKET>: a tile is 256 threads x 8 consecutive records (16-byte loads where the arrays are
// 16-byte aligned); the predicate answers all eight records of a thread at once (so that a membership predicate has eight
// independent lookups in flight); the block scan of ukm_device.h and lb_tile_base<TICKET> give the tile its output base
// (launch protocol: ukm_device.h, ukm_lb_launch); the survivors go through LDS so that a tile's stores are contiguous.
// Predicates:
//   FilterPred<W>  the low-complexity score of filterCode without a score array: "base i equals base i - 1" is one bit per
//                  base (W = u32 for k <= 32, u64 above), a window's sum is window * penalty_d + (penalty_s - penalty_d) *
//                  popcount(window bits), and "some tested sum >= threshold" is "the largest popcount >= need" with `need`
//                  worked out once on the host (penalty_s < penalty_d: the bits are inverted and the roles swap).
//   GrepLds        the distinct queries in an open-addressing table in LDS (4096 slots, at most GREP_LDS_MAX queries: load
//                  <= 0.5), built once per workgroup; the workgroup is PERSISTENT over tiles, lookups never leave the CU.
//   GrepDir        the queries sorted and deduplicated on the device (ukm_dev_sort + ukm_dev_unique) behind the prefix
//                  directory of ukm_dir.h: a directory pair plus a short search per record, as the window join of ukm_map.
//   TaxidPred      one bit per taxid in 0 .. max queried taxid (ukm_rfilter: the keep bitmap of the rank filter, one bit per
//                  id of the taxonomy).
// ukm_sample is a strided gather: no scan, no look-back.
#include <algorithm>

#include "ukm_device.h"
#include "ukm_dir.h"

namespace {

constexpr int NT = 256;
constexpr int VT = 8;  // consecutive records per thread
constexpr int TILE = NT * VT;
enum : u64 { SEL_FLAG_TIMEOUT = 4 };  // result word [1]

struct SelArgs {
    const u64 *k;
    const u32 *t;
    u64 n;
    u64 *out;
    u32 *tout;
    u64 out_cap;
    u64 *status;
    u32 *ticket;
    u64 *result;  // [0] records kept, [1] flags
    u64 ntiles;
};

// ---- predicates ---------------------------------------------------------------------------------------------------------
// keep(): x[s], t[s] = the records of one thread (bit s of `valid`: present); returns the mask of the kept ones and may
// replace x[s] by the code that is to be written.  setup(): once per workgroup, every thread, in front of the first tile.
struct NoShared {
    u32 unused;
};

// the even bits of x (bit 2j -> bit j); odd bits of x must be clear
__device__ __forceinline__ u32 even_bits16(u32 x) {
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}

template <typename W>
struct FilterPred {
    static constexpr bool PERSISTENT = false;
    typedef NoShared Shared;
    W kmask;   // bits 0 .. k - 1
    W flip;    // all ones when penalty_s < penalty_d
    W wmask;   // bits 0 .. window - 1
    int window;
    int ilast; // the last tested window position: max(k - window - 1, 0) (filter.go:202-205; k - window is never tested)
    int need;  // a record is a hit when some tested window has at least this many set bits
    u32 keep_hits;  // UKM_F_INVERT
    __device__ __forceinline__ void setup(Shared &, int) const {}
    __device__ __forceinline__ u32 keep(Shared &, u64 (&x)[VT], const u32 (&)[VT], u32 valid) const {
        W bits[VT];
#pragma unroll
        for (int s = 0; s < VT; s++) {
            // bases are read from the LOW end (filter.go:186,197); bit 2j of m: base j equals base j + 1, where the base
            // above bit 63 reads as 0 (`code >>= 2` in Go)
            const u64 c = x[s];
            const u64 e = ~(c ^ (c >> 2));
            const u64 m = e & (e >> 1) & 0x5555555555555555ull;
            const u32 same = even_bits16((u32)m) | (even_bits16((u32)(m >> 32)) << 16);
            // bit i: scores[i] == penalty_s; scores[0] = penalty_d whatever the base (filter.go:193-195); bases 33 .. 63 of a
            // hashed k > 32 are all "0 after 0"
            W b = (W)((W)same << 1);
            if (sizeof(W) == 8) b |= (W)(~0ull << 33);
            bits[s] = (b ^ flip) & kmask;
        }
        int mx[VT];
#pragma unroll
        for (int s = 0; s < VT; s++) mx[s] = 0;
        if (sizeof(W) == 4 && window < 32) {  // (uniform) one bit-field extract, one popcount, one max per record and position
            for (int i = 0; i <= ilast; i++) {
#pragma unroll
                for (int s = 0; s < VT; s++) {
                    const int pc = __popc(__builtin_amdgcn_ubfe((u32)bits[s], (u32)i, (u32)window));
                    mx[s] = pc > mx[s] ? pc : mx[s];
                }
            }
        } else {
            for (int i = 0; i <= ilast; i++) {
#pragma unroll
                for (int s = 0; s < VT; s++) {
                    const W win = (W)(bits[s] >> i) & wmask;
                    const int pc = sizeof(W) == 8 ? __popcll((u64)win) : __popc((u32)win);
                    mx[s] = pc > mx[s] ? pc : mx[s];
                }
            }
        }
        u32 kept = 0;
#pragma unroll
        for (int s = 0; s < VT; s++) kept |= ((mx[s] >= need ? 1u : 0u) == keep_hits) ? 1u << s : 0u;
        return kept & valid;
    }
};

// kmers.Canonical(code, k): the smaller of the code and its reverse complement
__device__ __forceinline__ u64 canonical_code(u64 code, int k) {
    u64 x = ~code;
    x = ((u64)__builtin_bitreverse32((u32)x) << 32) | (u64)__builtin_bitreverse32((u32)(x >> 32));
    x = ((x & 0xAAAAAAAAAAAAAAAAull) >> 1) | ((x & 0x5555555555555555ull) << 1);
    x >>= 64 - 2 * k;
    return x < code ? x : code;
}

constexpr u32 GREP_LDS_SLOTS = 4096;                // 32 KB
constexpr u64 GREP_LDS_MAX = GREP_LDS_SLOTS / 2;    // queries (counted with their duplicates) the table takes
constexpr u64 GREP_EMPTY = ~0ull;                   // (a query of this value is kept in `has_empty` instead)

struct GrepLdsShared {
    u64 tab[GREP_LDS_SLOTS];
    u32 has_empty;
};
struct GrepLds {
    static constexpr bool PERSISTENT = true;
    typedef GrepLdsShared Shared;
    const u64 *q;
    u32 nq;
    int canonical_k;
    u32 invert;
    static __device__ __forceinline__ u32 slot_of(u64 x) { return (u32)((x * 0x9E3779B97F4A7C15ull) >> 52); }  // 12 bits
    __device__ __forceinline__ void setup(Shared &sh, int tid) const {
        for (u32 i = (u32)tid; i < GREP_LDS_SLOTS; i += NT) sh.tab[i] = GREP_EMPTY;
        if (tid == 0) sh.has_empty = 0;
        __syncthreads();
        for (u32 i = (u32)tid; i < nq; i += NT) {
            const u64 v = q[i];
            if (v == GREP_EMPTY) { sh.has_empty = 1; continue; }
            // at most GREP_LDS_MAX distinct values in GREP_LDS_SLOTS slots: a free slot always turns up
            for (u32 s = slot_of(v);; s = (s + 1) & (GREP_LDS_SLOTS - 1)) {
                const u64 old = atomicCAS((unsigned long long *)&sh.tab[s], (unsigned long long)GREP_EMPTY, (unsigned long long)v);
                if (old == GREP_EMPTY || old == v) break;
            }
        }
        __syncthreads();
    }
    __device__ __forceinline__ u32 keep(Shared &sh, u64 (&x)[VT], const u32 (&)[VT], u32 valid) const {
        u32 hit = 0;
#pragma unroll
        for (int s = 0; s < VT; s++) {
            if (canonical_k) x[s] = canonical_code(x[s], canonical_k);
            const u64 v = x[s];
            bool h = false;
            if (v == GREP_EMPTY) h = sh.has_empty != 0;
            else
                for (u32 j = slot_of(v);; j = (j + 1) & (GREP_LDS_SLOTS - 1)) {
                    const u64 e = sh.tab[j];
                    if (e == v) { h = true; break; }
                    if (e == GREP_EMPTY) break;  // (the table is never full)
                }
            hit |= h ? 1u << s : 0u;
        }
        return (invert ? ~hit : hit) & valid;
    }
};

struct GrepDir {
    static constexpr bool PERSISTENT = false;
    typedef NoShared Shared;
    Dir d;
    int canonical_k;
    u32 invert;
    __device__ __forceinline__ void setup(Shared &, int) const {}
    __device__ __forceinline__ u32 keep(Shared &, u64 (&x)[VT], const u32 (&)[VT], u32 valid) const {
        if (canonical_k) {
#pragma unroll
            for (int s = 0; s < VT; s++) x[s] = canonical_code(x[s], canonical_k);
        }
        u32 lo[VT];
        const u32 hit = dir_search_n<VT>(d, x, valid, lo);
        return (invert ? ~hit : hit) & valid;
    }
};

struct TaxidPred {
    static constexpr bool PERSISTENT = false;
    typedef NoShared Shared;
    const u32 *bits;  // bit t of the bitmap: taxid t is queried, t = 0 .. max_taxid
    u32 max_taxid;
    u32 invert;
    __device__ __forceinline__ void setup(Shared &, int) const {}
    __device__ __forceinline__ u32 keep(Shared &, u64 (&)[VT], const u32 (&t)[VT], u32 valid) const {
        u32 hit = 0;
#pragma unroll
        for (int s = 0; s < VT; s++) {
            const bool in = ((valid >> s) & 1u) && t[s] <= max_taxid;
            const u32 w = in ? bits[t[s] >> 5] : 0u;
            hit |= ((w >> (t[s] & 31u)) & 1u) << s;
        }
        return (invert ? ~hit : hit) & valid;
    }
};

// ---- the selection kernel ---------------------------------------------------------------------------------------------------
template <class PRED, bool TAX, bool TICKET>
__global__ __launch_bounds__(NT) void select_kernel(SelArgs p, PRED pred) {
    __shared__ __attribute__((aligned(16))) u64 s_keys[TILE];
    __shared__ u32 s_tax[TAX ? TILE : 1];
    __shared__ u32 s_scan[NT / 64 + 1];
    __shared__ u64 s_misc[2];
    __shared__ typename PRED::Shared s_pred;
    const int tid = (int)threadIdx.x, lane = lane_id();
    pred.setup(s_pred, tid);
    const bool vec_k = ((uintptr_t)p.k & 15) == 0, vec_t = TAX && ((uintptr_t)p.t & 15) == 0;
    // a persistent workgroup goes on to tile blockIdx + i * gridDim (TICKET: to the next ticket) until the tiles are used up
    for (u64 it = 0;; it++) {
        const u64 tile = TICKET ? lb_tile_id<true>(p.ticket, &s_misc[0]) : (u64)blockIdx.x + it * (u64)gridDim.x;
        if (tile >= p.ntiles) break;
        const u64 i0 = tile * (u64)TILE + (u64)tid * VT;
        u64 x[VT];
        u32 t[VT];
        u32 valid = 0;
        if (i0 + VT <= p.n) {
            valid = (1u << VT) - 1;
            if (vec_k) {
#pragma unroll
                for (int s = 0; s < VT; s += 2) {
                    const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(p.k + i0 + s);
                    x[s] = v.x; x[s + 1] = v.y;
                }
            } else {
#pragma unroll
                for (int s = 0; s < VT; s++) x[s] = p.k[i0 + s];
            }
            if (TAX) {
                if (vec_t) {
#pragma unroll
                    for (int s = 0; s < VT; s += 4) {
                        const uint4 v = *reinterpret_cast<const uint4 *>(p.t + i0 + s);
                        t[s] = v.x; t[s + 1] = v.y; t[s + 2] = v.z; t[s + 3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int s = 0; s < VT; s++) t[s] = p.t[i0 + s];
                }
            }
        } else {
#pragma unroll
            for (int s = 0; s < VT; s++) {
                const bool in = i0 + s < p.n;
                x[s] = in ? p.k[i0 + s] : 0;
                if (TAX) t[s] = in ? p.t[i0 + s] : 0u;
                valid |= in ? 1u << s : 0u;
            }
        }
        if (!TAX) {
#pragma unroll
            for (int s = 0; s < VT; s++) t[s] = 0;
        }
        const u32 kept = pred.keep(s_pred, x, t, valid);
        u32 tot;
        const u32 excl = block_excl_scan_u32<NT>((u32)__popc(kept), s_scan, &tot);
        const u64 base = lb_tile_base<TICKET>(p.status, tile, (u64)tot, &p.result[1], SEL_FLAG_TIMEOUT, &s_misc[1], tid, lane);
        // the survivors side by side in LDS, then out in one piece
        u32 pos = excl;
#pragma unroll
        for (int s = 0; s < VT; s++)
            if ((kept >> s) & 1u) {
                s_keys[pos] = x[s];
                if (TAX) s_tax[pos] = t[s];
                pos++;
            }
        __syncthreads();
        if (base + tot <= p.out_cap) {
            u64 *o = p.out + base;
            const int sh = (int)(((uintptr_t)o >> 3) & 1);  // 16-byte stores on the aligned middle
            const int npairs = ((int)tot + sh + 1) >> 1;
            for (int m = tid; m < npairs; m += NT) {
                const int j0 = 2 * m - sh, j1 = j0 + 1;
                const bool v0 = j0 >= 0, v1 = j1 < (int)tot;
                const u64 k0 = s_keys[v0 ? j0 : 0], k1 = s_keys[v1 ? j1 : 0];
                if (v0 && v1) *reinterpret_cast<ulonglong2 *>(o + j0) = make_ulonglong2(k0, k1);
                else if (v0) o[j0] = k0;
                else if (v1) o[j1] = k1;
            }
            if (TAX) {
                u32 *to = p.tout + base;
                for (u32 i = (u32)tid; i < tot; i += NT) to[i] = s_tax[i];
            }
        } else {  // too small an output: what fits is written, the count goes on
            for (u32 i = (u32)tid; i < tot; i += NT) {
                const u64 w = base + i;
                if (w < p.out_cap) {
                    p.out[w] = s_keys[i];
                    if (TAX) p.tout[w] = s_tax[i];
                }
            }
        }
        if (tid == 0 && tile == p.ntiles - 1) p.result[0] = base + tot;
        if (!PRED::PERSISTENT) break;
        __syncthreads();  // (s_keys / s_misc are the next tile's)
    }
}

// ukm_sample: out[j] = record first + j * step
__global__ void sample_kernel(const u64 *k, const u32 *t, u64 first, u64 step, u64 m, u64 *out, u32 *tout) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
        const u64 i = first + j * step;
        out[j] = k[i];
        if (t) tout[j] = t[i];
    }
}

// ---- taxid bitmap -----------------------------------------------------------------------------------------------------------
__global__ void taxid_max_kernel(const u32 *q, u64 nq, u32 *mx) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    u32 m = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += stride) m = q[i] > m ? q[i] : m;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u32 o = (u32)__shfl_xor((int)m, d, 64);
        m = o > m ? o : m;
    }
    if (lane_id() == 0) atomicMax(mx, m);
}
__global__ void taxid_bitmap_kernel(const u32 *q, u64 nq, u32 *bits) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += stride) atomicOr(&bits[q[i] >> 5], 1u << (q[i] & 31u));
}

// ---- host steps -------------------------------------------------------------------------------------------------------------
unsigned blocks_for(const ukm_ctx *c, u64 n) { return (unsigned)std::max<u64>(1, std::min<u64>((n + NT - 1) / NT, (u64)c->num_cu * 16)); }

template <class PRED, bool TAX, bool TICKET>
int launch_one(ukm_ctx *c, const SelArgs &p, const PRED &pred) {
    u64 grid = p.ntiles;
    if (PRED::PERSISTENT) {
        // without tickets the look-back of a persistent kernel is live only while every workgroup of the grid is resident
        int per_cu = 0;
        UKM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, select_kernel<PRED, TAX, TICKET>, NT, 0));
        grid = std::min<u64>(p.ntiles, (u64)std::max(per_cu, 1) * (u64)c->num_cu);
    }
    hipLaunchKernelGGL((select_kernel<PRED, TAX, TICKET>), dim3((unsigned)grid), dim3(NT), 0, c->stream, p, pred);
    return UKM_OK;
}

// all pointers are device pointers; n >= 1
template <class PRED>
int run_select(ukm_ctx *c, const char *name, const PRED &pred, const u64 *k, const u32 *t, u64 n, u64 *out, u32 *tout, u64 out_cap,
               u64 *n_out) {
    SelArgs p;
    memset(&p, 0, sizeof(p));
    p.k = k; p.t = t; p.n = n; p.out = out; p.tout = tout; p.out_cap = out_cap;
    p.ntiles = (n + TILE - 1) / TILE;
    if (p.ntiles > 0xFFFFFFFFull) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu records in one call; split them over several calls", name, (unsigned long long)n);
    LbCtl blk;
    UKM_TRY(ukm_lb_ctl_alloc(c, p.ntiles, 0, &blk));
    p.status = blk.status; p.ticket = blk.ticket; p.result = blk.result;
    u64 res[2] = {0, 0};
    const LbLaunch how = {name, "selection kernel", SEL_FLAG_TIMEOUT, true, false, false};
    UKM_TRY(ukm_lb_launch(c, blk, how, [&](bool ticket) {
        if (t) return ticket ? launch_one<PRED, true, true>(c, p, pred) : launch_one<PRED, true, false>(c, p, pred);
        return ticket ? launch_one<PRED, false, true>(c, p, pred) : launch_one<PRED, false, false>(c, p, pred);
    }, res));
    *n_out = res[0];
    if (res[0] > out_cap)
        UKM_FAIL(UKM_ERR_CAPACITY, "%s: output needs %llu records, capacity is %llu", name, (unsigned long long)res[0], (unsigned long long)out_cap);
    return UKM_OK;
}

// every record kept as it is
int copy_all(ukm_ctx *c, const char *name, const u64 *k, const u32 *t, u64 n, u64 *out, u32 *tout, u64 out_cap, u64 *n_out) {
    *n_out = n;
    if (n > out_cap) UKM_FAIL(UKM_ERR_CAPACITY, "%s: output needs %llu records, capacity is %llu", name, (unsigned long long)n, (unsigned long long)out_cap);
    UKM_HIP(hipMemcpyAsync(out, k, n * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
    if (t) UKM_HIP(hipMemcpyAsync(tout, t, n * sizeof(u32), hipMemcpyDeviceToDevice, c->stream));
    return UKM_OK;
}

// Which shape answers a code query: the LDS table while the queries fit it, option "grep_lds" 0 never /
// 1 whenever they fit.
bool lds_route(const ukm_ctx *c, u64 nq) {
    if (nq > GREP_LDS_MAX) return false;
    const char *e = ukm_env(c, "UKM_GREP_LDS");
    if (e && *e) return e[0] != '0';
    return true;
}

int grep_codes(ukm_ctx *c, const char *name, const u64 *k, const u32 *t, u64 n, int canonical_k, const u64 *q, u64 nq, bool invert,
               u64 *out, u32 *tout, u64 out_cap, u64 *n_out) {
    if (nq == 0 && !invert) return UKM_OK;
    if (nq == 0 || lds_route(c, nq)) {  // (no queries, inverted: every record, through the kernel for canonical_k)
        c->stat_grep_route = 1;
        GrepLds pred;
        pred.q = q; pred.nq = (u32)nq; pred.canonical_k = canonical_k; pred.invert = invert ? 1u : 0u;
        return run_select(c, name, pred, k, t, n, out, tout, out_cap, n_out);
    }
    // the queries, sorted and distinct (all 64 bits: they are the caller's)
    u64 *qs = nullptr, *qd = nullptr;
    UKM_TRY(ws_alloc_t(c, nq, &qs));
    UKM_TRY(ws_alloc_t(c, nq, &qd));
    UKM_HIP(hipMemcpyAsync(qs, q, nq * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
    UKM_TRY(ukm_dev_sort(c, qs, nullptr, nq, 64));
    u64 nd = 0;
    UKM_TRY(ukm_dev_unique(c, qs, nullptr, nq, UKM_UNIQUE, qd, nullptr, nq, &nd));
    if (nd >= (1ull << 32)) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu distinct queries; the limit is 2^32 - 1", name, (unsigned long long)nd);
    // the directory spans the bits the largest query has: codes of k bases use 2k of the 64
    u64 qmax = 0;
    UKM_TRY(ukm_read_u64(c, qd + nd - 1, &qmax));
    int key_bits = 1;
    while (key_bits < 64 && (qmax >> key_bits) != 0) key_bits++;
    c->stat_grep_route = 2;
    GrepDir pred;
    UKM_TRY(build_dir(c, qd, nd, key_bits, DIR_SLACK_DEFAULT, &pred.d));
    pred.canonical_k = canonical_k; pred.invert = invert ? 1u : 0u;
    return run_select(c, name, pred, k, t, n, out, tout, out_cap, n_out);
}

int grep_taxids(ukm_ctx *c, const char *name, const u64 *k, const u32 *t, u32 file_taxid, u64 n, const u32 *q, u64 nq, bool invert,
                u64 *out, u32 *tout, u64 out_cap, u64 *n_out) {
    if (nq == 0) return invert ? copy_all(c, name, k, t, n, out, tout, out_cap, n_out) : UKM_OK;
    u64 *mx = nullptr;
    UKM_TRY(ws_alloc_t(c, 1, &mx));
    UKM_HIP(hipMemsetAsync(mx, 0, sizeof(u64), c->stream));
    hipLaunchKernelGGL(taxid_max_kernel, dim3(blocks_for(c, nq)), dim3(NT), 0, c->stream, q, nq, (u32 *)mx);
    UKM_HIP(hipGetLastError());
    u64 mxh = 0;
    UKM_TRY(ukm_read_u64(c, mx, &mxh));
    const u32 max_taxid = (u32)mxh;
    const size_t words = (size_t)(max_taxid >> 5) + 1;
    u32 *bits = nullptr;
    UKM_TRY(ws_alloc_t(c, (words + 1) & ~(size_t)1, &bits));
    UKM_HIP(hipMemsetAsync(bits, 0, ((words + 1) & ~(size_t)1) * sizeof(u32), c->stream));
    hipLaunchKernelGGL(taxid_bitmap_kernel, dim3(blocks_for(c, nq)), dim3(NT), 0, c->stream, q, nq, bits);
    UKM_HIP(hipGetLastError());
    if (!t) {
        // one taxid for the whole file (what ReadCodeWithTaxid hands out with every record): all or nothing
        bool hit = false;
        if (file_taxid <= max_taxid) {
            u64 w = 0;
            UKM_TRY(ukm_read_u64(c, (const u64 *)bits + (file_taxid >> 6), &w));
            hit = ((w >> (file_taxid & 63u)) & 1ull) != 0;
        }
        return hit != invert ? copy_all(c, name, k, nullptr, n, out, nullptr, out_cap, n_out) : UKM_OK;
    }
    c->stat_grep_route = 3;
    TaxidPred pred;
    pred.bits = bits; pred.max_taxid = max_taxid; pred.invert = invert ? 1u : 0u;
    return run_select(c, name, pred, k, t, n, out, tout, out_cap, n_out);
}

// the rank filter: a record's fate depends on its taxid alone -- one pass over the taxonomy writes a keep bit per taxid
// (ukm_tax.hip), and the selection is grep by taxid over that bitmap
int rfilter_taxids(ukm_ctx *c, const char *name, const u64 *k, const u32 *t, u32 file_taxid, u64 n, const ukm_rank_filter *f, u64 *out,
                   u32 *tout, u64 out_cap, u64 *n_out) {
    u32 *bits = nullptr;
    UKM_TRY(ukm_dev_rank_bitmap(c, name, f, &bits));
    const u32 max_taxid = c->tax_size - 1;
    if (!t) {
        bool hit = false;
        if (file_taxid <= max_taxid) {
            u64 w = 0;
            UKM_TRY(ukm_read_u64(c, (const u64 *)bits + (file_taxid >> 6), &w));
            hit = ((w >> (file_taxid & 63u)) & 1ull) != 0;
        }
        return hit ? copy_all(c, name, k, nullptr, n, out, nullptr, out_cap, n_out) : UKM_OK;
    }
    TaxidPred pred;
    pred.bits = bits; pred.max_taxid = max_taxid; pred.invert = 0u;
    return run_select(c, name, pred, k, t, n, out, tout, out_cap, n_out);
}

int filter_codes(ukm_ctx *c, const char *name, const u64 *k, const u32 *t, u64 n, int kk, int window, int ps, int pd, int threshold,
                 bool invert, u64 *out, u32 *tout, u64 out_cap, u64 *n_out) {
    if (window > kk) window = kk;  // filter.go:116-119
    // sum of a window = window * penalty_d + (penalty_s - penalty_d) * (bases equal to their predecessor); with
    // penalty_s < penalty_d the other kind of base is counted
    const long long d = (long long)ps - (long long)pd;
    const long long unit = d >= 0 ? d : -d, floor_sum = (long long)window * (d >= 0 ? pd : ps);
    long long need;
    if (unit == 0) need = floor_sum >= threshold ? 0 : (long long)window + 1;
    else {
        const long long a = (long long)threshold - floor_sum;
        need = a > 0 ? (a + unit - 1) / unit : 0;
        if (need > window) need = (long long)window + 1;
    }
    const int ilast = std::max(kk - window - 1, 0);
    const u64 kmask = kk == 64 ? ~0ull : ((1ull << kk) - 1), wmask = window == 64 ? ~0ull : ((1ull << window) - 1);
    if (kk <= 32) {
        FilterPred<u32> pred;
        pred.kmask = (u32)kmask; pred.flip = d < 0 ? ~0u : 0u; pred.wmask = (u32)wmask; pred.window = window; pred.ilast = ilast; pred.need = (int)need;
        pred.keep_hits = invert ? 1u : 0u;
        return run_select(c, name, pred, k, t, n, out, tout, out_cap, n_out);
    }
    FilterPred<u64> pred;
    pred.kmask = kmask; pred.flip = d < 0 ? ~0ull : 0ull; pred.wmask = wmask; pred.window = window; pred.ilast = ilast; pred.need = (int)need;
    pred.keep_hits = invert ? 1u : 0u;
    return run_select(c, name, pred, k, t, n, out, tout, out_cap, n_out);
}

int check_common(const char *name, const void *ctx, const void *n_out, const void *keys, const void *taxids, u64 n, const void *out_keys,
                 const void *out_taxids, u64 out_cap) {
    if (!ctx || !n_out || (!keys && n) || (!out_keys && out_cap)) UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
    if (taxids && !out_taxids && out_cap) UKM_FAIL(UKM_ERR_INVALID, "%s: taxids given but out_taxids is NULL", name);
    return UKM_OK;
}

// what the three entry points share: the call bracket and the staging of the record arrays around `body`
template <class F>
int select_entry(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint64_t n, uint64_t *out_keys, uint32_t *out_taxids,
                 uint64_t out_cap, uint64_t *n_out, F body) {
    *n_out = 0;
    if (n == 0) return UKM_OK;
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        const u64 *k = nullptr;
        const u32 *t = nullptr;
        u64 *out = nullptr;
        u32 *tout = nullptr;
        UKM_TRY(ukm_in_t(ctx, keys, n, &k));
        UKM_TRY(ukm_in_t(ctx, taxids, n, &t));
        UKM_TRY(ukm_out_t(ctx, out_keys, out_cap, &out));
        if (taxids) UKM_TRY(ukm_out_t(ctx, out_taxids, out_cap, &tout));
        const int r = body(k, t, out, tout);
        const u64 m = (r == UKM_OK) ? *n_out : 0;
        ukm_out_resize(ctx, out_keys, m * sizeof(u64));
        if (taxids && out_taxids) ukm_out_resize(ctx, out_taxids, m * sizeof(u32));
        return r;
    }();
    return ukm_finish(&s, rc);
}

}  // namespace

extern "C" int ukm_grep(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint32_t file_taxid, uint64_t n, int canonical_k,
                        const uint64_t *q_keys, const uint32_t *q_taxids, uint64_t nq, uint32_t flags, uint64_t *out_keys,
                        uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out) {
    const char *name = "ukm_grep";
    UKM_TRY(check_common(name, ctx, n_out, keys, taxids, n, out_keys, out_taxids, out_cap));
    if (q_keys && q_taxids) UKM_FAIL(UKM_ERR_INVALID, "%s: q_keys and q_taxids are both given; a query is one or the other", name);
    if (nq && !q_keys && !q_taxids) UKM_FAIL(UKM_ERR_INVALID, "%s: neither q_keys nor q_taxids is given", name);
    if (canonical_k < 0 || canonical_k > 32) UKM_FAIL(UKM_ERR_K, "%s: canonical_k = %d out of range (0, or 1..32)", name, canonical_k);
    if (nq >= (1ull << 32)) UKM_FAIL(UKM_ERR_INVALID, "%s: %llu queries; the limit is 2^32 - 1", name, (unsigned long long)nq);
    const bool invert = (flags & UKM_F_INVERT) != 0, by_taxid = q_taxids != nullptr || (!q_keys && (flags & UKM_F_QUERY_TAXID));
    if (ctx) ctx->stat_grep_route = 0;
    return select_entry(ctx, keys, taxids, n, out_keys, out_taxids, out_cap, n_out, [&](const u64 *k, const u32 *t, u64 *out, u32 *tout) -> int {
        if (by_taxid) {
            const u32 *q = nullptr;
            UKM_TRY(ukm_in_t(ctx, q_taxids, nq, &q));
            return grep_taxids(ctx, name, k, t, file_taxid, n, q, nq, invert, out, tout, out_cap, n_out);
        }
        const u64 *q = nullptr;
        UKM_TRY(ukm_in_t(ctx, q_keys, nq, &q));
        return grep_codes(ctx, name, k, t, n, canonical_k, q, nq, invert, out, tout, out_cap, n_out);
    });
}

extern "C" int ukm_filter(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint64_t n, int k, int window, int penalty_s,
                          int penalty_d, int threshold, uint32_t flags, uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap,
                          uint64_t *n_out) {
    const char *name = "ukm_filter";
    UKM_TRY(check_common(name, ctx, n_out, keys, taxids, n, out_keys, out_taxids, out_cap));
    if (k < 1 || k > 64) UKM_FAIL(UKM_ERR_K, "%s: k = %d out of range (1..64)", name, k);
    if (window < 1) UKM_FAIL(UKM_ERR_INVALID, "%s: window must be at least 1", name);
    if (threshold < 0) UKM_FAIL(UKM_ERR_INVALID, "%s: threshold must not be negative", name);
    return select_entry(ctx, keys, taxids, n, out_keys, out_taxids, out_cap, n_out, [&](const u64 *kd, const u32 *t, u64 *out, u32 *tout) -> int {
        return filter_codes(ctx, name, kd, t, n, k, window, penalty_s, penalty_d, threshold, (flags & UKM_F_INVERT) != 0, out, tout, out_cap, n_out);
    });
}

extern "C" int ukm_sample(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint64_t n, uint64_t start, uint64_t window,
                          uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out) {
    const char *name = "ukm_sample";
    UKM_TRY(check_common(name, ctx, n_out, keys, taxids, n, out_keys, out_taxids, out_cap));
    if (start < 1 || window < 1) UKM_FAIL(UKM_ERR_INVALID, "%s: start and window must be at least 1", name);
    // record j (1-based) with j >= start and (j - start) % window == 0
    const u64 m = n >= start ? (n - start) / window + 1 : 0;
    *n_out = m;
    if (m > out_cap) UKM_FAIL(UKM_ERR_CAPACITY, "%s: output needs %llu records, capacity is %llu", name, (unsigned long long)m, (unsigned long long)out_cap);
    if (m == 0) return UKM_OK;
    return select_entry(ctx, keys, taxids, n, out_keys, out_taxids, out_cap, n_out, [&](const u64 *k, const u32 *t, u64 *out, u32 *tout) -> int {
        hipLaunchKernelGGL(sample_kernel, dim3(blocks_for(ctx, m)), dim3(NT), 0, ctx->stream, k, t, start - 1, window, m, out, tout);
        UKM_HIP(hipGetLastError());
        *n_out = m;
        return UKM_OK;
    });
}

extern "C" int ukm_rfilter(ukm_ctx *ctx, const uint64_t *keys, const uint32_t *taxids, uint32_t file_taxid, uint64_t n,
                           const ukm_rank_filter *f, uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap, uint64_t *n_out) {
    const char *name = "ukm_rfilter";
    UKM_TRY(check_common(name, ctx, n_out, keys, taxids, n, out_keys, out_taxids, out_cap));
    if (!f) UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
    *n_out = 0;
    if (!ctx->tax_parent || !ctx->tax_rank) UKM_FAIL(UKM_ERR_NO_TAXONOMY, "%s: no taxonomy with ranks loaded (ukm_taxonomy_set_ranks)", name);
    {
        uint8_t sa[256], wa[256];
        UKM_TRY(ukm_rank_filter_plan(f, sa, wa));
    }
    return select_entry(ctx, keys, taxids, n, out_keys, out_taxids, out_cap, n_out, [&](const u64 *k, const u32 *t, u64 *out, u32 *tout) -> int {
        return rfilter_taxids(ctx, name, k, t, file_taxid, n, f, out, tout, out_cap, n_out);
    });
}
