// ukm_encode.hip — sequence -> uint64 window values on the GPU:
//   * 2-bit k-mer codes with optional canonicalisation: replaces
//     sketches.NewKmerIterator(...).NextKmer() (count.go:321,363) = shenwei356/kmers v0.1.0
//     (A=0 C=1 G=2 T/U=3, first base most significant, canonical = min(code, revcomp));
//   * ntHash v1 (will-rowe/nthash v0.4.0): replaces sketches.NewHashIterator(...).NextHash()
//     (count.go:319,361) / nthash.Hasher.Next (dump.go:253-260), fused with the Scaled-MinHash
//     filter `code > maxHash -> skip` (count.go:98,373-375).
//
// Kernel shape (both value kinds): one 256-thread workgroup per tile of WT = 2048 window start
// positions of the concatenated records (+64 bases of overlap), staged once in LDS.
//   phase 1 (blocked over positions): record lookup -> per-position info byte (bases left in
//            the record, "record long enough" bit) and record index; the per-position
//            ingredients of the value:
//              codes : 2-bit packed tile + illegal-base bit mask (16 bases per 32-bit word)
//              ntHash: XOR-prefix sums  P[n] = xor_{m<n} ror(seed[s_m], m),
//                                       Q[n] = xor_{m<n} rol(cseed[s_m], m)   (block XOR scan)
//   phase 2 (striped over windows, so stores are coalesced): window i is computed in O(1),
//            with no rolling dependency and no k-1 warm-up:
//              code(i)  = 2k-bit field at bit 2i of the packed tile; revcomp by bit reversal
//              fwd(i)   = rol(P[i+k] ^ P[i], i+k-1),  rev(i) = ror(Q[i+k] ^ Q[i], i)
//            (the first version rolled 16 windows per thread: (16+k-1)/16 = 4x redundant work
//            at k = 51 and 128-byte-strided stores; ntHash ran at 3.5e10 bases/s).
//   Scaled filter: survivors are compacted in window order with one wave64 ballot per round, a
//   per-tile prefix and the library's decoupled look-back.
// Windows that wrap (circular genomes) are recomputed directly from the record.
// Algorithmic bytes: 1 B/base read, 8 B/window written (8/scale with the Scaled filter).
//
// This file holds the unit's build knobs and table sizes (one block, below) and the host side: the policies that choose a
// kernel, the launches, run_windows / run_minimizer and the C entries.  The device code is in three headers that only this file includes, inside its anonymous namespace:
//   ukm_win_common.h     tile constants, base / seed tables, ENC_FLAG_*, small device helpers, tile_place_kept,
//                        window_count_kernel, tile_first_rec_kernel
//   ukm_win_kernels.h    window_kernel, nthash_strip_kernel, stripwin_kernel, each with its argument struct
//   ukm_win_minimizer.h  minimizer_kernel
#include <stdlib.h>

#include <algorithm>

#include "ukm_device.h"
#include "ukm_map.h"

namespace {

// ---- the unit's build knobs (-D) and the fixed sizes of its tiles and LDS tables, in one place -------------------------------
// What the headers below are compiled with.  tests/test_gpu_window_limits.py reads these lines and places its inputs on both
// sides of every table size; the kernel that owns a size says what happens beyond it.
#ifndef ENC_NT
#define ENC_NT 512
#endif
#ifndef ENC_WT
#define ENC_WT 2048
#endif
constexpr int ST_NT = 256;    // nthash_strip_kernel: lanes per tile
#ifndef ST_CAP_N
#define ST_CAP_N 1024
#endif
constexpr int ST_CAP = ST_CAP_N;  // nthash_strip_kernel: candidate list entries per tile
constexpr int SW_NT = 256;    // stripwin_kernel: lanes per tile
constexpr int SW_REC = 254;   // stripwin_kernel: records one tile may touch
#ifndef SW_ABL
#define SW_ABL 0              // developer ablations: 1 = no row stores
#endif
#ifndef MIN_MT
#define MIN_MT 2048  /* 1024 / 2048 / 4096: 1.24 / 1.01 / 1.19 ms per 1e8 windows incl. the ntHash pass (w = 15) */
#endif
constexpr int MW_MAX = 1024;  // minimizer_kernel: largest supported w (LDS halo)
constexpr int M_REC = 256;    // minimizer_kernel: records of a tile kept in LDS

#include "ukm_win_common.h"
#include "ukm_win_kernels.h"
#include "ukm_win_minimizer.h"

// the kernel that wrote the windows of a call: the values of the statistic "window_route" (ukm_internal.h)
enum WindowRoute : u64 { ROUTE_NO_LAUNCH = 0, ROUTE_WINDOW = 1, ROUTE_STRIPWIN = 2, ROUTE_NTHASH_STRIP = 3 };

// ---- host steps the launches below share ------------------------------------------------------------------------
// tile_rec[ntiles + 3] from the arena, filled by tile_first_rec_kernel for tiles of tile_size positions
int first_rec_of_tiles(ukm_ctx *c, const u64 *rec_off, u64 n_rec, u64 total, u64 ntiles, u64 tile_size, const u64 **tile_rec) {
    u64 *tr = nullptr;
    UKM_TRY(ws_alloc_t(c, ntiles + 3, &tr));
    hipLaunchKernelGGL(tile_first_rec_kernel, dim3((unsigned)((ntiles + 3 + 255) / 256)), dim3(256), 0, c->stream, rec_off,
                       n_rec, total, ntiles, tile_size, tr);
    *tile_rec = tr;
    return UKM_OK;
}
int check_capacity(u64 n, u64 out_cap) {
    if (n > out_cap)
        UKM_FAIL(UKM_ERR_CAPACITY, "output needs %llu values, capacity is %llu", (unsigned long long)n,
                 (unsigned long long)out_cap);
    return UKM_OK;
}
int check_legal(const u64 res[2]) {
    if (res[1] & ENC_FLAG_ILLEGAL) UKM_FAIL(UKM_ERR_ILLEGAL_BASE, "illegal base in sequence (kmers.ErrIllegalBase)");
    return UKM_OK;
}
// the control block's words in the argument struct of a kernel that compacts with the look-back
template <typename Args>
void bind_ctl(Args &p, const LbCtl &blk) {
    p.result = blk.result; p.ticket = blk.ticket; p.status = blk.status;
}
// one workgroup of nt threads per tile, of the kernel's <TICKET = false> or <TICKET = true> instantiation
template <typename Args>
int launch_tiles(void (*blockidx_form)(Args), void (*ticket_form)(Args), bool ticket, u64 ntiles, int nt, hipStream_t st, const Args &p) {
    hipLaunchKernelGGL(ticket ? ticket_form : blockidx_form, dim3((unsigned)ntiles), dim3(nt), 0, st, p);
    return UKM_OK;
}
u64 tiles_of(u64 total_bases, int nt, int L) { return (total_bases + (u64)nt * (u64)L - 1) / ((u64)nt * (u64)L); }

// ---- Scaled-MinHash sketch: nthash_strip_kernel ------------------------------------------------------------------
// policy: the strip length L, or 0 when the strip kernel does not apply and the general kernel runs
int strip_filter_L(const ukm_ctx *c, const u8 *bases, int canonical, u64 max_hash, u64 total_bases) {
    // developer / test knob: UKM_NTHASH_STRIP=0 never, =1 always (whatever the scale; overflow still falls back)
    const char *fe = ukm_env(c, "UKM_NTHASH_STRIP");
    const int force = fe ? atoi(fe) : -1;
    if (force == 0) return 0;
    if (((uintptr_t)bases & 3) != 0) return 0;
    // expected candidates per tile = NT * L * (max_hash / 2^64), twice that when canonical (min(f, r) <= m iff
    // f <= m or r <= m); keep it below 0.6 of the list
    const double frac = ((double)max_hash + 1.0) / 18446744073709551616.0 * (canonical ? 2.0 : 1.0);
    int L = 1024;
    // enough tiles to fill the chip
    while (L > 256 && total_bases / ((u64)ST_NT * (u64)L) < 2048) L >>= 1;
    // (the count is Poisson: 0.6 x capacity leaves more than ten standard deviations of head room)
    while (L > 64 && (double)ST_NT * L * frac > ST_CAP * 0.6) L >>= 1;
    if (force != 1 && ((double)ST_NT * L * frac > ST_CAP * 0.6 || L < 256)) return 0;  // small --scale: general kernel
    if (const char *le = ukm_env(c, "UKM_STRIP_L")) L = std::min(1024, std::max(64, atoi(le) / 64 * 64));  // developer knob; s_ci packs the window index into 11 bits
    if (tiles_of(total_bases, ST_NT, L) > 0x7FFFFFFFull) return 0;
    return L;
}

// *done = false (with UKM_OK): a tile's candidate list overflowed, the caller runs the general kernel
int launch_strip_filter(ukm_ctx *c, int L, const u8 *bases, const u64 *rec_off, u64 n_rec, int k, int canonical, u64 max_hash,
                        u64 *out, u64 out_cap, u64 *n_out, u64 total_bases, bool *done) {
    *done = false;
    const u64 ntiles = tiles_of(total_bases, ST_NT, L);
    LbCtl blk;
    UKM_TRY(ukm_lb_ctl_alloc(c, ntiles, 0, &blk));
    StripArgs p;
    memset(&p, 0, sizeof(p));
    p.bases = bases; p.rec_off = rec_off; p.n_rec = n_rec; p.total_bases = total_bases; p.k = k;
    p.canonical = canonical; p.L = L; p.max_hash = max_hash; p.out = out; p.out_cap = out_cap; p.ntiles = ntiles;
    bind_ctl(p, blk);
    UKM_TRY(first_rec_of_tiles(c, rec_off, n_rec, total_bases, ntiles, (u64)ST_NT * (u64)L, &p.tile_rec));
    u64 res[2] = {0, 0};
    const LbLaunch how = {"ntHash strip kernel", "ntHash strip kernel", ENC_FLAG_TIMEOUT, true, false, false};
    UKM_TRY(ukm_lb_launch(c, blk, how, [&](bool ticket) {
        return launch_tiles(nthash_strip_kernel<false>, nthash_strip_kernel<true>, ticket, ntiles, ST_NT, c->stream, p);
    }, res));
    if (res[1] & ENC_FLAG_OVERFLOW) {  // candidate list overflow: general kernel
        c->stat_window_strip_declined++;
        return UKM_OK;
    }
    c->stat_window_route = ROUTE_NTHASH_STRIP;
    *n_out = res[0];
    UKM_TRY(check_capacity(*n_out, out_cap));
    *done = true;
    return UKM_OK;
}

// ---- every window of long records: stripwin_kernel -----------------------------------------------------------------
// policy: the strip length L, or 0 when the strip kernel does not apply (short records, tiny input) and window_kernel runs
int strip_windows_L(const ukm_ctx *c, bool hash, const u8 *bases, u64 n_rec, int k, u64 total_bases) {
    const char *fe = ukm_env(c, "UKM_WIN_STRIP");  // developer / test knob: 0 never, 1 whenever it is correct
    const int force = fe ? atoi(fe) : -1;
    if (force == 0) return 0;
    if (((uintptr_t)bases & 3) != 0 || (!hash && k > 32)) return 0;
    // small inputs have too few strips to fill the chip (measured cross-over: 8e6 bases for L = 64, 1.6e7 for L = 128;
    // 1.6e7 bases: codes 0.042 ms against 0.060 ms for the general kernel)
    const u64 min_bases = (k <= 32) ? (1ull << 23) : (1ull << 24);
    // Records: the kernel also wins on short ones — 1e8 bases of 150-bp reads: codes 0.20 ms against 0.43 ms for the
    // general kernel, ntHash k = 51 0.25 against 0.51 ms (0.29 / 0.32 ms with value-by-value boundary rows, 0.264 /
    // 0.285 ms with one strip shift per tile, round 3) — as long as a tile's records fit its table (254 per 256 x L
    // positions, else the call falls back after one wasted launch): average length >= 80 bases for L = 64, >= 140
    // for L = 128.
    const u64 min_avg = (k <= 32) ? 80 : 140;
    if (force != 1 && (total_bases < min_bases || n_rec * min_avg > total_bases)) return 0;
    // several rounds of workgroups per CU matter more than the k - 1 warm-up steps per strip (measured at 1e8
    // bases, codes: L = 64 / 128 / 256 / 512 -> 0.178 / 0.185 / 0.21 / 0.22 ms; ntHash k = 51: 0.242 / 0.230 / 0.244)
    // (1e9 bases: codes 1.71 / 1.84 / 1.94 ms, ntHash k = 51 2.23 / 1.89 / 1.96 ms: short strips keep a wave's 64 output
    // rows close together in memory, which is worth more than the shorter warm-up of long ones)
    int L = (k <= 32) ? 64 : 128;  // twice the warm-up
    if (const char *le = ukm_env(c, "UKM_WIN_STRIP_L")) L = std::max(64, atoi(le) / 64 * 64);
    if (tiles_of(total_bases, SW_NT, L) > 0x7FFFFFFFull) return 0;
    return L;
}

// The sort's first histogram, counted by the kernel that writes the windows (ukm_count).  hist = 256 zeroed device words,
// key_bits = the width the values will be sorted by.  After run_windows shift >= 0 says that the histogram of digit
// (value >> shift) & 255 of ALL values written is in hist (the strip kernel ran with it: SwArgs); -1: nobody counted, the
// sort runs its own pre-pass.
struct FusedHist { u64 *hist; int key_bits; int shift; };

// *done = false (with UKM_OK): a tile touches more records than its table holds, the caller runs window_kernel.  `blk` is
// the caller's control block (no look-back here: its two result words).  fused (may be null): the launch counts into it when
// it can, sets fused->shift when it answered and zeroes the partial count when it gave up.
int launch_strip_windows(ukm_ctx *c, int L, bool hash, const u8 *bases, const u64 *rec_off, const u64 *out_off, u64 n_rec, int k,
                         int canonical, u64 *out, u64 total_bases, u64 total_windows, const LbCtl &blk, bool *done, FusedHist *fused) {
    *done = false;
    const u64 tile_pos = (u64)SW_NT * (u64)L;
    const u64 ntiles = tiles_of(total_bases, SW_NT, L);
    SwArgs p;
    memset(&p, 0, sizeof(p));
    p.bases = bases; p.rec_off = rec_off; p.out_off = out_off; p.n_rec = n_rec; p.total_bases = total_bases;
    p.k = k; p.canonical = canonical; p.L = L; p.out = out; p.result = blk.result;
    UKM_TRY(first_rec_of_tiles(c, rec_off, n_rec, total_bases, ntiles, tile_pos, &p.tile_rec));
    // (k <= 16 writes the rows a record cuts value by value, without the count; 16-bit counters: a tile of <= 65,535 positions)
    const int fsh = (fused && fused->hist && k >= 17 && tile_pos <= 65535) ? ukm_sort_first_shift(c, total_windows, fused->key_bits) : -1;
    if (fsh >= 0) { p.fhist = fused->hist; p.fshift = fsh; }
    u64 res[2] = {0, 0};
    const LbLaunch how = {"strip window kernel", "strip window kernel", 0, true, false, false};  // (no look-back: one attempt)
    UKM_TRY(ukm_lb_launch(c, blk, how, [&](bool) {
        if (hash) hipLaunchKernelGGL(stripwin_kernel<true>, dim3((unsigned)ntiles), dim3(SW_NT), 0, c->stream, p);
        else hipLaunchKernelGGL(stripwin_kernel<false>, dim3((unsigned)ntiles), dim3(SW_NT), 0, c->stream, p);
        return UKM_OK;
    }, res));
    if (res[1] & ENC_FLAG_OVERFLOW) {  // a tile with more records than the table holds: general kernel
        c->stat_window_strip_declined++;
        if (p.fhist) UKM_HIP(hipMemsetAsync(fused->hist, 0, 256 * sizeof(u64), c->stream));  // (a partial count of the launch that gave up)
        return UKM_OK;
    }
    c->stat_window_route = ROUTE_STRIPWIN;
    UKM_TRY(check_legal(res));
    if (p.fhist) fused->shift = fsh;
    *done = true;
    return UKM_OK;
}

// ---- any input: window_kernel ----------------------------------------------------------------------------------------
int launch_window_kernel(ukm_ctx *c, bool hash, bool filter, const u8 *bases, const u64 *rec_off, const u64 *out_off, u64 n_rec, int k,
                         int canonical, int circular, u64 max_hash, u64 *out, u64 out_cap, u64 total_bases, u64 ntiles,
                         const LbCtl &blk, u64 res[2]) {
    WinArgs p;
    memset(&p, 0, sizeof(p));
    p.bases = bases; p.rec_off = rec_off; p.out_off = out_off; p.n_rec = n_rec;
    p.total_bases = total_bases; p.k = k; p.canonical = canonical; p.circular = circular;
    p.max_hash = max_hash; p.out = out; p.out_cap = out_cap; p.ntiles = ntiles;
    bind_ctl(p, blk);
    UKM_TRY(first_rec_of_tiles(c, rec_off, n_rec, total_bases, ntiles, (u64)WT, &p.tile_rec));
    const LbLaunch how = {"window kernel", "ntHash filter kernel", filter ? ENC_FLAG_TIMEOUT : 0, true, false, false};
    UKM_TRY(ukm_lb_launch(c, blk, how, [&](bool ticket) {
        if (!hash) hipLaunchKernelGGL((window_kernel<false, false>), dim3((unsigned)ntiles), dim3(NT), 0, c->stream, p);
        else if (!filter) hipLaunchKernelGGL((window_kernel<true, false>), dim3((unsigned)ntiles), dim3(NT), 0, c->stream, p);
        else return launch_tiles(window_kernel<true, true, false>, window_kernel<true, true, true>, ticket, ntiles, NT, c->stream, p);
        return UKM_OK;
    }, res));
    c->stat_window_route = ROUTE_WINDOW;
    return check_legal(res);
}

// fused (may be null; ukm_count): see FusedHist
int run_windows(ukm_ctx *c, bool hash, const u8 *bases, const u64 *rec_off, u64 n_rec, int k,
                int canonical, int circular, u64 max_hash, u64 *out, u64 out_cap, u64 *n_out,
                u64 total_bases, const u64 **win_off = nullptr, FusedHist *fused = nullptr) {
    *n_out = 0;
    c->stat_window_route = ROUTE_NO_LAUNCH;
    if (fused) fused->shift = -1;
    if (win_off) *win_off = nullptr;
    if (n_rec == 0 || total_bases == 0) return UKM_OK;
    const bool filter = hash && max_hash != 0;
    bool done = false;
    // Scaled-MinHash sketch: the rolling strip kernel when the filter is selective enough
    if (filter && !circular && !win_off) {
        if (const int L = strip_filter_L(c, bases, canonical, max_hash, total_bases))
            UKM_TRY(launch_strip_filter(c, L, bases, rec_off, n_rec, k, canonical, max_hash, out, out_cap, n_out, total_bases, &done));
        if (done) return UKM_OK;
    }
    // per-record window counts -> exclusive scan (n_rec + 1 entries: off[n_rec] = total)
    u64 *cnt = nullptr, *off = nullptr;
    UKM_TRY(ws_alloc_t(c, n_rec + 1, &cnt));
    UKM_TRY(ws_alloc_t(c, n_rec + 1, &off));
    if (win_off) *win_off = off;
    hipLaunchKernelGGL(window_count_kernel, dim3((unsigned)((n_rec + 1 + 255) / 256)), dim3(256), 0, c->stream,
                       rec_off, n_rec, k, circular, cnt);
    const u64 ntiles = (total_bases + WT - 1) / WT;
    LbCtl blk;  // (only the filter compacts: no status lines without it)
    UKM_TRY(ukm_lb_ctl_alloc(c, filter ? ntiles : 0, 0, &blk));
    u64 *total_dev = blk.result + 3;  // (one of the head's free words; read before the first launch zeroes the block)
    UKM_TRY(ukm_dev_exclusive_scan_u64(c, cnt, off, n_rec + 1, total_dev));
    u64 total_windows = 0;
    UKM_TRY(ukm_read_u64(c, total_dev, &total_windows));
    if (total_windows == 0) return UKM_OK;
    // without a filter the size is known before any window is written
    if (!filter && total_windows > out_cap) {
        *n_out = total_windows;
        return check_capacity(total_windows, out_cap);
    }
    // long records: the rolling strip kernel
    if (!circular && !filter) {
        if (const int L = strip_windows_L(c, hash, bases, n_rec, k, total_bases))
            UKM_TRY(launch_strip_windows(c, L, hash, bases, rec_off, off, n_rec, k, canonical, out, total_bases, total_windows, blk, &done, fused));
        if (done) {
            *n_out = total_windows;
            return UKM_OK;
        }
    }
    // the general kernel
    u64 res[2] = {0, 0};
    UKM_TRY(launch_window_kernel(c, hash, filter, bases, rec_off, off, n_rec, k, canonical, circular, max_hash, out, out_cap, total_bases,
                                 ntiles, blk, res));
    *n_out = filter ? res[0] : total_windows;
    return check_capacity(*n_out, out_cap);
}

int run_minimizer(ukm_ctx *c, const u8 *bases, const u64 *rec_off, u64 n_rec, int k, int w, int circular,
                  u64 max_hash, u64 *out, u64 *out_pos, u64 out_cap, u64 *n_out, u64 total_bases) {
    *n_out = 0;
    if (n_rec == 0 || total_bases == 0) return UKM_OK;
    // every canonical hash, in a workspace buffer (windows <= bases, also when circular)
    u64 *h = nullptr;
    UKM_TRY(ws_alloc_t(c, total_bases, &h));
    u64 n_h = 0;
    const u64 *off = nullptr;
    UKM_TRY(run_windows(c, true, bases, rec_off, n_rec, k, 1, circular, 0, h, total_bases, &n_h, total_bases, &off));
    if (n_h == 0) return UKM_OK;
    const u64 ntiles = (n_h + MT - 1) / MT;
    LbCtl blk;
    UKM_TRY(ukm_lb_ctl_alloc(c, ntiles, 0, &blk));
    MinArgs p;
    memset(&p, 0, sizeof(p));
    p.h = h; p.off = off; p.n_rec = n_rec; p.total = n_h; p.w = w; p.max_hash = max_hash;
    p.out = out; p.out_pos = out_pos; p.out_cap = out_cap; p.ntiles = ntiles;
    bind_ctl(p, blk);
    UKM_TRY(first_rec_of_tiles(c, off, n_rec, n_h, ntiles, (u64)MT, &p.tile_rec));
    u64 res[2] = {0, 0};
    const LbLaunch how = {"minimizer kernel", "minimizer kernel", ENC_FLAG_TIMEOUT, true, false, false};
    UKM_TRY(ukm_lb_launch(c, blk, how, [&](bool ticket) {
        return launch_tiles(minimizer_kernel<false>, minimizer_kernel<true>, ticket, ntiles, NT, c->stream, p);
    }, res));
    *n_out = res[0];
    return check_capacity(res[0], out_cap);
}

// ---- what the C entries share ----------------------------------------------------------------------------------------
// the NULL test and the range of k of every entry over (bases, rec_off) that writes values into out[out_cap]
int check_window_args(const char *name, const void *ctx, const void *n_out, const void *out, u64 out_cap, const void *bases,
                      const void *rec_off, u64 n_rec, int k, int hashed) {
    if (!ctx || !n_out || (!out && out_cap) || (n_rec && (!rec_off || !bases))) UKM_FAIL(UKM_ERR_INVALID, "%s: NULL argument", name);
    if (k < 1 || k > (hashed ? 64 : 32)) UKM_FAIL(UKM_ERR_K, "%s: k = %d out of range", name, k);
    return UKM_OK;
}

int windows_entry(ukm_ctx *ctx, bool hash, const uint8_t *bases, const uint64_t *rec_off,
                  uint64_t n_rec, int k, int canonical, int circular, uint64_t max_hash,
                  uint64_t *out, uint64_t out_cap, uint64_t *n_out, const char *name) {
    UKM_TRY(check_window_args(name, ctx, n_out, out, out_cap, bases, rec_off, n_rec, k, hash));
    *n_out = 0;
    if (n_rec == 0) return UKM_OK;
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        const u64 *off = nullptr;
        const u8 *b = nullptr;
        u64 total_bases = 0;
        UKM_TRY(ukm_dev_stage_records(ctx, name, bases, rec_off, n_rec, &off, &b, &total_bases));
        u64 *o = nullptr;
        UKM_TRY(ukm_out_t(ctx, out, out_cap, &o));
        int r = run_windows(ctx, hash, b, off, n_rec, k, canonical, circular, max_hash, o, out_cap, n_out, total_bases);
        ukm_out_resize(ctx, out, (r == UKM_OK ? *n_out : 0) * sizeof(u64));
        return r;
    }();
    return ukm_finish(&s, rc);
}

// ukm_count: the size of the window buffer.  windows <= bases (circular records: one per base); with a Scaled filter a
// small share of them, an estimate that the caller's retry loop corrects when a low-complexity input defeats it
u64 count_window_estimate(u64 total_bases, int hashed, u64 max_hash) {
    u64 wcap = total_bases + 1;
    if (hashed && max_hash && max_hash != ~0ull) {
        const double keep = 2.0 * ((double)max_hash / 18446744073709551615.0);  // canonical = the smaller of two hashes
        wcap = std::min<u64>(wcap, (u64)((double)total_bases * std::min(1.0, 1.5 * keep)) + (1u << 20));
    }
    return wcap;
}
// ukm_count: the number of low bits its sort has to look at (2k for codes; every hash that passed the filter is <= max_hash)
int count_sort_bits(int k, int hashed, u64 max_hash) {
    if (hashed && max_hash && max_hash != ~0ull) return 64 - __builtin_clzll(max_hash);
    return hashed ? 64 : 2 * k;
}

}  // namespace

// run_windows for the library's other files (ukm_map.h)
int ukm_dev_windows(ukm_ctx *c, bool hash, const u8 *bases, const u64 *rec_off, u64 n_rec, int k, int canonical, int circular,
                    u64 *out, u64 out_cap, u64 *n_out, u64 total_bases, const u64 **win_off) {
    return run_windows(c, hash, bases, rec_off, n_rec, k, canonical, circular, 0, out, out_cap, n_out, total_bases, win_off);
}

// the first step of every entry over (bases, rec_off) (ukm_map.h)
int ukm_dev_stage_records(ukm_ctx *c, const char *name, const u8 *bases, const u64 *rec_off, u64 n_rec, const u64 **rec_off_dev,
                          const u8 **bases_dev, u64 *total_bases) {
    UKM_TRY(ukm_in_t(c, rec_off, n_rec + 1, rec_off_dev));
    // the total number of bases is rec_off[n_rec]; rec_off[0] must be 0
    u64 first = 0;
    if (ukm_is_device_ptr(rec_off)) {
        UKM_TRY(ukm_read_u64(c, *rec_off_dev + n_rec, total_bases));
        UKM_TRY(ukm_read_u64(c, *rec_off_dev, &first));
    } else {
        *total_bases = rec_off[n_rec];
        first = rec_off[0];
    }
    if (first != 0) UKM_FAIL(UKM_ERR_INVALID, "%s: rec_off[0] must be 0", name);
    return ukm_in_t(c, bases, (size_t)*total_bases, bases_dev);
}

extern "C" int ukm_encode_kmers(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off,
                                uint64_t n_rec, int k, int canonical, int circular, uint64_t *out,
                                uint64_t out_cap, uint64_t *n_out) {
    return windows_entry(ctx, false, bases, rec_off, n_rec, k, canonical, circular, 0, out, out_cap, n_out,
                         "ukm_encode_kmers");
}

extern "C" int ukm_nthash(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off, uint64_t n_rec,
                          int k, int canonical, int circular, uint64_t max_hash, uint64_t *out,
                          uint64_t out_cap, uint64_t *n_out) {
    return windows_entry(ctx, true, bases, rec_off, n_rec, k, canonical, circular, max_hash, out, out_cap, n_out,
                         "ukm_nthash");
}

// sketches.NewMinimizerSketch(seq, k, w, circular).NextMinimizer() (count.go:316,357) + the Scaled
// filter applied to the emitted minimizers (count.go:373-375)
extern "C" int ukm_minimizer(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off, uint64_t n_rec,
                             int k, int w, int circular, uint64_t max_hash, uint64_t *out,
                             uint64_t *out_pos, uint64_t out_cap, uint64_t *n_out) {
    const char *name = "ukm_minimizer";
    UKM_TRY(check_window_args(name, ctx, n_out, out, out_cap, bases, rec_off, n_rec, k, 1));
    if (w < 1 || w > MW_MAX) UKM_FAIL(UKM_ERR_INVALID, "%s: w = %d out of range [1, %d]", name, w, MW_MAX);
    *n_out = 0;
    if (n_rec == 0) return UKM_OK;
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        const u64 *off = nullptr;
        const u8 *b = nullptr;
        u64 total_bases = 0;
        UKM_TRY(ukm_dev_stage_records(ctx, name, bases, rec_off, n_rec, &off, &b, &total_bases));
        u64 *o = nullptr, *op = nullptr;
        UKM_TRY(ukm_out_t(ctx, out, out_cap, &o));
        if (out_pos) UKM_TRY(ukm_out_t(ctx, out_pos, out_cap, &op));
        int r = run_minimizer(ctx, b, off, n_rec, k, w, circular, max_hash, o, op, out_cap, n_out, total_bases);
        ukm_out_resize(ctx, out, (r == UKM_OK ? *n_out : 0) * sizeof(u64));
        if (out_pos) ukm_out_resize(ctx, out_pos, (r == UKM_OK ? *n_out : 0) * sizeof(u64));
        return r;
    }();
    return ukm_finish(&s, rc);
}

// `count` in ONE call: every window (codes, or ntHash with the Scaled filter) -> sort -> the distinct / repeated / singleton
// set, the body of the Run closure count.go:285-436 (iterator, `m[code] = struct{}{}` per k-mer, the `-u` / `-d` marks) and
// its sort count.go:581.  The windows never leave the device: they are produced into the context's workspace, sorted there
// and reduced into `out`; one stream synchronisation and one read-back for the whole call instead of three of each (round-5
// review: the CLI's count_on_device was the caller the fused entry point did not have).
extern "C" int ukm_count(ukm_ctx *ctx, const uint8_t *bases, const uint64_t *rec_off, uint64_t n_rec, int k, int canonical,
                         int circular, int hashed, uint64_t max_hash, int mode, uint64_t *out, uint64_t out_cap, uint64_t *n_out) {
    const char *name = "ukm_count";
    UKM_TRY(check_window_args(name, ctx, n_out, out, out_cap, bases, rec_off, n_rec, k, hashed));
    if (mode != UKM_UNIQUE && mode != UKM_REPEATED && mode != UKM_SINGLETON)
        UKM_FAIL(UKM_ERR_INVALID, "%s: mode must be UKM_UNIQUE, UKM_REPEATED (-d) or UKM_SINGLETON (-u)", name);
    if (!hashed && max_hash) UKM_FAIL(UKM_ERR_INVALID, "%s: max_hash (--scale) needs hashed = 1", name);
    *n_out = 0;
    if (n_rec == 0) return UKM_OK;
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        const u64 *off = nullptr;
        const u8 *b = nullptr;
        u64 total_bases = 0;
        UKM_TRY(ukm_dev_stage_records(ctx, name, bases, rec_off, n_rec, &off, &b, &total_bases));
        u64 *o = nullptr;
        UKM_TRY(ukm_out_t(ctx, out, out_cap, &o));
        u64 wcap = count_window_estimate(total_bases, hashed, max_hash);
        const bool estimated = wcap < total_bases + 1;
        const int bits = count_sort_bits(k, hashed, max_hash);
        // the sort's first histogram is counted by the kernel that writes the windows (the strip kernel, when it runs)
        FusedHist fh = {nullptr, bits, -1};
        UKM_TRY(ws_alloc_t(ctx, 256, &fh.hist));
        const WsMark before_w = ws_mark(ctx);
        u64 *w = nullptr;
        u64 nw = 0;
        for (int pass = 0;; pass++) {
            UKM_TRY(ws_alloc_t(ctx, (size_t)wcap, &w));
            UKM_HIP(hipMemsetAsync(fh.hist, 0, 256 * sizeof(u64), ctx->stream));
            fh.shift = -1;
            const int rw = run_windows(ctx, hashed != 0, b, off, n_rec, k, canonical, circular, max_hash, w, wcap, &nw, total_bases, nullptr, &fh);
            // More windows passed the Scaled filter than the estimate allowed for (a low-complexity record whose one hash lies
            // below max_hash): the buffer is the library's own, so this is not the caller's UKM_ERR_CAPACITY.  The filter
            // kernel has counted past the cap with its stores guarded and run_windows has read the count back (the stream is
            // idle): the pass runs once more into a buffer of exactly that size.
            if (rw != UKM_ERR_CAPACITY || !estimated || pass > 0 || nw <= wcap) {
                UKM_TRY(rw);
                break;
            }
            ctx->stat_count_window_retries++;
            ws_release(ctx, before_w);
            wcap = nw;
        }
        if (nw == 0) {
            ukm_out_resize(ctx, out, 0);
            return UKM_OK;
        }
        UKM_TRY(ukm_dev_sort_hist(ctx, w, nullptr, nw, bits, fh.shift >= 0 ? fh.hist : nullptr, fh.shift));
        int r = ukm_dev_unique(ctx, w, nullptr, nw, mode, o, nullptr, out_cap, n_out);
        ukm_out_resize(ctx, out, (r == UKM_OK ? *n_out : 0) * sizeof(u64));
        return r;
    }();
    return ukm_finish(&s, rc);
}

// count.go:98  maxHash := uint64(float64(^uint64(0)) / float64(scale))
extern "C" uint64_t ukm_max_hash(uint64_t scale) {
    if (scale <= 1) return ~0ull;
    double d = 18446744073709551615.0 / (double)scale;  // float64(^uint64(0)) rounds to 2^64
    return (uint64_t)d;
}
