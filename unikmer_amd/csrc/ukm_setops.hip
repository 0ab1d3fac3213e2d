// ukm_setops.hip — 2-way sorted set operations (union / inter / diff) on device-resident
// (code uint64 [, taxid uint32]) streams: the MI355X replacement for the reference's per-k-mer
// hash-map / 2-pointer loops (union.go:186-208, inter.go:205-278, diff.go:379-454).
//
// One translation unit in four files.  This one holds the host side: the choice of the tile variant, the passes, the
// chained link, the device-level entries and the C ABI.  The device code is in three headers that nothing else includes:
//   ukm_setop_part.h     SetopArgs, the result flags, the merge-path partition and its launcher
//   ukm_setop_tile.h     the building blocks of a tile (staging, order check, merge loops, compaction, flushes)
//   ukm_setop_kernels.h  the tile kernels, the taxid epilogues, the launchers; Tiles / Variant / launch_variant
//
// Design (HBM-bound integer path, no MFMA):
//   1. partition  — the merge-path split of every tile boundary (A before B on ties) -> mp[t], in one of three forms
//                   (PartKernels): FUSED, from 4 x 64 tiles: a workgroup per segment of 64 boundaries places the segment's
//                   two ends with a wave's 64-ary search over the whole inputs and the others with a thread's bracketed
//                   binary search between them, and clears the control block on the way -- one launch; TWO_LEVEL, the same
//                   two levels as two kernels (a chained link of many tiles, whose sizes are on the device); SINGLE, a wave
//                   per boundary (few tiles).
//      The public entry keeps the table of its last call in the context (ukm_ctx::PartCache), and a pass has one of three
//      plans (Plan): SEARCH as above; VERIFY_LOOKBACK: the cached table, checked against the inputs as they are now, one
//      thread per boundary; VERIFY_TABLE: the cached match counts as well, which give every tile its output offset before
//      the launch.  A table or counts that no longer hold cost a second pass, never a wrong result (run_setop_pass).
//   2. tile kernel — one 512-thread workgroup per tile of NTS * VT merged items; VT by variant (Tiles): 19 for plain codes
//                   and one taxid per file (9728 items, 76 KiB of LDS, two workgroups per CU), 7 with per-record taxids
//                   (3584 items, three per CU), 12 where ranks or a diff's taxids ride along (6144 items):
//        * coalesced loads of the tile's A range and B range (+1-element halos) into LDS -- interior tiles of plain
//          codes by LDS-DMA, without a register round trip,
//        * per-thread merge-path search in LDS, then a VT-step serial merge that decides
//          emit/skip per item from the neighbouring element (sets: an equal pair is adjacent),
//          checking strict sortedness of both inputs on the fly,
//        * wave64 shuffle scan + LDS for the block prefix, single-pass decoupled look-back
//          over tile aggregates (blockIdx-ordered or ticketed tile ids, agent-scope 8-byte status words) for the
//          global output offset -- or no look-back at all under VERIFY_TABLE; inputs are read once and outputs
//          written once,
//        * survivors compacted through LDS and stored as contiguous coalesced runs.
//   3. ukm_setop2_multi — two or three operations of one pair of plain codes from ONE merge: setop_multi_tile_kernel
//                   (512 x 19) publishes the tiles' MATCH counts, and one look-back over them places all outputs.  A
//                   partition of its own, no cache.
//   Algorithmic bytes per launch: 8(|A|+|B|) read + 8|out| written (12 B/record with taxids).
//   Multisets (duplicate codes inside an input; legal for `inter`/`diff`, inter.go:198) are
//   detected by the fast path and re-run on (code, rank-in-run) pairs, which reproduces the
//   reference's "equality advances both cursors" semantics exactly.
#include <algorithm>

#include "ukm_device.h"
#include "ukm_setop_order.h"

namespace {

#include "ukm_setop_part.h"
#include "ukm_setop_tile.h"
#include "ukm_setop_kernels.h"

// Operations that take their tile offsets from the cached match counts whatever the size, 1 << op each (union 1, inter 2,
// diff 4): inter's TABLE kernel is 0.4 ms faster than its look-back at 2 x 1e9 (profiles/offs_reuse_notes.md section 3).
// The union's, with tile = block, tied with its look-back; with each XCD on consecutive tiles (below) it is 6 to 9 % faster
// at every size measured, 2 x 1e7 to 2 x 1e9 (profiles/xcd_order_notes.md): the union takes the table from
// SETOP_OFFS_UNION_MIN_TILES tiles, the smallest size measured, and keeps the look-back below.
#ifndef SETOP_OFFS_OPS
#define SETOP_OFFS_OPS 6
#endif
#ifndef SETOP_OFFS_UNION_MIN_TILES
#define SETOP_OFFS_UNION_MIN_TILES 2048  /* 2 x 1e7 codes are 2056 tiles */
#endif
// The tile order of a TABLE pass, 1 << op each: set = each XCD runs a range of consecutive tiles (ukm_setop_order.h), clear
// = tile = block.  The union gains 0.3 ms of 4.8 at 2 x 1e9; the intersection, which stores a third as much, LOSES 1 to
// 4 % at every size (profiles/xcd_order_notes.md), and the difference is the intersection's shape.  UKM_SETOP_XCD_ORDER=0|1
// (developer knob): no table pass / every table pass.
#ifndef SETOP_XCD_ORDER
#define SETOP_XCD_ORDER 1
#endif

// what a pass and a chained link (na = the bound, the link adds na_dev) hand to their kernels, less the control block
SetopArgs setop_args(ukm_ctx *c, const u64 *a, const u32 *ta, const u32 *ra, u64 na, const u64 *b, const u32 *tb, const u32 *rb, u64 nb,
                     u64 tile_items, u32 flags, u64 *out, u32 *tout, u64 out_cap, u32 cta, u32 ctb) {
    SetopArgs p;
    memset(&p, 0, sizeof(p));
    p.a = a; p.b = b; p.ta = ta; p.tb = tb; p.ra = ra; p.rb = rb;
    p.na = na; p.nb = nb;
    p.out = out; p.tout = tout; p.out_cap = out_cap;
    p.ntiles = (na + nb + tile_items - 1) / tile_items;
    p.tax = ukm_taxdev(c);
    p.flags = flags;
    p.cta = cta;
    p.ctb = ctb;
    return p;
}

// the control block of a launch, where the kernels look for it; the partition points are the words behind its status lines
void bind_ctl(SetopArgs &p, const LbCtl &blk) {
    p.result = blk.result;
    p.ticket = blk.ticket;
    p.status = blk.status;
    p.mp = blk.tail;
}

// The host side of -DUKM_PROFILE_PHASES (the kernels' side: PH_BEGIN / PH / PH_END in ukm_setop_kernels.h): eight words per
// tile in front of the launches, and behind them one line on stderr, "[phases <label> tiles=N] cycles per tile: p0=.. ..
// total=..".  Nothing in the product build.
// (the words are indexed by BLOCK: a table pass in XCD order has up to ukm_setop_order::XCDS - 1 more blocks than tiles)
int setop_phases_begin(ukm_ctx *c, SetopArgs &p) {
#ifdef UKM_PROFILE_PHASES
    const size_t nblocks = (size_t)ukm_setop_order::grid_of(p.ntiles, 1);
    UKM_TRY(ws_alloc_t(c, nblocks * 8, &p.dbg));
    UKM_HIP(hipMemsetAsync(p.dbg, 0, nblocks * 8 * sizeof(u64), c->stream));
#endif
    return UKM_OK;
}
int setop_phases_report(const SetopArgs &p, const char *label_fmt, int label_arg) {
#ifdef UKM_PROFILE_PHASES
    const size_t nblocks = (size_t)ukm_setop_order::grid_of(p.ntiles, 1);
    std::vector<u64> h(nblocks * 8);
    UKM_HIP(hipMemcpy(h.data(), p.dbg, h.size() * sizeof(u64), hipMemcpyDeviceToHost));
    double sum[8] = {0};
    for (size_t t = 0; t < nblocks; t++) for (int i = 0; i < 8; i++) sum[i] += (double)h[t * 8 + i];
    double tot = 0; for (int i = 0; i < 7; i++) tot += sum[i];
    fprintf(stderr, "[phases ");
    fprintf(stderr, label_fmt, label_arg);
    fprintf(stderr, " tiles=%llu] cycles per tile:", (unsigned long long)p.ntiles);
    for (int i = 0; i < 7; i++) fprintf(stderr, " p%d=%.0f", i, sum[i] / sum[7]);
    fprintf(stderr, " total=%.0f\n", tot / sum[7]);
#endif
    return UKM_OK;
}

// Which tiles a pass launches (Tiles, ukm_setop_kernels.h).  tax: the records carry taxids; a stream whose ta / tb is null
// carries its file's (SetopArgs::cta); ra != null: the multiset re-run.
Variant choose_variant(ukm_ctx *c, int op, bool tax, const u32 *ta, const u32 *tb, const u32 *ra, u32 flags) {
    const bool rank = ra != nullptr;
    bool ct = tax && !ta && !tb;
    // per-record taxids on plain sets: EITHER the taxid instantiation (on a taxonomy with one-byte clade codes its DEFER
    // form: small tiles, the LCAs walked densely behind the merge loop) OR the plain-key kernel writing a source word per
    // output record + a second launch that turns the words into taxids (tile_flush_src / setop_taxid_gather_kernel).
    // Round 6, 2 x 3e8 records, inter: uniformly random taxids 3.66 against 4.32 ms, taxids that repeat (one per file as
    // arrays, runs of 4096) 2.62 against 2.41 -- the taxid instantiation is the default where its DEFER form exists, the
    // source words where it does not (round 5: 1.60 against 1.78 ms at 2 x 1e8 with the look-ups inside the merge step);
    // union loses through the words by 20 % either way.  UKM_SETOP_SRC: 0 = never, 1 = inter, 2 = every operation but
    // diff -t, whose survivors depend on their taxids; never the multiset re-run with ranks.
    const bool defer_form = SETOP_TAX_DEFER != 0 && c->tax_pair != nullptr && !ukm_env_is(c, "UKM_SETOP_DEFER", '0');
    const int src_mode = ukm_env_int(c, "UKM_SETOP_SRC", defer_form ? 0 : 1);
    if (tax && !ct && !rank && src_mode != 0 && (op == UKM_OP_INTER || (src_mode == 2 && !(op == UKM_OP_DIFF && (flags & UKM_F_CMP_TAXID))))) ct = true;
    if (ct) tax = false;  // the plain-key kernel; the taxids are an epilogue of it
    // (diff WITHOUT -t carries the taxids along and looks nothing up: the large tile, two workgroups per CU -- 2.22 against
    //  2.35 ms at 2 x 3e8 through the small one)
    const bool tax_stream = tax && !rank && op == UKM_OP_DIFF && !(flags & UKM_F_CMP_TAXID);
    Variant v = {Tiles::PLAIN, false};
    if (rank) v.tiles = tax ? Tiles::RANK_TAX : (ct ? Tiles::RANK_CT : Tiles::RANK);
    else if (tax_stream) v.tiles = Tiles::TAX_STREAM;
    else if (tax) v.tiles = defer_form ? Tiles::TAX_DEFER : Tiles::TAX;
    else if (ct) v.tiles = Tiles::CT;
    v.fix = v.tiles == Tiles::TAX_DEFER && (op == UKM_OP_UNION || op == UKM_OP_INTER) && !ukm_env_is(c, "UKM_SETOP_FIX", '0');
    return v;
}

// How a pass gets its merge-path table and its tiles' output offsets, and what it does about the slot's match counts
// (DESIGN.md section 4.1 has the table of cases).  Chosen once; only the two downgrades of pass_downgrade change it.
enum class Plan {
    SEARCH,           // a partition launch fills the table; offsets by look-back
    VERIFY_LOOKBACK,  // the cached table, verified; offsets by look-back
    VERIFY_TABLE,     // the cached table and counts, verified; offsets from the counts (TABLE tiles, no look-back)
};
enum class Counts {
    NONE,    // the pass leaves no valid counts in the slot
    KEPT,    // the slot's counts are valid and stay (VERIFY_TABLE: and are used)
    RECORD,  // setop_counts_record_kernel writes them behind the look-back
};

// One pass of the tiled set operation, as its steps hand it on (run_setop_pass).
struct Pass {
    ukm_ctx *c;
    int op;
    Variant v;
    u64 tile_items;
    SetopArgs p;
    LbCtl blk;
    bool two_level, fused;  // the partition kernels of a search: PartKernels::FUSED, TWO_LEVEL, or neither: SINGLE
    ukm_ctx::PartCache::Key key;
    bool cache;    // the pass works on the context's slot: p.mp is the slot's table, p.stale its stale word
    bool offs_on;  // ... and the slot's match counts are in play: used, kept or recorded
    Plan plan;
    Counts counts;
};

// The cache policy and the plan that follows from what the slot holds.
void pass_open_cache(Pass &s, bool may_cache) {
    ukm_ctx *c = s.c;
    SetopArgs &p = s.p;
    // The partition cache (ukm_ctx::PartCache): only where the fused kernel would run -- below 4 * PART_COARSE tiles the
    // partition is a 12 us kernel --, never with ranks (the multiset re-run), never on a chained link (sizes on the device:
    // another entry point).  UKM_SETOP_PART_REUSE=0 (developer knob) turns it off.
    ukm_ctx::PartCache &pc = c->part_cache;
    s.key = {p.a, p.b, p.na, p.nb, s.tile_items};
    s.cache = may_cache && s.fused && !s.v.rank() && p.na && p.nb && !pc.off && !ukm_env_is(c, "UKM_SETOP_PART_REUSE", '0') && pc.reserve(p.ntiles);
    // The match counts MP of the slot (its second column; setop_offset_of has the formulas): a plain-key union / inter /
    // diff that hits the partition cache while they are valid takes its tiles' output offsets from them -- the TABLE
    // instantiation, no look-back -- and every other such pass on the slot's table records them behind its look-back.
    // UKM_SETOP_OFFS_REUSE=0 turns both off; UKM_SETOP_OFFS_OPS (developer knob) = which operations use the counts,
    // 1 << op each (profiles/offs_reuse_notes.md has the measurements behind the default).
    const bool plain3 = s.v.tiles == Tiles::PLAIN && (s.op == UKM_OP_UNION || s.op == UKM_OP_INTER || s.op == UKM_OP_DIFF);
    s.offs_on = s.cache && plain3 && !pc.offs_off && !ukm_env_is(c, "UKM_SETOP_OFFS_REUSE", '0');
    s.plan = Plan::SEARCH;
    s.counts = s.offs_on ? Counts::RECORD : Counts::NONE;
    if (!s.cache) return;
    const ukm_ctx::PartCache::Opened slot = pc.open(s.key);
    p.stale = pc.stale_word();
    p.mp = pc.table();
    if (slot.hit) {
        s.plan = Plan::VERIFY_LOOKBACK;
        if (slot.counts) {  // the column still belongs to the table this pass works on
            s.counts = Counts::KEPT;
            // the default: SETOP_OFFS_OPS, and the union from SETOP_OFFS_UNION_MIN_TILES tiles; the knob names the operations itself
            const int large_union = p.ntiles >= SETOP_OFFS_UNION_MIN_TILES ? 1 << UKM_OP_UNION : 0;
            if (s.offs_on && ((ukm_env_int(c, "UKM_SETOP_OFFS_OPS", SETOP_OFFS_OPS | large_union) >> s.op) & 1) != 0) s.plan = Plan::VERIFY_TABLE;
            // the table pass's tile order (a grid of whole chunks that no longer fits 32 bits: tile = block)
            const int xcd_knob = ukm_env_int(c, "UKM_SETOP_XCD_ORDER", -1);
            const int xcd_ops = xcd_knob < 0 ? SETOP_XCD_ORDER : (xcd_knob ? 7 : 0);
            if (s.plan == Plan::VERIFY_TABLE && ((xcd_ops >> s.op) & 1) != 0 && ukm_setop_order::grid_of(p.ntiles, 1) <= 0xFFFFFFFFull)
                p.xcd_order = 1;
        }
    }
}

// The partition points (they survive a repeated launch): searched, or the slot's verified.  A plain call's search takes the
// fused kernel, which also zeroes the control block for the first attempt; the verification does the same.
int pass_partition(Pass &s) {
    ukm_ctx *c = s.c;
    SetopArgs &p = s.p;
    if (s.plan == Plan::SEARCH)
        return launch_partition(c, p, s.tile_items, s.v.rank(), s.fused ? PartKernels::FUSED : (s.two_level ? PartKernels::TWO_LEVEL : PartKernels::SINGLE));
    p.base = s.blk.tail;  // (the arena's table words, which p.mp does not occupy on a cached pass)
    hipLaunchKernelGGL(setop_partition_verify_kernel, dim3((unsigned)((p.ntiles + 1 + 255) / 256)), dim3(256), 0, c->stream, p, (int)s.tile_items,
                       (u32)LbCtl::HEAD, s.plan == Plan::VERIFY_TABLE ? (const u64 *)c->part_cache.counts(p.ntiles) : (const u64 *)nullptr, s.op);
    UKM_HIP(hipGetLastError());
    return UKM_OK;
}

// The tiles of the plan as it stands, through the watchdog ladder; result_host[0] = total, [1] = flags.
// first_zeroed: a kernel of pass_partition has cleared the control block for the first attempt.
int pass_launch(Pass &s, bool first_zeroed, u64 result_host[2]) {
    ukm_ctx *c = s.c;
    // (the bracket holds the tile kernel with its CT / fix / gather kernels, not the partition)
    const LbLaunch how = {"setop", "set-op kernel", FLAG_TIMEOUT, true, false, first_zeroed};
    return ukm_lb_launch(c, s.blk, how, [&](bool ticket) {
        const SetopArgs &p = s.p;
        if (s.plan == Plan::VERIFY_TABLE) launch_table_tiles(s.op, p, c->stream);
        else launch_variant(s.v, s.op, p, c->stream, ticket);
        if (s.counts == Counts::RECORD)
            hipLaunchKernelGGL(setop_counts_record_kernel, dim3((unsigned)((p.ntiles + 1 + 255) / 256)), dim3(256), 0, c->stream, p, (int)s.tile_items, s.op,
                               c->part_cache.counts(p.ntiles));
        if (p.stale) hipLaunchKernelGGL(setop_stale_report_kernel, dim3(1), dim3(1), 0, c->stream, p);
        return UKM_OK;
    }, result_host);
}

// The two downgrades of a pass that worked on the slot, each taken once at the most.
int pass_downgrade(Pass &s, u64 result_host[2]) {
    ukm_ctx *c = s.c;
    ukm_ctx::PartCache &pc = c->part_cache;
    if (s.plan != Plan::SEARCH) {
        const bool stale = (result_host[1] & FLAG_STALE) != 0;
        pc.note_table(stale);
        if (stale) {
            // VERIFY_* -> SEARCH.  The buffers were rewritten under the key.  No tile has run (the other flags of that pass mean
            // nothing): the search after all -- the fused kernel, which clears the stale word and the control block; without
            // ranks, which the cache excludes -- and the launch again.  The counts go with the table: this pass records fresh ones.
            c->stat_setop_part_stale++;
            s.plan = Plan::SEARCH;
            s.counts = s.offs_on ? Counts::RECORD : Counts::NONE;
            UKM_TRY(pass_partition(s));
            UKM_TRY(pass_launch(s, s.fused, result_host));
        } else {
            c->stat_setop_part_hits++;
        }
    }
    if (s.plan == Plan::VERIFY_TABLE) {
        const u64 fl = result_host[1];
        if (!(fl & FLAG_OFFS)) {
            c->stat_setop_offs_hits++;
            pc.note_counts(false);
        } else if (!(fl & (FLAG_DUP | FLAG_UNSORTED))) {
            // VERIFY_TABLE -> VERIFY_LOOKBACK, on the same (verified) table.  The contents changed in place under an intact
            // partition: some tile counted another number of records than its step.  The output is void; the pass again with
            // the look-back (cleared control block and status lines: the verification cleared no status line) -- which
            // records fresh counts.
            c->stat_setop_offs_stale++;
            pc.note_counts(true);
            s.plan = Plan::VERIFY_LOOKBACK;
            s.counts = Counts::RECORD;
            UKM_TRY(pass_launch(s, false, result_host));
        } else {
            s.counts = Counts::NONE;  // duplicates or disorder beside FLAG_OFFS: the caller discards this pass anyway -- no second one
        }
        result_host[1] &= ~(u64)FLAG_OFFS;
    }
    return UKM_OK;
}

// One pass of the tiled set operation.  result_host[0] = total, [1] = flags.
// (cta, ctb): the file taxid of a stream whose ta / tb is null (SetopArgs); tax && !ta && !tb = the CT variant
// may_cache: a and b are the caller's own device buffers (the public 2-way entry): the pass may take its merge-path table
// from the context's partition cache, verified, and leave its own there.  Results never depend on the cache, only time does.
int run_setop_pass(ukm_ctx *c, int op, const u64 *a, const u32 *ta, const u32 *ra, u64 na,
                   const u64 *b, const u32 *tb, const u32 *rb, u64 nb, bool tax, u32 flags,
                   u64 *out, u32 *tout, u64 out_cap, u64 result_host[2], u32 cta = 0, u32 ctb = 0, bool may_cache = false) {
    Pass s;
    s.c = c;
    s.op = op;
    s.v = choose_variant(c, op, tax, ta, tb, ra, flags);
    s.tile_items = s.v.tile_items();
    SetopArgs &p = s.p;
    p = setop_args(c, a, ta, ra, na, b, tb, rb, nb, s.tile_items, flags, out, tout, out_cap, cta, ctb);
    if (p.ntiles > 0xFFFFFFFFull) UKM_FAIL(UKM_ERR_INVALID, "setop: input too large");
    UKM_TRY(ukm_lb_ctl_alloc(c, p.ntiles, p.ntiles + 1, &s.blk));  // the partition points behind it
    bind_ctl(p, s.blk);
    if (s.v.fix) {
        UKM_TRY(ws_alloc_t(c, (size_t)p.ntiles * FIX_SLOTS, &p.fix));
        UKM_TRY(ws_alloc_t(c, (size_t)p.ntiles, &p.fix_cnt));
    }
    UKM_TRY(setop_phases_begin(c, p));
    s.two_level = p.ntiles >= 4 * PART_COARSE;
    s.fused = s.two_level && !ukm_env_is(c, "UKM_SETOP_FUSED_PART", '0');  // (developer knob)
    pass_open_cache(s, may_cache);
    UKM_TRY(pass_partition(s));
    UKM_TRY(pass_launch(s, s.fused, result_host));
    UKM_TRY(pass_downgrade(s, result_host));
    if (result_host[1] & FLAG_STALE) UKM_FAIL(UKM_ERR_HIP, "setop: a fresh partition table failed its verification");
    // the counts: kept or freshly recorded, and only behind a pass that came back with no flag at all
    if (s.cache) c->part_cache.commit(s.key, s.counts != Counts::NONE && result_host[1] == 0);
    return setop_phases_report(p, "op=%d", op);
}

// One pass over plain codes that writes every operation of `ops` (1 << UKM_OP_x each, at least two).  result_host[0] = M,
// the number of matched pairs, [1] = flags.  A partition table of its own in the arena: the context's partition cache is
// neither read nor written, so the passes around this one find it as they left it.
int run_setop_multi_pass(ukm_ctx *c, u32 ops, const u64 *a, u64 na, const u64 *b, u64 nb, u64 *const out[3], const u64 out_cap[3],
                         u64 result_host[2]) {
    const u64 tile_items = (u64)NTS * VT_MULTI;
    SetopArgs p = setop_args(c, a, nullptr, nullptr, na, b, nullptr, nullptr, nb, tile_items, 0u, nullptr, nullptr, 0, 0u, 0u);
    if (p.ntiles > 0xFFFFFFFFull) UKM_FAIL(UKM_ERR_INVALID, "setop: input too large");
    SetopMultiOut mo;
    for (int x = 0; x < 3; x++) {
        const bool want = ((ops >> x) & 1u) != 0;
        mo.out[x] = want ? out[x] : nullptr;
        mo.cap[x] = want ? out_cap[x] : 0;
    }
    LbCtl blk;  // the partition points behind it
    UKM_TRY(ukm_lb_ctl_alloc(c, p.ntiles, p.ntiles + 1, &blk));
    bind_ctl(p, blk);
    UKM_TRY(setop_phases_begin(c, p));
    const bool fused = p.ntiles >= 4 * PART_COARSE;  // (the fused kernel also zeroes the control block for the first attempt)
    UKM_TRY(launch_partition(c, p, tile_items, false, fused ? PartKernels::FUSED : PartKernels::SINGLE));
    const LbLaunch how = {"setop_multi", "fused set-op kernel", FLAG_TIMEOUT, true, false, fused};
    UKM_TRY(ukm_lb_launch(c, blk, how, [&](bool ticket) {
        if (ops == 3u) launch_multi<3>(p, mo, c->stream, ticket);
        else if (ops == 5u) launch_multi<5>(p, mo, c->stream, ticket);
        else if (ops == 6u) launch_multi<6>(p, mo, c->stream, ticket);
        else launch_multi<7>(p, mo, c->stream, ticket);
        return UKM_OK;
    }, result_host));
    return setop_phases_report(p, "multi ops=%d", (int)ops);
}

}  // namespace

// Two or three operations of one pair.  ops: 1 << UKM_OP_x each; the arrays are indexed by UKM_OP_x and only the
// requested entries are touched.  Plain codes and at least two operations: one fused pass; everything else -- taxids of
// either kind, one operation, duplicate codes inside an input -- one ukm_dev_setop2_ct per operation (the split route).
int ukm_dev_setop2_multi(ukm_ctx *c, u32 ops, const u64 *a, const u32 *ta, u32 cta, u64 na, const u64 *b, const u32 *tb, u32 ctb,
                         u64 nb, u32 flags, u64 *const out[3], u32 *const tout[3], const u64 out_cap[3], u64 n_out[3]) {
    if (ops == 0 || ops >= 8u) UKM_FAIL(UKM_ERR_INVALID, "ukm_setop2_multi: ops %u names no operation or an unknown one", ops);
    if (ta) cta = 0;
    if (tb) ctb = 0;
    const bool tax = ta != nullptr || tb != nullptr || cta != 0 || ctb != 0;
    const bool part_cache = (flags & UKM_F_INTERNAL_PART_CACHE) != 0;
    flags &= ~UKM_F_INTERNAL_PART_CACHE;
    if (!tax && (ops & (ops - 1)) != 0 && na + nb > 0) {
        if (na + nb >= (1ull << 61)) UKM_FAIL(UKM_ERR_INVALID, "ukm_setop2_multi: input too large");
        u64 res[2] = {0, 0};
        UKM_TRY(run_setop_multi_pass(c, ops, a, na, b, nb, out, out_cap, res));
        if (res[1] & FLAG_UNSORTED) UKM_FAIL(UKM_ERR_UNSORTED, "ukm_setop2_multi: an input stream is not sorted");
        if (!(res[1] & FLAG_DUP)) {
            const u64 m = res[0];
            const u64 total[3] = {na + nb - m, m, na - m};
            bool fits = true;
            for (int x = 0; x < 3; x++) {
                if (!((ops >> x) & 1u)) continue;
                n_out[x] = total[x];
                if (total[x] > out_cap[x]) fits = false;
            }
            c->stat_setop_multi_fused++;
            if (!fits) UKM_FAIL(UKM_ERR_CAPACITY, "ukm_setop2_multi: an output needs more records than its capacity");
            // (a caller that wants taxids of streams that carry none: such records have taxid 0, as in ukm_dev_setop2_ct)
            for (int x = 0; x < 3; x++)
                if (((ops >> x) & 1u) && tout[x] && total[x]) UKM_HIP(hipMemsetAsync(tout[x], 0, total[x] * sizeof(u32), c->stream));
            return UKM_OK;
        }
        // multiset inputs: the rank re-run and the unique fold stay where they are
    }
    c->stat_setop_multi_split++;
    int rc = UKM_OK;
    for (int x = 0; x < 3; x++) {
        if (!((ops >> x) & 1u)) continue;
        // (every operation runs, so that every n_out holds the size needed when one of them does not fit)
        const int r = ukm_dev_setop2_ct(c, x, a, ta, cta, na, b, tb, ctb, nb, flags | (part_cache ? UKM_F_INTERNAL_PART_CACHE : 0u), out[x],
                                        tout[x], out_cap[x], &n_out[x]);
        if (r == UKM_ERR_CAPACITY) rc = r;
        else UKM_TRY(r);
    }
    return rc;
}

// internal entry: all pointers are device pointers
// One link of a chained fold: A's size is *na_dev (<= na_max), nothing is read back.  `ctl` = 8 zeroed words
// owned by the caller ([0] result count, [1] flags, [2] ticket) that stay valid until the chain is read;
// status lines and partition points come from the arena (the caller marks / releases around the call: the
// stream orders the next link's memset after this link's kernels).  Plain sets only (no rank path).
int ukm_dev_setop2_link(ukm_ctx *c, int op, const u64 *a, const u32 *ta, u64 na_max, const u64 *na_dev, const u64 *b,
                        const u32 *tb, u64 nb, u32 flags, u64 *out, u32 *tout, u64 out_cap, u64 *ctl, u32 cta, u32 ctb) {
    // A link's own, narrower choice: per-record taxids on either side go through the merge (never the DEFER or the source-word
    // form); both streams with one taxid per file: plain kernel + taxid epilogue (ctl[4]); else plain codes.
    const bool tax = (ta != nullptr) || (tb != nullptr) || cta != 0 || ctb != 0;
    const Variant v = {!tax ? Tiles::PLAIN : ((ta || tb) ? Tiles::TAX : Tiles::CT), false};
    const u64 tile_items = v.tile_items();
    SetopArgs p = setop_args(c, a, ta, nullptr, na_max, b, tb, nullptr, nb, tile_items, flags, out, tout, out_cap, cta, ctb);
    p.na_dev = na_dev;
    if (p.ntiles == 0) return UKM_OK;
#ifndef SETOP_LINK_SMALL_TILES
#define SETOP_LINK_SMALL_TILES 2048
#endif
    // links of up to a few thousand tiles: ONE partition kernel (a wave per boundary) that also clears the status lines
    // (three launches less per link than memset + two-level partition; a 1000-file fold is launch bound)
    const bool small = p.ntiles < SETOP_LINK_SMALL_TILES;
    LbCtl blk;  // the head is the caller's; one status line more than tiles, the partition points behind them
    UKM_TRY(ukm_lb_ctl_alloc(c, p.ntiles + 1, p.ntiles + 1, &blk, ctl));
    if (small) p.zero_status = (u32)(p.ntiles + 1);  // cleared by the partition kernel: one launch less
    else UKM_TRY(ukm_lb_ctl_zero(c, blk));
    bind_ctl(p, blk);
    UKM_TRY(launch_partition(c, p, tile_items, false, small ? PartKernels::SINGLE : PartKernels::TWO_LEVEL));
    launch_variant(v, op, p, c->stream, c->setop_force_ticket);
    // (neither stream carries taxids but the fold's later files do: these records have taxid 0)
    if (v.tiles == Tiles::PLAIN && tout && out_cap) UKM_HIP(hipMemsetAsync(tout, 0, out_cap * sizeof(u32), c->stream));
    UKM_HIP(hipGetLastError());
    return UKM_OK;
}

int ukm_dev_setop2(ukm_ctx *c, int op, const u64 *a, const u32 *ta, u64 na, const u64 *b,
                   const u32 *tb, u64 nb, u32 flags, u64 *out, u32 *tout, u64 out_cap, u64 *n_out) {
    return ukm_dev_setop2_ct(c, op, a, ta, 0u, na, b, tb, 0u, nb, flags, out, tout, out_cap, n_out);
}

// cta / ctb: the file taxid of a stream without per-record taxids (ta / tb null); 0 = the stream has no taxid at all
int ukm_dev_setop2_ct(ukm_ctx *c, int op, const u64 *a, const u32 *ta, u32 cta, u64 na, const u64 *b,
                      const u32 *tb, u32 ctb, u64 nb, u32 flags, u64 *out, u32 *tout, u64 out_cap, u64 *n_out) {
    if (op != UKM_OP_UNION && op != UKM_OP_INTER && op != UKM_OP_DIFF && op != UKM_OP_MERGE_INTERNAL)
        UKM_FAIL(UKM_ERR_INVALID, "ukm_setop2: unknown op %d", op);
    if (ta) cta = 0;
    if (tb) ctb = 0;
    const bool tax = (ta != nullptr) || (tb != nullptr) || cta != 0 || ctb != 0;
    if (tax && !tout) UKM_FAIL(UKM_ERR_INVALID, "ukm_setop2: taxids given but out_taxids is NULL");
    const bool need_lca = tax && op != UKM_OP_MERGE_INTERNAL && (op != UKM_OP_DIFF || (flags & UKM_F_CMP_TAXID));
    if (need_lca && c->tax_parent == nullptr)
        UKM_FAIL(UKM_ERR_NO_TAXONOMY, "ukm_setop2: records carry taxids but no taxonomy is loaded");
    *n_out = 0;
    if (na + nb == 0) return UKM_OK;
    if (na + nb >= (1ull << 61)) UKM_FAIL(UKM_ERR_INVALID, "ukm_setop2: input too large");

    // (the partition cache serves this first pass alone: the re-runs below work on arena copies or with ranks)
    const bool may_cache = (flags & UKM_F_INTERNAL_PART_CACHE) != 0 && op != UKM_OP_MERGE_INTERNAL;
    flags &= ~UKM_F_INTERNAL_PART_CACHE;
    u64 res[2] = {0, 0};
    UKM_TRY(run_setop_pass(c, op, a, ta, nullptr, na, b, tb, nullptr, nb, tax, flags, out, tout,
                           out_cap, res, cta, ctb, may_cache));
    if (res[1] & FLAG_UNSORTED) UKM_FAIL(UKM_ERR_UNSORTED, "ukm_setop2: an input stream is not sorted");
    if ((res[1] & FLAG_DUP) && op != UKM_OP_MERGE_INTERNAL) {
        // multiset inputs: redo with the exact reference semantics
        if (op == UKM_OP_UNION) {
            // union is a set: fold duplicates (LCA) inside each input first, then merge
            u64 *ua = nullptr, *ub = nullptr;
            u32 *uta = nullptr, *utb = nullptr;
            u64 nua = 0, nub = 0;
            UKM_TRY(ws_alloc_t(c, na + 1, &ua));
            UKM_TRY(ws_alloc_t(c, nb + 1, &ub));
            if (ta) UKM_TRY(ws_alloc_t(c, na + 1, &uta));
            if (tb) UKM_TRY(ws_alloc_t(c, nb + 1, &utb));
            // (a stream with one taxid per file keeps it: LCA(x, x) = x)
            UKM_TRY(ukm_dev_unique(c, a, ta, na, UKM_UNIQUE, ua, uta, na, &nua));
            UKM_TRY(ukm_dev_unique(c, b, tb, nb, UKM_UNIQUE, ub, utb, nb, &nub));
            UKM_TRY(run_setop_pass(c, op, ua, uta, nullptr, nua, ub, utb, nullptr, nub, tax, flags,
                                   out, tout, out_cap, res, cta, ctb));
        } else {
            u32 *ra = nullptr, *rb = nullptr;
            UKM_TRY(ws_alloc_t(c, na + 1, &ra));
            UKM_TRY(ws_alloc_t(c, nb + 1, &rb));
            if (na) hipLaunchKernelGGL(rank_in_run_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, c->stream, a, na, ra);
            if (nb) hipLaunchKernelGGL(rank_in_run_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, c->stream, b, nb, rb);
            if (op == UKM_OP_DIFF && !(flags & UKM_F_INTERNAL_KEEP_DUPS)) {
                // the reference's survivor map collapses duplicate codes (diff.go:449-453);
                // the last record of a run wins.  (ONE later file: the n-file fold keeps the running list as it is between
                // its files -- mc1 = mc2, diff.go:437 -- and collapses once at the end: UKM_F_INTERNAL_KEEP_DUPS)
                u64 *tk = nullptr;
                u32 *tt = nullptr;
                UKM_TRY(ws_alloc_t(c, na + 1, &tk));
                if (tax) UKM_TRY(ws_alloc_t(c, na + 1, &tt));
                UKM_TRY(run_setop_pass(c, op, a, ta, ra, na, b, tb, rb, nb, tax, flags, tk, tt, na, res, cta, ctb));
                if (!(res[1] & FLAG_UNSORTED)) {
                    u64 nu = 0;
                    const int ru = ukm_dev_unique(c, tk, tax ? tt : nullptr, res[0], 5 /*UNIQUE_LAST*/, out, tout, out_cap, &nu);
                    if (ru == UKM_ERR_CAPACITY) *n_out = nu;  // (the size needed leaves with the error, as below)
                    UKM_TRY(ru);
                    res[0] = nu;
                }
            } else {
                UKM_TRY(run_setop_pass(c, op, a, ta, ra, na, b, tb, rb, nb, tax, flags, out, tout,
                                       out_cap, res, cta, ctb));
            }
        }
        if (res[1] & FLAG_UNSORTED) UKM_FAIL(UKM_ERR_UNSORTED, "ukm_setop2: an input stream is not sorted");
    }
    *n_out = res[0];
    if (res[0] > out_cap)
        UKM_FAIL(UKM_ERR_CAPACITY, "ukm_setop2: output needs %llu records, capacity is %llu",
                 (unsigned long long)res[0], (unsigned long long)out_cap);
    // the caller wants taxids but neither stream carries any (two files without taxid information inside an n-file
    // operation whose other files have some; the only stream with taxids is empty): such records have taxid 0
    if (!tax && tout && res[0]) UKM_HIP(hipMemsetAsync(tout, 0, res[0] * sizeof(u32), c->stream));
    return UKM_OK;
}

// ---- the C ABI.  What ukm_setop2_ft and ukm_setop2_multi do alike with their arguments: ----
namespace {

// the staged inputs of one pair, and what follows from them
struct Setop2In {
    const u64 *a = nullptr, *b = nullptr;
    const u32 *ta = nullptr, *tb = nullptr;
    bool tax_in = false;  // the call carries taxids of either kind
    u32 cta = 0, ctb = 0;
    u32 flags = 0;  // the caller's taxid flags | UKM_F_INTERNAL_PART_CACHE where the call may use the partition cache
};
int setop2_stage_in(ukm_ctx *ctx, const CallScope &s, const uint64_t *a_keys, const uint32_t *a_taxids, uint32_t a_file_taxid, uint64_t na,
                    const uint64_t *b_keys, const uint32_t *b_taxids, uint32_t b_file_taxid, uint64_t nb, uint32_t flags, Setop2In *in) {
    UKM_TRY(ukm_in_t(ctx, a_keys, na, &in->a));
    UKM_TRY(ukm_in_t(ctx, b_keys, nb, &in->b));
    UKM_TRY(ukm_in_t(ctx, a_taxids, na, &in->ta));
    UKM_TRY(ukm_in_t(ctx, b_taxids, nb, &in->tb));
    in->tax_in = a_taxids || b_taxids || a_file_taxid || b_file_taxid;
    // (an empty stream's per-record pointer may be null: its file taxid plays no part then)
    in->cta = in->ta ? 0u : a_file_taxid;
    in->ctb = in->tb ? 0u : b_file_taxid;
    // both key streams are the caller's device memory (ukm_in_t hands a device pointer back as it is; a host array
    // becomes an arena copy, whose address the next call reuses with other data): the call may use the partition cache
    // (ukm_setop2_multi: its split route's passes; the fused pass never does)
    const u32 cacheable = (s.top && na && nb && in->a == a_keys && in->b == b_keys) ? UKM_F_INTERNAL_PART_CACHE : 0u;
    in->flags = (flags & (UKM_F_MIX_TAXID | UKM_F_CMP_TAXID)) | cacheable;
    return UKM_OK;
}
// one output: (a size query, out_cap == 0, may leave both arrays NULL; without taxids out_taxids stays optional)
int setop2_stage_out(ukm_ctx *ctx, bool tax_in, uint64_t *out_keys, uint32_t *out_taxids, uint64_t out_cap, u64 **out, u32 **tout) {
    UKM_TRY(ukm_out_query_t(ctx, out_keys, out_cap, out));
    if (tax_in) UKM_TRY(ukm_out_query_t(ctx, out_taxids, out_cap, tout));
    else UKM_TRY(ukm_out_t(ctx, out_taxids, out_cap, tout));
    return UKM_OK;
}
// ... and its n records on the way out (an error: none)
void setop2_resize_out(ukm_ctx *ctx, uint64_t *out_keys, uint32_t *out_taxids, u64 n) {
    ukm_out_resize(ctx, out_keys, n * sizeof(u64));
    if (out_taxids) ukm_out_resize(ctx, out_taxids, n * sizeof(u32));
}

}  // namespace

extern "C" int ukm_setop2_ft(ukm_ctx *ctx, int op, const uint64_t *a_keys, const uint32_t *a_taxids, uint32_t a_file_taxid,
                             uint64_t na, const uint64_t *b_keys, const uint32_t *b_taxids, uint32_t b_file_taxid,
                             uint64_t nb, uint32_t flags, uint64_t *out_keys, uint32_t *out_taxids,
                             uint64_t out_cap, uint64_t *n_out) {
    if (!ctx || !n_out || (!a_keys && na) || (!b_keys && nb) || (!out_keys && out_cap))
        UKM_FAIL(UKM_ERR_INVALID, "ukm_setop2: NULL argument");
    if (op != UKM_OP_UNION && op != UKM_OP_INTER && op != UKM_OP_DIFF)
        UKM_FAIL(UKM_ERR_INVALID, "ukm_setop2: unknown op %d", op);
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        Setop2In in;
        u64 *out = nullptr;
        u32 *tout = nullptr;
        UKM_TRY(setop2_stage_in(ctx, s, a_keys, a_taxids, a_file_taxid, na, b_keys, b_taxids, b_file_taxid, nb, flags, &in));
        UKM_TRY(setop2_stage_out(ctx, in.tax_in, out_keys, out_taxids, out_cap, &out, &tout));
        const int r = ukm_dev_setop2_ct(ctx, op, in.a, in.ta, in.cta, na, in.b, in.tb, in.ctb, nb, in.flags, out, tout, out_cap, n_out);
        setop2_resize_out(ctx, out_keys, out_taxids, (r == UKM_OK) ? *n_out : 0);
        return r;
    }();
    return ukm_finish(&s, rc);
}

extern "C" int ukm_setop2(ukm_ctx *ctx, int op, const uint64_t *a_keys, const uint32_t *a_taxids,
                          uint64_t na, const uint64_t *b_keys, const uint32_t *b_taxids,
                          uint64_t nb, uint32_t flags, uint64_t *out_keys, uint32_t *out_taxids,
                          uint64_t out_cap, uint64_t *n_out) {
    return ukm_setop2_ft(ctx, op, a_keys, a_taxids, 0u, na, b_keys, b_taxids, 0u, nb, flags, out_keys, out_taxids, out_cap, n_out);
}

extern "C" int ukm_setop2_multi(ukm_ctx *ctx, uint32_t ops, const uint64_t *a_keys, const uint32_t *a_taxids, uint32_t a_file_taxid,
                                uint64_t na, const uint64_t *b_keys, const uint32_t *b_taxids, uint32_t b_file_taxid, uint64_t nb,
                                uint32_t flags, uint64_t *const out_keys[3], uint32_t *const out_taxids[3], const uint64_t out_cap[3],
                                uint64_t n_out[3]) {
    if (!ctx || !n_out || !out_keys || !out_cap || (!a_keys && na) || (!b_keys && nb))
        UKM_FAIL(UKM_ERR_INVALID, "ukm_setop2_multi: NULL argument");
    if (ops == 0 || ops >= 8u) UKM_FAIL(UKM_ERR_INVALID, "ukm_setop2_multi: ops %u names no operation or an unknown one", ops);
    for (int x = 0; x < 3; x++)
        if (((ops >> x) & 1u) && !out_keys[x] && out_cap[x]) UKM_FAIL(UKM_ERR_INVALID, "ukm_setop2_multi: NULL argument");
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        Setop2In in;
        u64 *out[3] = {nullptr, nullptr, nullptr};
        u32 *tout[3] = {nullptr, nullptr, nullptr};
        u64 cap[3] = {0, 0, 0};
        UKM_TRY(setop2_stage_in(ctx, s, a_keys, a_taxids, a_file_taxid, na, b_keys, b_taxids, b_file_taxid, nb, flags, &in));
        for (int x = 0; x < 3; x++) {  // (entries of operations that were not requested are never looked at)
            if (!((ops >> x) & 1u)) continue;
            cap[x] = out_cap[x];
            UKM_TRY(setop2_stage_out(ctx, in.tax_in, out_keys[x], out_taxids ? out_taxids[x] : nullptr, cap[x], &out[x], &tout[x]));
        }
        u64 n[3] = {0, 0, 0};
        const int r = ukm_dev_setop2_multi(ctx, ops, in.a, in.ta, in.cta, na, in.b, in.tb, in.ctb, nb, in.flags, out, tout, cap, n);
        for (int x = 0; x < 3; x++) {
            if (!((ops >> x) & 1u)) continue;
            n_out[x] = n[x];
            setop2_resize_out(ctx, out_keys[x], out_taxids ? out_taxids[x] : nullptr, (r == UKM_OK) ? n[x] : 0);
        }
        return r;
    }();
    return ukm_finish(&s, rc);
}

extern "C" int ukm_partition_points(ukm_ctx *ctx, const uint64_t *keys, uint64_t n,
                                    const uint64_t *splitters, int n_split, uint64_t *cuts) {
    if (!ctx || (!keys && n) || !splitters || !cuts || n_split <= 0)
        UKM_FAIL(UKM_ERR_INVALID, "ukm_partition_points: bad argument");
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        const u64 *k = nullptr, *q = nullptr;
        u64 *o = nullptr;
        UKM_TRY(ukm_in_t(ctx, keys, n, &k));
        UKM_TRY(ukm_in_t(ctx, splitters, (u64)n_split, &q));
        UKM_TRY(ukm_out_t(ctx, cuts, (u64)n_split, &o));
        hipLaunchKernelGGL(lower_bound_kernel, dim3((n_split + 63) / 64), dim3(64), 0, ctx->stream, k, n, q, n_split, o);
        UKM_HIP(hipGetLastError());
        return UKM_OK;
    }();
    return ukm_finish(&s, rc);
}
