// ukm_setop_kernels.h — the kernels of the 2-way set operation and their launchers: the two-launch taxid epilogue, the tile
// kernel, the fused multi-operation kernel, the small kernels around them, and launch_variant, the one place where a
// named tile variant becomes template arguments.  Part of ukm_setops.hip's translation unit (included there, inside its
// anonymous namespace, behind ukm_setop_tile.h) and of nothing else.

// -DUKM_PROFILE_PHASES (tools/README.md): thread 0 of every workgroup adds up the cycles between the PH(i) marks of a tile
// kernel and leaves them in p.dbg[8 * block ...], [7] = 1; the host prints the means (setop_phases_report).  PH_BEGIN()
// stands behind the declaration of `tid`, PH_END(p) at the kernel's end.  All three are empty in the product build.
#ifdef UKM_PROFILE_PHASES
#define PH_BEGIN() u64 ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}; u64 tlast = clock64()
#define PH(i) do { if (tid == 0) { u64 _t = clock64(); ph[i] += _t - tlast; tlast = _t; } } while (0)
#define PH_END(p) do { if (tid == 0 && (p).dbg) { for (int i = 0; i < 7; i++) (p).dbg[blockIdx.x * 8 + i] = ph[i]; (p).dbg[blockIdx.x * 8 + 7] = 1; } } while (0)
#else
#define PH_BEGIN() do {} while (0)
#define PH(i) do {} while (0)
#define PH_END(p) do {} while (0)
#endif

// ---- per-record taxids on plain sets, in two launches (round 5) ---------------------------------------------------------
// The taxid instantiation carries the taxids through the merge: 13 items per thread instead of 19, 80 KB of LDS, no LDS-DMA,
// 128 registers with spills, and the LCA of a matched pair -- two dependent table reads -- inside a thread's SERIAL merge
// loop: 132 vector and 85 scalar lane-instructions per record against 67 / 22 for plain codes (profiles/r05_setop_tax_pmc.txt).
// Which input an output record came from does not depend on any taxid (union, inter, diff without -t, the keep-everything
// merge), so: launch 1 = the PLAIN-key kernel, whose epilogue writes one SOURCE WORD per output record where its taxid will
// stand ([13:0] the record's place in the tile's A range, [27:14] in its B range, [28] a matched pair, [29] taken from
// B; put together from the two bit masks of the thread's steps: ~10 instructions per step); launch 2 = one workgroup per
// tile turns the words into taxids IN PLACE: a thread per output record, every taxid read and every LCA independent of
// every other -- the table reads of a whole tile are in flight together instead of one pair at a time per thread.
// 8 more bytes of HBM traffic per output record (the word written and read back).
constexpr u32 SRC_MATCH = 1u << 28, SRC_FROM_B = 1u << 29;
template <int OP, int NTH, int VT>
__device__ __forceinline__ void tile_flush_src(const SetopArgs &p, int tid, u64 base, u32 count, u32 excl, u32 mask, u32 amask,
                                               u32 mmask, int ia0, int ib0, u32 *s_t32) {
    static_assert(NTH * VT + 8 < (1 << 14), "a place in the tile takes 14 bits");
    __syncthreads();  // every thread has stored its share of the compacted codes
#pragma unroll
    for (int s = 0; s < VT; s++) {
        if (mask & (1u << s)) {
            const u32 below = (1u << s) - 1u;
            const int na_before = __popc(amask & below);
            const u32 ia = (u32)(ia0 + na_before), ib = (u32)(ib0 + s - na_before);
            const bool at = (amask >> s) & 1u, m = (mmask >> s) & 1u;
            s_t32[excl + (u32)__popc(mask & below)] = ia | (ib << 14) | (m ? SRC_MATCH : 0u) | (at ? 0u : SRC_FROM_B);
        }
    }
    __syncthreads();
    for (u32 i = (u32)tid; i < count; i += NTH)
        if (base + i < p.out_cap) p.tout[base + i] = s_t32[i];
}

constexpr int GATHER_NT = 256;
#ifndef GATHER_U
#define GATHER_U 8  /* records per thread and step (experiments: 2, 4, 8) */
#endif
template <int OP, int TILE>
__global__ __launch_bounds__(GATHER_NT) void setop_taxid_gather_kernel(SetopArgs p) {
    setop_resolve_sizes(p, (u64)TILE);
    const u64 tile = blockIdx.x;
    if (tile >= p.ntiles) return;
    if (setop_table_stale(p)) return;  // (no tile has run: the host partitions and launches again)
    if (sload_u64(&p.result[1]) & FLAG_TIMEOUT) return;  // (the host runs the pass again: the status words are incomplete)
    u64 base, end;
    if (OP == UKM_OP_MERGE_INTERNAL) {
        base = tile * (u64)TILE;
        end = base + TILE < p.na + p.nb ? base + TILE : p.na + p.nb;
    } else {
        base = tile ? (lb_load(&p.status[(tile - 1) * LB_STRIDE]) & LB_VAL) : 0ull;
        end = lb_load(&p.status[tile * LB_STRIDE]) & LB_VAL;
    }
    if (end > p.out_cap) end = p.out_cap;
    if (end <= base) return;
    const u64 a0 = p.mp[tile], b0 = tile * (u64)TILE - a0;
    const bool mix = (p.flags & UKM_F_MIX_TAXID) != 0;
    const u32 *safe32 = reinterpret_cast<const u32 *>(p.result);  // (always mapped: where a lane has nothing to read)
    constexpr bool LCA_OP = OP == UKM_OP_UNION || OP == UKM_OP_INTER;
    __shared__ CladeLdsOpt<LCA_OP> s_clade_tab;  // the clade-pair step out of LDS (ukm_device.h)
    const bool lds_pairs = LCA_OP && p.tax.cpath != nullptr;  // (uniform; every early return above is uniform too)
    if constexpr (LCA_OP) {
        clade_lds_load(p.tax, s_clade_tab.t, (int)threadIdx.x, GATHER_NT);
        __syncthreads();
    }
    // U records per thread and step: four rounds of loads -- the words, the taxids, the clade codes, the clade pairs -- each
    // round with all of its reads in flight, none inside a branch.  (Measured at 2 x 1e8, inter with one taxid per file as arrays:
    // 256 threads x 8 records 0.99 ms, x 4 1.06, x 2 1.13; a whole tile per 1024-thread workgroup in ONE step 1.22.)
    constexpr int U = GATHER_U;
    constexpr bool LCA = OP == UKM_OP_UNION || OP == UKM_OP_INTER;
    for (u64 i0 = base + threadIdx.x; i0 < end; i0 += (u64)GATHER_NT * U) {
        u32 w[U], va[U], vb[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u64 i = i0 + (u64)u * GATHER_NT;
            w[u] = p.tout[i < end ? i : base];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u32 ia = w[u] & 0x3FFFu, ib = (w[u] >> 14) & 0x3FFFu;
            // Every lane reads BOTH inputs' taxid at its place, needed or not: the places of neighbouring records are neighbours, so
            // the unneeded reads fall into lines the wave fetches anyway.  A place beyond its input (the B record behind the last
            // one; an unsorted input, whose result the host discards) is clamped into it.
            const u64 ga = a0 + ia, gb = b0 + ib;
            va[u] = p.cta;
            vb[u] = p.ctb;
            if (p.ta) va[u] = *(p.na ? p.ta + (ga < p.na ? ga : p.na - 1) : safe32);  // (uniform branches)
            if (p.tb) vb[u] = *(p.nb ? p.tb + (gb < p.nb ? gb : p.nb - 1) : safe32);
        }
        u32 quick[U];
        u32 qmask = 0;
        if (LCA && p.tax.pair != nullptr && p.tax.clade8 != nullptr) {  // (uniform)
            u32 ca[U], cb[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const bool look = (w[u] & SRC_MATCH) != 0 && va[u] != vb[u] && va[u] != 0 && vb[u] != 0 && va[u] < p.tax.size && vb[u] < p.tax.size;
                ca[u] = p.tax.clade8[look ? va[u] : 0u];
                cb[u] = p.tax.clade8[look ? vb[u] : 0u];
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const bool q = ca[u] != cb[u] && ca[u] != 0 && cb[u] != 0;
                qmask |= q ? (1u << u) : 0u;
                if constexpr (LCA_OP) {
                    if (lds_pairs) quick[u] = q ? lca_clade_pair_lds(p.tax, s_clade_tab.t, ca[u], cb[u]) : 0u;
                    else quick[u] = p.tax.pair[q ? ca[u] * p.tax.kp + cb[u] : 0u];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u64 i = i0 + (u64)u * GATHER_NT;
            if (i >= end) continue;
            const bool from_b = (w[u] & SRC_FROM_B) != 0, m = (w[u] & SRC_MATCH) != 0;
            u32 tv;
            if (LCA && m) {
                if (OP == UKM_OP_INTER && mix && (va[u] == 0 || vb[u] == 0)) tv = va[u] == 0 ? vb[u] : va[u];
                else if ((qmask >> u) & 1u) tv = quick[u];
                else tv = lca_dev(p.tax, va[u], vb[u]);  // relatives, zero / unknown / merged ids, no clade tables
            } else {
                tv = from_b ? vb[u] : va[u];
            }
            p.tout[i] = tv;
        }
    }
}

// the pairs the DEFER tiles left behind (SetopArgs::fix): one thread per place of the list
__global__ __launch_bounds__(256) void setop_taxid_fix_kernel(SetopArgs p) {
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 tile = g / FIX_SLOTS;
    if (tile >= p.ntiles) return;
    if (setop_table_stale(p)) return;  // (no tile has run: nobody has written fix_cnt)
    if (sload_u64(&p.result[1]) & FLAG_TIMEOUT) return;  // (the host runs the pass again: not every tile has written its count)
    if ((u32)(g % FIX_SLOTS) >= p.fix_cnt[tile]) return;
    const uint4 e = p.fix[g];
    const u64 pos = ((u64)e.y << 32) | e.x;
    // (a != b, both non-zero, not settled by their clade codes: straight to the root paths, as the tile would have gone)
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    const TaxDev &T = p.tax;
    if (pos < p.out_cap) p.tout[pos] = lca_from_rows(T, e.z, e.w, e.z < T.size ? T.anc[e.z] : zero4, e.w < T.size ? T.anc[e.w] : zero4);
}

// result[4] of a CT call: [31:0] the taxid of a matched pair (inter --mix-taxid: a zero on either side yields the other,
// inter.go:229-236), [32] diff -t keeps matched codes (diff.go:404-409: the later file's taxid equals the first file's or
// lies below it).  One thread; runs between the partition launch (which clears the control words) and the tile kernel.
__global__ void setop_ct_kernel(SetopArgs p, int op) {
    const u32 a = p.cta, b = p.ctb;
    u32 l;
    if (op == UKM_OP_INTER && (p.flags & UKM_F_MIX_TAXID)) l = a == 0 ? b : (b == 0 ? a : lca_dev(p.tax, a, b));
    else l = lca_dev(p.tax, a, b);
    const bool keep = op == UKM_OP_DIFF && (p.flags & UKM_F_CMP_TAXID) && (a == b || lca_dev(p.tax, b, a) == a);
    p.result[4] = (u64)l | ((u64)(keep ? 1u : 0u) << 32);
}

// ---- the tile kernel: one workgroup per tile of NTH*VT merged items ------------------------------------
// TICKET = false (default): tile id = blockIdx.x, so the partition words are fetched with scalar
//   loads at kernel entry and no atomic sits in front of the tile loads (measured -0.7 ms of
//   7.4 ms).  Look-back then relies on the hardware dispatching workgroups in increasing
//   order (observed on MI355X; each XCD's dispatcher walks its share of the grid in order), so
//   every predecessor of a running tile is running or done.  Results never depend on that: if
//   a predecessor fails to publish within LB_SPIN_LIMIT polls the kernel raises FLAG_TIMEOUT
//   and the host re-runs with TICKET = true, where tile ids come from an atomic counter and
//   forward progress holds for any dispatch order.
// TABLE = true (plain keys, union / inter / diff): the tiles' output offsets are known before the launch (p.base, see
//   setop_partition_verify_kernel).  No ticket, nothing published, nobody waited for: the tiles are independent of each
//   other.  A tile whose count differs from its step of the table raises FLAG_OFFS and stores no more than the step.
//   Tile id = ukm_setop_order::tile_of(blockIdx.x) when p.xcd_order is set: each XCD runs a range of consecutive tiles, so
//   neighbouring tiles share an L2 (the lines their ranges begin and end in; mp[] and base[]).  ONLY this form may: under
//   a look-back a chunk's first tile would wait for the last tile of the chunk in front of it, which starts a whole
//   chunk of dispatches later -- every look-back form keeps blockIdx.x or tickets, and so does setop_multi_tile_kernel.
// UKM_OP_MERGE_INTERNAL (ukm_internal.h): plain 2-way MERGE of two non-decreasing streams, every record
//   kept (A first on ties).  Output size is known (|A| + |B|), so the tile kernel needs no look-back for it.
// Up to 80 KB of LDS per workgroup (plain keys; taxids OR ranks riding along): two 512-thread workgroups per CU = 4
// waves per SIMD, so the register budget is 128 and the allocator is told so (by itself it budgets 256 for a
// 512-thread workgroup: the plain kernel came out at 129 with its two load paths, the union with taxids at 131 once
// the LCA grew -- one workgroup per CU, union with taxids 1.45 -> 1.92 ms).  Taxids AND ranks (106 KB of LDS, one
// workgroup per CU anyway) keep the default budget.
#ifndef SETOP_WAVES
#define SETOP_WAVES 4  /* experiments only: 6 = three workgroups per CU (needs SETOP_VT <= 12) */
#endif
#ifndef SETOP_WAVES_TAX
#define SETOP_WAVES_TAX 6  /* per-record taxids, no ranks: THREE workgroups per CU (SETOP_VT_TAX <= 7) */
#endif
template <int OP, bool TAX, bool RANK, bool TICKET, int NTH, int VT, bool CT = false, bool DEFER = false, bool TABLE = false>
__global__ __launch_bounds__(NTH) __attribute__((amdgpu_waves_per_eu((TAX && RANK) ? 2 : ((TAX && VT <= 8) ? SETOP_WAVES_TAX : SETOP_WAVES), (TAX && RANK) ? 8 : ((TAX && VT <= 8) ? SETOP_WAVES_TAX : SETOP_WAVES))))
void setop_tile_kernel(SetopArgs p) {
    static_assert(!(CT && TAX), "CT: no per-record taxids");
    static_assert(!TABLE || (!TAX && !RANK && !TICKET && !CT && !DEFER && OP != UKM_OP_MERGE_INTERNAL), "TABLE: plain keys only");
    constexpr int TILE = NTH * VT;
    constexpr int SLOTS = TILE + 8;
    constexpr int NP = TilePairs<NTH, VT>::NP;
    __shared__ __attribute__((aligned(16))) u64 s_keys[SLOTS];
    __shared__ __attribute__((aligned(16))) u32 s_tax[TAX ? SLOTS : 2];
    __shared__ __attribute__((aligned(16))) u32 s_rank[RANK ? SLOTS : 2];
    __shared__ u32 s_scan[NTH / 64 + 1];
    __shared__ u64 s_misc[2];
    __shared__ CladeLdsOpt<TAX> s_clade_tab;
    __shared__ FixLdsOpt<DEFER> s_fix;
    const int tid = (int)threadIdx.x;
    if constexpr (DEFER) {
        if (tid == 0) s_fix.t.n = 0;  // (read behind the barriers of the tile's staging)
    }
    PH_BEGIN();
    u64 tile;
    if constexpr (TABLE) tile = ukm_setop_order::tile_of(blockIdx.x, p.ntiles, p.xcd_order);  // (a block without a tile: >= p.ntiles)
    else tile = lb_tile_id<TICKET>(p.ticket, &s_misc[0]);
    PH(0);
    setop_resolve_sizes(p, (u64)TILE);
    // chained call: the launch covers the upper bound of |A|.  A cached partition that failed its verification: EVERY
    // workgroup of the launch leaves here -- nothing loaded, published or stored, nobody waits in a look-back.  (Nothing but
    // the return: a store on this way out, even one thread's, costs the plain instantiations 14 spilled registers;
    // setop_stale_report_kernel tells the host.)
    if (tile >= p.ntiles || setop_table_stale(p)) return;
    const TileGeom g = tile_geom<NTH, VT>(p, tile);
    u64 tbase = 0, tstep = 0;  // TABLE only: this tile's offset and its step of the table (scalar loads beside the mp words)
    if constexpr (TABLE) {
        tbase = sload_u64(p.base + tile);
        tstep = sload_u64(p.base + tile + 1) - tbase;
    }
    u32 bad = 0;
    bool fast = false;  // workgroup-uniform
#ifndef SETOP_NO_FAST
    if (!TAX && !RANK) fast = tile_is_fast<NTH, VT>(p, g);
#endif
    if (fast) {
        // interior tile of plain keys: LDS-DMA staging; its order check runs after the aggregate is published (below)
        tile_dma_fast<NTH, VT>(p, g, tid, s_keys);
        __syncthreads();  // hipcc puts the vmcnt(0) for the LDS-DMA in front of the barrier
        PH(1);
    } else {
        u64 rk[2 * NP];
        u32 rt[2 * NP], rr[2 * NP];
        tile_load<TAX, RANK, NTH, VT>(p, g, tid, rk, rt, rr);
        if constexpr (TAX) clade_lds_load(p.tax, s_clade_tab.t, tid, NTH);
        tile_to_lds<TAX, RANK, NTH, VT>(tid, rk, rt, rr, s_keys, s_tax, s_rank);
        __syncthreads();
        PH(1);
        bad = tile_check_order<RANK, NTH, VT>(g, tid, rk, rr, s_keys, s_rank);
    }
    u64 ok[VT];
    u32 ot[VT];
    u32 tbm[VT];  // DEFER only: B's taxid of every step, `need` = the steps that wait for an LCA
    u32 need = 0, nneed = 0, qpos = 0;
    u32 mask, amask = 0, mmask = 0;
    int ia0 = 0, ib0 = 0;
    u32 ct_lca = 0;
    bool ct_keep = false;
    if (CT) {  // (written by setop_ct_kernel in front of this launch: a scalar load)
        const u64 w = sload_u64(&p.result[4]);
        ct_lca = (u32)w;
        ct_keep = ((w >> 32) & 1ull) != 0;
    }
#ifdef SETOP_ABL_NOMERGE  // experiment only: timing without the search + serial merge
    mask = 0xAAAAu | (u32)(tid & 1);
#pragma unroll
    for (int s = 0; s < VT; s++) { ok[s] = s_keys[tid * VT + s]; ot[s] = 0; }
#else
    tile_merge<OP, TAX, RANK, CT, NTH, VT, DEFER>(p, g, tid, s_keys, s_tax, s_rank, ok, ot, mask, amask, mmask, ct_keep, ia0, ib0,
                                           TAX ? reinterpret_cast<const CladeLds *>(&s_clade_tab.t) : nullptr, tbm, need);
#endif
    PH(2);
    u32 tile_total;
    // The block scan, opened up: the tile's aggregate is known (and published) behind its FIRST barrier; the order
    // check of an interior tile's inputs -- which nothing downstream needs -- runs between the two barriers, i.e.
    // AFTER the publication instead of in front of the merge.  Successors see the aggregate ~1 k cycles earlier
    // relative to this tile's own look-back, which is what their look-back waits for (round 3: union 5.0 -> 4.8 ms,
    // inter 4.15 -> 4.0 ms at 2 x 1e9).  Unsorted input only makes the merge emit garbage that the flag voids.
    u32 excl;
    {
        constexpr int NW = NTH / 64;
        // (DEFER: the queue positions ride in the upper half of the same scan; both sums stay below 2^16)
        const u32 v = (u32)__popc(mask) | (DEFER ? (u32)__popc(need) << 16 : 0u);
        const int lane = lane_id(), wave = tid >> 6;
        const u32 incl = wave_incl_scan_u32(v);
        if (lane == 63) s_scan[wave] = incl;
        __syncthreads();
        u32 wbase = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            const u32 t = s_scan[w];
            if (w < wave) wbase += t;
            tot += t;
        }
        tile_total = tot;
        excl = wbase + incl - v;
        if (DEFER) {
            static_assert(!DEFER || NTH * VT + 8 < (1 << 16), "two 16-bit sums in one word");
            nneed = tot >> 16;
            qpos = excl >> 16;
            tile_total = tot & 0xFFFFu;
            excl &= 0xFFFFu;
        }
        if (!TABLE && OP != UKM_OP_MERGE_INTERNAL && tid == 0) lb_publish(p.status, tile, (u64)tile_total);
        if (fast) bad |= tile_check_order_lds<NTH, VT>(g, tid, s_keys);
        __syncthreads();  // every thread has finished reading the tile from LDS; s_scan may be reused
    }
#ifndef SETOP_ABL_NOCOMPACT
    tile_compact<TAX, VT>(excl, mask, ok, ot, s_keys, s_tax);
#endif
    if constexpr (DEFER) {
        // the LCAs, dense: the queue lies behind the compacted records (a match leaves one place free in a union's tile
        // -- its B record is dropped, here or as the next tile's first step -- and more in an intersection's)
        tile_queue_lca<VT>(excl, mask, need, qpos, tbm, s_keys + tile_total);
        __syncthreads();
        tile_lca_dense<NTH>(p.tax, s_clade_tab.t, tid, nneed, s_keys + tile_total, s_tax, p.fix ? &s_fix.t : nullptr);
    }
    PH(3);
    if (OP == UKM_OP_MERGE_INTERNAL) {
        if (tid == 0) s_misc[1] = tile * (u64)TILE;  // every record is kept: the tile's output offset is known
    } else if (TABLE) {
        if ((u64)tile_total != tstep) bad |= FLAG_OFFS;  // (workgroup-uniform)
    } else if (tid < 64) {
        bool timed_out = false;
#ifdef LB_PRE_SLEEP
        __builtin_amdgcn_s_sleep(LB_PRE_SLEEP);
#endif
#ifdef SETOP_ABL_NOLB  // experiment only: wrong output positions, no look-back
        const u64 base = tile * (u64)TILE;
#else
        const u64 base = lb_resolve(p.status, tile, (u64)tile_total, lane_id(), TICKET ? nullptr : &timed_out);
#endif
        if (tid == 0) s_misc[1] = base;
        if (timed_out) bad |= FLAG_TIMEOUT;
    }
    PH(4);
    if (OP == UKM_OP_MERGE_INTERNAL) bad &= ~FLAG_DUP;  // duplicates are legal in a plain merge
    {
        // one atomic per wave at most (a stream full of duplicates would otherwise send one per thread
        // to the same word)
        u32 wbad = 0;
#pragma unroll
        for (u32 f = 1; f <= (TABLE ? FLAG_OFFS : FLAG_TIMEOUT); f <<= 1)
            if (__ballot((bad & f) != 0)) wbad |= f;
        if (wbad && lane_id() == 0) atomicOr((unsigned long long *)&p.result[1], (unsigned long long)wbad);
    }
    __syncthreads();
    u64 base;
    if constexpr (TABLE) {
        base = tbase;
        // (a step that does not fit the tile's count, a "negative" one included: what is stored stays inside both)
        if (tstep < (u64)tile_total) tile_total = (u32)tstep;
    } else {
        base = s_misc[1];
    }
    if constexpr (DEFER) {
        if (p.fix) {  // (uniform) the pairs left to setop_taxid_fix_kernel, at their output positions
            const u32 nf = s_fix.t.n < FIX_SLOTS ? s_fix.t.n : FIX_SLOTS;
            if ((u32)tid < nf) {
                const u64 pos = base + s_fix.t.w[tid];
                p.fix[tile * FIX_SLOTS + (u32)tid] = make_uint4((u32)pos, (u32)(pos >> 32), s_fix.t.a[tid], s_fix.t.b[tid]);
            }
            if (tid == 0) p.fix_cnt[tile] = nf;
        }
    }
#ifndef SETOP_ABL_NOFLUSH
    tile_flush<TAX, NTH>(p, tid, base, tile_total, s_keys, s_tax);
    if (CT) {
        if (p.ta != nullptr || p.tb != nullptr)  // (uniform) per-record taxids on a stream: source words now, setop_taxid_gather_kernel next
            tile_flush_src<OP, NTH, VT>(p, tid, base, tile_total, excl, mask, amask, mmask, ia0, ib0, reinterpret_cast<u32 *>(s_keys));
        else
            tile_flush_ct<OP, NTH, VT>(p, tid, base, tile_total, excl, mask, amask, mmask, ct_lca, reinterpret_cast<u32 *>(s_keys));
    }
#endif
    if (tid == 0 && tile == p.ntiles - 1) p.result[0] = TABLE ? tbase + tstep : base + tile_total;  // (TABLE: base[ntiles])
    PH(5);
    PH_END(p);
}

// ---- two or three operations of one pair from ONE merge (ukm_setop2_multi) ----------------------
// Plain codes only.  The union's merge with CT masks decides everything: `mask` = the union's records, `mmask` = the
// intersection's (a matched pair, at its A step), `amask & ~mmask` = the difference's.  The tiles publish their MATCH count
// and one look-back over it places all outputs (setop_offset_of): inter at MP, diff at a_t - MP, union at d_t - MP + s_t.
// Two compaction rounds through the tile's LDS image: the union's survivors, flushed; then inter's at [0, m) and diff's
// behind them -- disjoint subsets of the tile's A records, so they fit where the union's have just left.
// OPS = 1 << UKM_OP_x of every requested operation, at least two.  out / cap are indexed by UKM_OP_x.
struct SetopMultiOut {
    u64 *out[3];
    u64 cap[3];
};
template <int OPS, bool TICKET, int NTH, int VT>
__global__ __launch_bounds__(NTH) __attribute__((amdgpu_waves_per_eu(SETOP_WAVES, SETOP_WAVES)))
void setop_multi_tile_kernel(SetopArgs p, SetopMultiOut mo) {
    constexpr bool WU = (OPS >> UKM_OP_UNION) & 1, WI = (OPS >> UKM_OP_INTER) & 1, WD = (OPS >> UKM_OP_DIFF) & 1;
    static_assert(OPS > 0 && OPS < 8 && (int)WU + (int)WI + (int)WD >= 2, "two or three of union / inter / diff");
    static_assert(NTH * VT + 8 < (1 << 16), "two 16-bit sums in one word");
    constexpr int TILE = NTH * VT;
    constexpr int SLOTS = TILE + 8;
    constexpr int NP = TilePairs<NTH, VT>::NP;
    constexpr int NW = NTH / 64;
    __shared__ __attribute__((aligned(16))) u64 s_keys[SLOTS];
    __shared__ u32 s_scan[NW + 1];
    __shared__ u32 s_scan_d[NW + 1];
    __shared__ u64 s_misc[3];
    const int tid = (int)threadIdx.x;
    PH_BEGIN();
    u64 tile = lb_tile_id<TICKET>(p.ticket, &s_misc[0]);
    // (a ticket comes out of LDS, i.e. in a vector register, and the tile's whole geometry with it: said to be uniform --
    //  and 32 bits wide, as the counter is -- it stays in scalar registers as the blockIdx form's does; the ticketed form
    //  spilled 19 to 23 registers without this)
    if (TICKET) tile = (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)tile);
    PH(0);
    if (tile >= p.ntiles) return;
    const TileGeom g = tile_geom<NTH, VT>(p, tile);
    u32 bad = 0;
    const bool fast = tile_is_fast<NTH, VT>(p, g);  // workgroup-uniform
    if (fast) {
        tile_dma_fast<NTH, VT>(p, g, tid, s_keys);
        __syncthreads();
        PH(1);
    } else {
        u64 rk[2 * NP];
        u32 rt[2 * NP], rr[2 * NP];
        tile_load<false, false, NTH, VT>(p, g, tid, rk, rt, rr);
        tile_to_lds<false, false, NTH, VT>(tid, rk, rt, rr, s_keys, nullptr, nullptr);
        __syncthreads();
        PH(1);
        bad = tile_check_order<false, NTH, VT>(g, tid, rk, rr, s_keys, nullptr);
    }
    u64 ok[VT];
    u32 ot[VT], tbm[VT];  // (unused without taxids)
    u32 need = 0, mask, amask = 0, mmask = 0;
    int ia0 = 0, ib0 = 0;
    tile_merge<UKM_OP_UNION, false, false, true, NTH, VT, false>(p, g, tid, s_keys, nullptr, nullptr, ok, ot, mask, amask, mmask, false,
                                                                 ia0, ib0, nullptr, tbm, need);
    const u32 dmask = amask & ~mmask;
    PH(2);
    // The block scan of setop_tile_kernel with the match count riding in the upper half of the union's word; the
    // difference's count, where it is asked for, in a scan of its own behind the same barrier.  The
    // MATCH count is what the tile publishes, behind the first barrier; an interior tile's order check runs after that.
    u32 utot, mtot, dtot = 0, uexcl, mexcl, dexcl = 0, strad = 0;
    {
        const u32 v = (WU ? (u32)__popc(mask) : 0u) | ((u32)__popc(mmask) << 16);
        const u32 vd = (u32)__popc(dmask);
        const int lane = lane_id(), wave = tid >> 6;
        const u32 incl = wave_incl_scan_u32(v);
        u32 incl_d = 0;
        if (WD) incl_d = wave_incl_scan_u32(vd);
        if (lane == 63) {
            s_scan[wave] = incl;
            if (WD) s_scan_d[wave] = incl_d;
        }
        __syncthreads();
        u32 wbase = 0, tot = 0, wbase_d = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            const u32 t = s_scan[w];
            if (w < wave) wbase += t;
            tot += t;
            if (WD) {
                const u32 td = s_scan_d[w];
                if (w < wave) wbase_d += td;
                dtot += td;
            }
        }
        const u32 excl = wbase + incl - v;
        utot = tot & 0xFFFFu;
        mtot = tot >> 16;
        uexcl = excl & 0xFFFFu;
        mexcl = excl >> 16;
        if (WD) dexcl = wbase_d + incl_d - vd;
        if (tid == 0) lb_publish(p.status, tile, (u64)mtot);
        // s_t: a matched pair straddles the tile's front boundary (A[a0 - 1] == B[b0]; B[b0] is the next-B halo of a tile
        // without B records) -- read by the look-back's wave before the image goes
        if (WU && tid < 64) {
            const bool pair = g.has_prev_a && (g.nb_t > 0 || g.has_next_b);
            strad = (pair && s_keys[g.base_a - 1] == s_keys[g.base_b]) ? 1u : 0u;
        }
        if (fast) bad |= tile_check_order_lds<NTH, VT>(g, tid, s_keys);
        __syncthreads();  // every thread has finished reading the tile from LDS
    }
    if (WU) tile_compact<false, VT>(uexcl, mask, ok, ot, s_keys, nullptr);
    PH(3);
    if (tid < 64) {
        bool timed_out = false;
        const u64 mp = lb_resolve(p.status, tile, (u64)mtot, lane_id(), TICKET ? nullptr : &timed_out);
        if (tid == 0) {
            // (disordered inputs can count more matches than A records: the flag voids the outputs, the clamp keeps the
            //  offsets below inside [0, d_t + 1] whatever was counted)
            s_misc[1] = mp < g.a0 ? mp : g.a0;
            s_misc[2] = strad;
        }
        if (timed_out) bad |= FLAG_TIMEOUT;
    }
    PH(4);
    {
        u32 wbad = 0;
#pragma unroll
        for (u32 f = 1; f <= FLAG_TIMEOUT; f <<= 1)
            if (__ballot((bad & f) != 0)) wbad |= f;
        if (wbad && lane_id() == 0) atomicOr((unsigned long long *)&p.result[1], (unsigned long long)wbad);
    }
    __syncthreads();
    const u64 m0 = s_misc[1];
    if (WU) {
        SetopArgs pu = p;
        pu.out = mo.out[UKM_OP_UNION];
        pu.out_cap = mo.cap[UKM_OP_UNION];
        tile_flush<false, NTH>(pu, tid, setop_offset_of(UKM_OP_UNION, m0, g.a0, tile * (u64)TILE, s_misc[2]), utot, s_keys, nullptr);
        __syncthreads();  // the union's survivors have left the image
    }
    const u32 dfrom = WI ? mtot : 0u;  // the difference's survivors lie behind the intersection's
    if (WI) tile_compact<false, VT>(mexcl, mmask, ok, ot, s_keys, nullptr);
    if (WD) tile_compact<false, VT>(dfrom + dexcl, dmask, ok, ot, s_keys, nullptr);
    __syncthreads();
    if (WI) {
        SetopArgs pi = p;
        pi.out = mo.out[UKM_OP_INTER];
        pi.out_cap = mo.cap[UKM_OP_INTER];
        tile_flush<false, NTH>(pi, tid, setop_offset_of(UKM_OP_INTER, m0, g.a0, 0, 0), mtot, s_keys, nullptr);
    }
    if (WD) {
        SetopArgs pd = p;
        pd.out = mo.out[UKM_OP_DIFF];
        pd.out_cap = mo.cap[UKM_OP_DIFF];
        tile_flush<false, NTH>(pd, tid, setop_offset_of(UKM_OP_DIFF, m0, g.a0, 0, 0), dtot, s_keys + dfrom, nullptr);
    }
    if (tid == 0 && tile == p.ntiles - 1) p.result[0] = m0 + mtot;  // M: the host derives the three totals
    PH(5);
    PH_END(p);
}

// rank of each element inside its run of equal codes (multiset path)
__global__ void rank_in_run_kernel(const u64 *k, u64 n, u32 *rank) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 key = k[i];
    u32 r = 0;
    while (r < 32 && i > r && k[i - r - 1] == key) r++;
    if (r == 32 && i > r && k[i - r - 1] == key) {  // long run: lower_bound
        u64 lo = 0, hi = i - 32;
        while (lo < hi) {
            u64 mid = (lo + hi) >> 1;
            if (k[mid] < key) lo = mid + 1; else hi = mid;
        }
        r = (u32)(i - lo);
    }
    rank[i] = r;
}

__global__ void lower_bound_kernel(const u64 *k, u64 n, const u64 *q, int nq, u64 *out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    u64 key = q[i], lo = 0, hi = n;
    while (lo < hi) {
        u64 mid = (lo + hi) >> 1;
        if (k[mid] < key) lo = mid + 1; else hi = mid;
    }
    out[i] = lo;
}

// behind the kernels of a launch that works on the cached table: the verdict of its verification, where the host reads the flags
__global__ void setop_stale_report_kernel(SetopArgs p) {
    if (setop_table_stale(p)) p.result[1] = FLAG_STALE;  // (no tile has run: there are no other flags)
}

template <int OP, bool TAX, bool RANK, int NTH, int VT, bool CT = false, bool DEFER = false>
void launch_tile(const SetopArgs &p, hipStream_t st, bool ticket) {
    if (CT) hipLaunchKernelGGL(setop_ct_kernel, dim3(1), dim3(1), 0, st, p, OP);
    if (ticket)
        hipLaunchKernelGGL((setop_tile_kernel<OP, TAX, RANK, true, NTH, VT, CT, DEFER>), dim3((unsigned)p.ntiles), dim3(NTH), 0, st, p);
    else
        hipLaunchKernelGGL((setop_tile_kernel<OP, TAX, RANK, false, NTH, VT, CT, DEFER>), dim3((unsigned)p.ntiles), dim3(NTH), 0, st, p);
    if constexpr (DEFER) {
        if (p.fix) hipLaunchKernelGGL(setop_taxid_fix_kernel, dim3((unsigned)((p.ntiles * FIX_SLOTS + 255) / 256)), dim3(256), 0, st, p);
    }
    if constexpr (CT && !RANK) {
        if (p.ta != nullptr || p.tb != nullptr)  // the source words of the launch above -> taxids
            hipLaunchKernelGGL((setop_taxid_gather_kernel<OP, NTH * VT>), dim3((unsigned)p.ntiles), dim3(GATHER_NT), 0, st, p);
    }
}

// the TABLE instantiations: plain keys, the three public operations
template <int NTH, int VT>
void launch_table(int op, const SetopArgs &p, hipStream_t st) {
    const dim3 grid((unsigned)ukm_setop_order::grid_of(p.ntiles, p.xcd_order)), block(NTH);
    if (op == UKM_OP_UNION) hipLaunchKernelGGL((setop_tile_kernel<UKM_OP_UNION, false, false, false, NTH, VT, false, false, true>), grid, block, 0, st, p);
    else if (op == UKM_OP_INTER) hipLaunchKernelGGL((setop_tile_kernel<UKM_OP_INTER, false, false, false, NTH, VT, false, false, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((setop_tile_kernel<UKM_OP_DIFF, false, false, false, NTH, VT, false, false, true>), grid, block, 0, st, p);
}

template <bool TAX, bool RANK, int NTH, int VT, bool CT = false, bool DEFER = false>
void launch_op(int op, const SetopArgs &p, hipStream_t st, bool ticket) {
    if (op == UKM_OP_UNION) launch_tile<UKM_OP_UNION, TAX, RANK, NTH, VT, CT, DEFER>(p, st, ticket);
    else if (op == UKM_OP_INTER) launch_tile<UKM_OP_INTER, TAX, RANK, NTH, VT, CT, DEFER>(p, st, ticket);
    else if (op == UKM_OP_MERGE_INTERNAL) {
        if constexpr (!RANK) launch_tile<UKM_OP_MERGE_INTERNAL, TAX, false, NTH, VT, CT>(p, st, ticket);
    } else launch_tile<UKM_OP_DIFF, TAX, RANK, NTH, VT, CT>(p, st, ticket);
}

#ifndef SETOP_NT
#define SETOP_NT 512
#endif
#ifndef SETOP_VT
#define SETOP_VT 19
#endif

constexpr int NTS = SETOP_NT;       // threads per workgroup (512: two workgroups per CU)
constexpr int VT_PLAIN = SETOP_VT;  // 19 items per thread: 76 KiB of keys in LDS per workgroup (2 x 78 KB fit the CU's 160 KB)
// With per-record taxids the tile is SMALL: 7 items per thread = 43 KB of tile + the 5 KB clade table, so that THREE
// workgroups share a CU (6 waves per SIMD at 75 registers).  A tile spends most of its time in round trips that depend on
// each other (loads, the clade bytes of its matches, look-back, flush); with two large tiles per CU neither HBM nor the
// address unit was busy.  2 x 3e8, random taxids: 12 items (two per CU) union 4.41 / inter 4.08 ms, 9: 4.55 / 4.22,
// 7 (three per CU): 3.94 / 3.66, 6: 4.08 / 3.81, 5 (four per CU, 8 waves per SIMD): 4.01 / 3.72.
#ifndef SETOP_VT_TAX
#define SETOP_VT_TAX 7
#endif
constexpr int VT_TAX = SETOP_VT_TAX;
constexpr int VT_RANK = 12;  // ranks ride along (the multiset re-run), with or without taxids

// ---- ukm_setop2_multi: the fused pass (setop_multi_tile_kernel) ----
#ifndef SETOP_VT_MULTI
#define SETOP_VT_MULTI SETOP_VT
#endif
constexpr int VT_MULTI = SETOP_VT_MULTI;  // items per thread of the fused kernel (its partition is its own: any tile size would do)

template <int OPS>
void launch_multi(const SetopArgs &p, const SetopMultiOut &mo, hipStream_t st, bool ticket) {
    const dim3 grid((unsigned)p.ntiles), block(NTS);
    if (ticket) hipLaunchKernelGGL((setop_multi_tile_kernel<OPS, true, NTS, VT_MULTI>), grid, block, 0, st, p, mo);
    else hipLaunchKernelGGL((setop_multi_tile_kernel<OPS, false, NTS, VT_MULTI>), grid, block, 0, st, p, mo);
}

// ---- the tile variant: which family of setop_tile_kernel instantiations a pass or a chained link launches ----
// Chosen by the host (ukm_setops.hip: choose_variant for a pass, ukm_dev_setop2_link for a link) and turned into template
// arguments by launch_variant alone.  (The TABLE instantiations are not a variant: they are the PLAIN variant's tiles under
// Plan::VERIFY_TABLE, launch_table_tiles.)
enum class Tiles {
    PLAIN,       // plain codes: LDS-DMA staging, VT_PLAIN items per thread
    CT,          // PLAIN + a taxid epilogue: one taxid per file on both sides (setop_ct_kernel in front), or per-record taxids
                 // as source words (setop_taxid_gather_kernel behind)
    TAX,         // per-record taxids through the merge, the LCAs inside the merge loop: the small tile, VT_TAX
    TAX_DEFER,   // ... union / inter: the LCAs dense behind the loop (tile_merge_loop_deferred); diff: as TAX
    TAX_STREAM,  // diff without -t: the taxids ride along, nothing is looked up: the tile of VT_RANK items
    RANK,        // the multiset re-run on (code, rank-in-run): VT_RANK
    RANK_CT,     // ... with one taxid per file on both sides
    RANK_TAX,    // ... with per-record taxids
};
struct Variant {
    Tiles tiles;
    bool fix;  // TAX_DEFER only: the tiles leave the pairs their clade codes do not settle to setop_taxid_fix_kernel (SetopArgs::fix)
    bool rank() const { return tiles == Tiles::RANK || tiles == Tiles::RANK_CT || tiles == Tiles::RANK_TAX; }
    int vt() const {
        if (tiles == Tiles::PLAIN || tiles == Tiles::CT) return VT_PLAIN;
        return (tiles == Tiles::TAX || tiles == Tiles::TAX_DEFER) ? VT_TAX : VT_RANK;
    }
    u64 tile_items() const { return (u64)NTS * vt(); }
};

void launch_table_tiles(int op, const SetopArgs &p, hipStream_t st) { launch_table<NTS, VT_PLAIN>(op, p, st); }

void launch_variant(const Variant &v, int op, const SetopArgs &p, hipStream_t st, bool ticket) {
    switch (v.tiles) {
    case Tiles::RANK_TAX: launch_op<true, true, NTS, VT_RANK>(op, p, st, ticket); break;
    case Tiles::RANK_CT: launch_op<false, true, NTS, VT_RANK, true>(op, p, st, ticket); break;
    case Tiles::RANK: launch_op<false, true, NTS, VT_RANK>(op, p, st, ticket); break;
    case Tiles::TAX_STREAM: launch_tile<UKM_OP_DIFF, true, false, NTS, VT_RANK>(p, st, ticket); break;  // (op is UKM_OP_DIFF)
    case Tiles::TAX_DEFER: launch_op<true, false, NTS, VT_TAX, false, true>(op, p, st, ticket); break;
    case Tiles::TAX: launch_op<true, false, NTS, VT_TAX>(op, p, st, ticket); break;
    case Tiles::CT: launch_op<false, false, NTS, VT_PLAIN, true>(op, p, st, ticket); break;
    case Tiles::PLAIN: launch_op<false, false, NTS, VT_PLAIN>(op, p, st, ticket); break;
    }
}

