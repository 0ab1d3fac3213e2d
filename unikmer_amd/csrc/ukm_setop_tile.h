// ukm_setop_tile.h — the device functions a tile of the 2-way set operation is put together from: geometry, staging (through
// registers, or LDS-DMA for interior tiles of plain codes), order check, the merge loops, the dense LCA walk, compaction and
// the flushes.  Part of ukm_setops.hip's translation unit (included there, inside its anonymous namespace, behind
// ukm_setop_part.h) and of nothing else.

// ---- tile building blocks (shared by the kernels of ukm_setop_kernels.h) -----------------------------
// Everything here is written branch-free on purpose: the first version of the merge step
// compiled to ~80 instructions (exec-mask juggling, phi copies, 64-bit selects) and the kernel
// was VALU/SALU-issue bound at 31 % of HBM peak.
struct TileGeom {
    u64 a0, b0;
    int na_t, nb_t;
    bool has_prev_a, has_prev_b, has_next_a, has_next_b;
    // LDS slots:  [sa0] prevA | A items [base_a, end_a) | [end_a] nextA | pad | [sb0] prevB |
    //             B items [base_b, end_b) | [end_b] nextB
    // sa0 / sb0 carry a one-slot parity offset so that an EVEN slot always holds an element
    // whose global address is 16-byte aligned: pairs of slots then move with one dwordx4 load,
    // one ds_write_b128 and (on the way out) one dwordx4 store.
    int sa0, base_a, end_a, sb0, base_b, end_b, split;  // split = first (even) slot of region B
};

template <int NTH, int VT>
__device__ __forceinline__ TileGeom tile_geom(const SetopArgs &p, u64 tile) {
    constexpr int TILE = NTH * VT;
    const u64 N = p.na + p.nb;
    const u64 d0 = tile * (u64)TILE;
    const u64 d1 = (d0 + TILE < N) ? d0 + TILE : N;
    const u64 a0 = p.mp[tile], a1 = p.mp[tile + 1];
    const u64 b0 = d0 - a0, b1 = d1 - a1;
    TileGeom g;
    g.a0 = a0; g.b0 = b0;
    g.na_t = (int)(a1 - a0); g.nb_t = (int)(b1 - b0);
    g.has_prev_a = a0 > 0; g.has_prev_b = b0 > 0;
    g.has_next_a = a1 < p.na; g.has_next_b = b1 < p.nb;
    // parity (in 8-byte units) of the address of a[a0 - 1] / b[b0 - 1]
    g.sa0 = (int)((((uintptr_t)p.a >> 3) + a0 + 1) & 1);
    g.base_a = g.sa0 + 1;
    g.end_a = g.base_a + g.na_t;
    g.split = (g.end_a + 2) & ~1;
    g.sb0 = g.split + (int)((((uintptr_t)p.b >> 3) + b0 + 1) & 1);
    g.base_b = g.sb0 + 1;
    g.end_b = g.base_b + g.nb_t;
    return g;
}

// pairs of LDS slots each thread moves: ceil((TILE + 8) / 2 / NTH)
template <int NTH, int VT> struct TilePairs { static constexpr int NP = ((NTH * VT + 8) / 2 + NTH - 1) / NTH; };

// Coalesced global loads of the tile (+halos) into registers, two slots per load; nothing is
// waited for here.
template <bool TAX, bool RANK, int NTH, int VT>
__device__ __forceinline__ void tile_load(const SetopArgs &p, const TileGeom &g, int tid,
                                          u64 (&rk)[2 * TilePairs<NTH, VT>::NP], u32 (&rt)[2 * TilePairs<NTH, VT>::NP],
                                          u32 (&rr)[2 * TilePairs<NTH, VT>::NP]) {
    constexpr int NP = TilePairs<NTH, VT>::NP;
    const int alo = g.sa0 + (g.has_prev_a ? 0 : 1), ahi = g.end_a + (g.has_next_a ? 1 : 0);
    const int blo = g.sb0 + (g.has_prev_b ? 0 : 1), bhi = g.end_b + (g.has_next_b ? 1 : 0);
    // slot s of region A is a[a0 - 1 + (s - sa0)]; slot s of region B is b[b0 - 1 + (s - sb0)]
    const u64 *pa = p.a + g.a0 - 1 - g.sa0;
    const u64 *pb = p.b + g.b0 - 1 - g.sb0;
    const u32 *pta = TAX && p.ta ? p.ta + g.a0 - 1 - g.sa0 : nullptr;
    const u32 *ptb = TAX && p.tb ? p.tb + g.b0 - 1 - g.sb0 : nullptr;
    const u32 *pra = RANK ? p.ra + g.a0 - 1 - g.sa0 : nullptr;
    const u32 *prb = RANK ? p.rb + g.b0 - 1 - g.sb0 : nullptr;
    // Every load below is UNCONDITIONAL (idle lanes read a harmless aligned word of the control
    // block): a branch around a load makes the compiler wait for the previous one at the join
    // (measured: vmcnt(0) in front of every dwordx4, kernel 30 % slower).
    const u64 *safe = p.result;  // 256-byte aligned, always mapped
    const u32 *safe32 = reinterpret_cast<const u32 *>(p.result);
#pragma unroll
    for (int j = 0; j < NP; j++) {
        const int s0 = 2 * (tid + j * NTH), s1 = s0 + 1;
        const bool in_a = s0 < g.split;
        const int lo = in_a ? alo : blo, hi = in_a ? ahi : bhi;
        const bool v0 = s0 >= lo && s0 < hi, v1 = s1 >= lo && s1 < hi;
        const bool both = v0 && v1;
        const u64 *src = in_a ? pa : pb;
        // (per-record taxids: the streams go past L2 with the non-temporal hint, in and out, so that the clade table stays in
        //  it -- union of 2 x 3e8 with random taxids 5.75 -> 5.03 ms, of which the stores are 0.5; the plain kernel, which
        //  gathers nothing, was slower with the hint: profiles/r01_notes.md)
        ulonglong2 q;
        if (TAX) {
            typedef u64 v2u64 __attribute__((ext_vector_type(2)));
            const v2u64 w = __builtin_nontemporal_load(reinterpret_cast<const v2u64 *>(both ? src + s0 : safe));
            q.x = w.x;
            q.y = w.y;
        } else {
            q = *reinterpret_cast<const ulonglong2 *>(both ? src + s0 : safe);  // aligned by construction
        }
        rk[2 * j] = q.x;      // slots without a real element keep whatever was read: they are
        rk[2 * j + 1] = q.y;  // never compared (order check and merge only touch real slots)
        u32 t0 = 0, t1 = 0, r0 = 0, r1 = 0;
        if (TAX) {
            const u32 *ts = in_a ? pta : ptb;
            const bool h0 = ts && v0, h1 = ts && v1;
            t0 = __builtin_nontemporal_load(h0 ? ts + s0 : safe32);
            t1 = __builtin_nontemporal_load(h1 ? ts + s1 : safe32);
            const u32 tc = in_a ? p.cta : p.ctb;  // a stream without per-record taxids carries its file's taxid (0: none, mix-taxid)
            t0 = ts ? t0 : tc;
            t1 = ts ? t1 : tc;
        }
        if (RANK) {
            const u32 *rs = in_a ? pra : prb;
            r0 = *(v0 ? rs + s0 : safe32);
            r1 = *(v1 ? rs + s1 : safe32);
        }
        rt[2 * j] = t0; rt[2 * j + 1] = t1;
        rr[2 * j] = r0; rr[2 * j + 1] = r1;
    }
    // the (at most four) pairs per tile with exactly one real element, at the region edges
#pragma unroll
    for (int j = 0; j < NP; j++) {
        const int s0 = 2 * (tid + j * NTH), s1 = s0 + 1;
        const bool in_a = s0 < g.split;
        const int lo = in_a ? alo : blo, hi = in_a ? ahi : bhi;
        const bool v0 = s0 >= lo && s0 < hi, v1 = s1 >= lo && s1 < hi;
        if (v0 != v1) {
            const u64 *src = in_a ? pa : pb;
            if (v0) rk[2 * j] = src[s0]; else rk[2 * j + 1] = src[s1];
        }
    }
}

template <bool TAX, bool RANK, int NTH, int VT>
__device__ __forceinline__ void tile_to_lds(int tid, const u64 (&rk)[2 * TilePairs<NTH, VT>::NP],
                                            const u32 (&rt)[2 * TilePairs<NTH, VT>::NP],
                                            const u32 (&rr)[2 * TilePairs<NTH, VT>::NP], u64 *s_keys, u32 *s_tax,
                                            u32 *s_rank) {
    constexpr int NP = TilePairs<NTH, VT>::NP;
    constexpr int SLOTS = NTH * VT + 8;
#pragma unroll
    for (int j = 0; j < NP; j++) {
        const int s0 = 2 * (tid + j * NTH);
        if (s0 < SLOTS) {
            *reinterpret_cast<ulonglong2 *>(s_keys + s0) = make_ulonglong2(rk[2 * j], rk[2 * j + 1]);
            if (TAX) *reinterpret_cast<uint2 *>(s_tax + s0) = make_uint2(rt[2 * j], rt[2 * j + 1]);
            if (RANK) *reinterpret_cast<uint2 *>(s_rank + s0) = make_uint2(rr[2 * j], rr[2 * j + 1]);
        }
    }
}

// Strict-order check of both inputs as one vector pass (call after the barrier that follows
// tile_to_lds).  A slot is compared with its predecessor only when both hold real elements of
// the same input; the in-pair comparison uses the registers, the cross-pair one a single LDS
// read.  Replaces two 64-bit compares per merge step.
template <bool RANK, int NTH, int VT>
__device__ __forceinline__ u32 tile_check_order(const TileGeom &g, int tid, const u64 (&rk)[2 * TilePairs<NTH, VT>::NP],
                                                const u32 (&rr)[2 * TilePairs<NTH, VT>::NP], const u64 *s_keys,
                                                const u32 *s_rank) {
    constexpr int NP = TilePairs<NTH, VT>::NP;
    const int alo = g.sa0 + (g.has_prev_a ? 0 : 1), ahi = g.end_a + (g.has_next_a ? 1 : 0);
    const int blo = g.sb0 + (g.has_prev_b ? 0 : 1), bhi = g.end_b + (g.has_next_b ? 1 : 0);
    u32 bad = 0;
#pragma unroll
    for (int j = 0; j < NP; j++) {
        const int s0 = 2 * (tid + j * NTH), s1 = s0 + 1;
        const bool in_a = s0 < g.split;
        const int lo = in_a ? alo : blo, hi = in_a ? ahi : bhi;
        // (s-1, s) is a real adjacent pair of one input iff lo < s < hi
        const bool c0 = s0 > lo && s0 < hi, c1 = s1 > lo && s1 < hi;
        const int ip = c0 ? s0 - 1 : 0;
        const u64 pk = s_keys[ip], k0 = rk[2 * j], k1 = rk[2 * j + 1];
        if (RANK) {
            const u32 pr = s_rank[ip], r0 = rr[2 * j], r1 = rr[2 * j + 1];
            bad |= (c0 & ((pk > k0) | ((pk == k0) & (pr >= r0)))) ? FLAG_UNSORTED : 0u;
            bad |= (c1 & ((k0 > k1) | ((k0 == k1) & (r0 >= r1)))) ? FLAG_UNSORTED : 0u;
        } else {
            bad |= ((c0 & (pk > k0)) | (c1 & (k0 > k1))) ? FLAG_UNSORTED : 0u;
            bad |= ((c0 & (pk == k0)) | (c1 & (k0 == k1))) ? FLAG_DUP : 0u;
        }
    }
    return bad;
}

// ---- fast load / order check for tiles well inside both inputs (plain keys only) ---------------------
// When a0 >= 2, a1 + 2 <= na, b0 >= 2 and b1 + 5 <= nb, every slot of region A [0, split) and of
// region B [split, SLOTS) can be filled from the input itself: the slots that are padding in the
// generic layout (slot 0 under odd parity, the gap in front of region B, the tail) then hold the
// real neighbours a[a0-2], a[a1+1], b[b0-2], b[b1+1 ...].  Each region is a run of adjacent input
// elements, so neither the loads nor the order check need per-slot validity logic (about 200 of
// the 1200 VALU instructions a wave spends on a tile).  A violation seen in an over-read element
// is a real violation of the input (the neighbouring tile reports it too).
template <int NTH, int VT>
__device__ __forceinline__ bool tile_is_fast(const SetopArgs &p, const TileGeom &g) {
    return g.na_t + g.nb_t == NTH * VT && g.a0 >= 2 && g.a0 + (u64)g.na_t + 2 <= p.na && g.b0 >= 2 &&
           g.b0 + (u64)g.nb_t + 5 <= p.nb;
}

// The same tile, global memory -> LDS without a register round trip (gfx950 LDS-DMA, `global_load_lds_dwordx4`): the
// LDS image is lane-linear (wave-uniform base + 16 bytes per lane), which is exactly the staging layout above; the
// source address is per lane.  Saves the 40 staging VGPRs and the ds_write_b128 pass of the tile.
// SETOP_DMA_NT: the cache policy of these loads (the `aux` operand of the builtin; on gfx950 bit 1 = nt, "non-temporal":
// the lines are the first to leave the caches).  0 = the default policy, 1 = nt.  An experiment switch like SETOP_WAVES:
// the measurements behind the default are in profiles/part_reuse_notes.md.
#ifndef SETOP_DMA_NT
#define SETOP_DMA_NT 0
#endif
template <int NTH, int VT>
__device__ __forceinline__ void tile_dma_fast(const SetopArgs &p, const TileGeom &g, int tid, u64 *s_keys) {
    constexpr int NP = TilePairs<NTH, VT>::NP;
    constexpr int AUX = SETOP_DMA_NT ? 2 : 0;
    constexpr int SLOTS = NTH * VT + 8;
    typedef __attribute__((address_space(3))) void lds_void;
    typedef __attribute__((address_space(1))) const void glb_void;
    const u64 *pa = p.a + g.a0 - 1 - g.sa0;  // slot s of region A is pa[s]
    const u64 *pb = p.b + g.b0 - 1 - g.sb0;  // slot s of region B is pb[s]
    const int wbase = __builtin_amdgcn_readfirstlane(tid & ~63);
#pragma unroll
    for (int j = 0; j < NP; j++) {
        const int s0 = 2 * (tid + j * NTH);
        const u64 *src = (s0 < g.split ? pa : pb) + s0;
        u64 *dst = s_keys + 2 * (wbase + j * NTH);  // wave-uniform; lane l lands 16 l bytes behind it
        if (2 * (NTH - 1 + j * NTH) + 1 >= SLOTS) {  // last round only (compile time): lanes beyond the tile stay off
            if (s0 < SLOTS) __builtin_amdgcn_global_load_lds((glb_void *)src, (lds_void *)dst, 16, 0, AUX);
        } else {
            __builtin_amdgcn_global_load_lds((glb_void *)src, (lds_void *)dst, 16, 0, AUX);
        }
    }
}

template <int NTH, int VT>
__device__ __forceinline__ u32 tile_check_order_lds(const TileGeom &g, int tid, const u64 *s_keys) {
    constexpr int NP = TilePairs<NTH, VT>::NP;
    constexpr int SLOTS = NTH * VT + 8;
    bool unsorted = false, dup = false;
#pragma unroll
    for (int j = 0; j < NP; j++) {
        const int s0 = 2 * (tid + j * NTH);
        bool c0 = (s0 != 0) & (s0 != g.split), c1 = true;  // slot s0 - 1 belongs to the same region
        if (2 * (NTH - 1 + j * NTH) + 1 >= SLOTS) { c1 = s0 < SLOTS; c0 &= c1; }
        const int sr = c1 ? s0 : 0;
        const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(s_keys + sr);
        const u64 pk = s_keys[sr > 0 ? sr - 1 : 0], k0 = q.x, k1 = q.y;
        unsorted |= (c0 & (pk > k0)) | (c1 & (k0 > k1));
        dup |= (c0 & (pk == k0)) | (c1 & (k0 == k1));
    }
    return (unsorted ? FLAG_UNSORTED : 0u) | (dup ? FLAG_DUP : 0u);
}

// Per-thread merge-path search inside the LDS tile, then a VT-step serial merge that decides
// emit/skip for each merged item.  Outputs stay in registers (ok/ot + bit mask).
// Sets are strictly increasing, so an equal (A[i], B[j]) pair is adjacent in merge order (A
// first): when A is taken and equals the pending B, that B is the next merged item.
//
// INTERIOR = the tile is full and both "next" halos hold real elements.  Then no cursor needs a
// bounds check: by the merge-path property every B item left in the tile is < A[a1] (the nextA
// halo) and every A item left is <= B[b1] (the nextB halo), so comparing against the halo picks
// the right side by itself, and the equality test against the nextB halo is a real match test.
// That removes ~10 of the ~29 instructions of a step; edge tiles take the checked loop.
// CT (both streams carry one taxid per FILE): the step also records which side an item came from (amask) and whether it
// was a matched pair (mmask) -- two bit masks instead of a taxid per item; ct_keep (diff -t, resolved once per call)
// leaves matched codes in the result.
// union / inter with per-record taxids, the LCAs BEHIND the merge loop and DENSE (round 6; needs the clade table in LDS).
// With the look-ups inside the loop every one of the VT serial steps waits for its own round trip to L2 with a quarter of
// the lanes active (53 % of a tile's cycles in the phase profile, profiles/r06_notes.md section 4).  Here the loop only
// notes which steps need an LCA (`need`) and keeps B's taxid of every step; after the compaction each such step queues
// (place of its output record, B's taxid) in the LDS words the matched records have left free -- a union's tile gives up
// one place per match, an intersection's more -- and the workgroup walks the queue with every lane busy: two clade bytes
// per lane and round, the pair step out of LDS (lca_clade_pair_lds), relatives / unknown / merged ids (about 1 % of
// uniformly random pairs) through the root paths in place.  ~3 dense rounds per tile instead of VT sparse ones.
// (Measured and dropped on the way: the same look-ups per THREAD behind the loop, 2 x 4 / 6 / 12 gathers in flight per
// lane with idle lanes reading entry 0 -- 6.35 / 6.65 / 7.5 ms against 5.56 inside the loop at 2 x 3e8.)
#ifndef SETOP_TAX_DEFER
#define SETOP_TAX_DEFER 1
#endif
template <int OP, bool RANK, bool INTERIOR, int VT>
__device__ __forceinline__ void tile_merge_loop_deferred(const SetopArgs &p, const TileGeom &g, int pa, int pb, const u64 *s_keys,
                                                         const u32 *s_tax, const u32 *s_rank, u64 (&ok)[VT], u32 (&ot)[VT],
                                                         u32 &mask, u32 (&tbm)[VT], u32 &need) {
    static_assert(OP == UKM_OP_UNION || OP == UKM_OP_INTER, "operations whose survivors do not depend on an LCA");
    const int base_a = g.base_a, end_a = g.end_a, end_b = g.end_b;
    const int end_bx = end_b + (g.has_next_b ? 1 : 0);
    u64 ak = s_keys[pa], bk = s_keys[pb];
    u32 ar = 0, br = 0;
    if (RANK) { ar = s_rank[pa]; br = s_rank[pb]; }
    bool eq_prev = false;
    if (OP == UKM_OP_UNION) {
        const bool pv = (pa > base_a) || g.has_prev_a;
        eq_prev = pv && (INTERIOR || pb < end_b) && key_eq<RANK>(s_keys[pa - 1], RANK ? s_rank[pa - 1] : 0, bk, br);
    }
    const bool mix = OP == UKM_OP_INTER && (p.flags & UKM_F_MIX_TAXID) != 0;
    need = 0;  // matched steps whose two taxids differ and are both non-zero: ot[s] holds A's, tbm[s] B's
    mask = 0;
#pragma unroll
    for (int s = 0; s < VT; s++) {
        bool take_a, take_b, match;
        if (INTERIOR) {
            take_a = key_le<RANK>(ak, ar, bk, br);
            take_b = !take_a;
            match = key_eq<RANK>(ak, ar, bk, br);
        } else {
            const bool a_ok = pa < end_a, b_ok = pb < end_b;
            take_a = a_ok && (!b_ok || key_le<RANK>(ak, ar, bk, br));
            take_b = !take_a && b_ok;
            match = take_a && (pb < end_bx) && key_eq<RANK>(ak, ar, bk, br);
        }
        bool emit;
        u64 ek = ak;
        if (OP == UKM_OP_UNION) {
            emit = take_a || (take_b && !eq_prev);
            ek = take_a ? ak : bk;
            eq_prev = match;
        } else {
            emit = match;
        }
        const u32 ta = s_tax[pa], tb = s_tax[pb];
        u32 et = (OP == UKM_OP_UNION && !take_a) ? tb : ta;  // (a match takes A: et = A's taxid)
        const bool zero = ta == 0 || tb == 0;
        if (match && zero) et = mix ? (ta | tb) : 0u;  // LCA(x, 0) = 0; inter --mix-taxid: the other one (inter.go:229-236)
        need |= (match && !zero && ta != tb) ? (1u << s) : 0u;
        tbm[s] = tb;
        ok[s] = ek;
        ot[s] = et;
        mask |= emit ? (1u << s) : 0u;
        pa += take_a ? 1 : 0;
        pb += take_b ? 1 : 0;
        const int idx = take_a ? pa : pb;
        const u64 nk = s_keys[idx];
        ak = take_a ? nk : ak;
        bk = take_a ? bk : nk;
        if (RANK) {
            const u32 nr = s_rank[idx];
            ar = take_a ? nr : ar;
            br = take_a ? br : nr;
        }
    }
}
// the queue: one 8-byte word per step in `need`, behind the tile's compacted records (call with tile_compact)
template <int VT>
__device__ __forceinline__ void tile_queue_lca(u32 excl, u32 mask, u32 need, u32 qpos, const u32 (&tbm)[VT], u64 *s_queue) {
#pragma unroll
    for (int s = 0; s < VT; s++) {
        if (need & (1u << s)) {
            const u32 below = (1u << s) - 1u;
            const u32 w = excl + (u32)__popc(mask & below);
            s_queue[qpos + (u32)__popc(need & below)] = ((u64)w << 32) | tbm[s];
        }
    }
}
// every lane busy: s_tax[w] = LCA(s_tax[w], b) for the n queued (w, b).  A pair the clade codes do not settle (about 1 % of
// uniformly random pairs) would cost its wave two or three more dependent table reads -- 7 % of the kernel, since most waves
// hold one: the tile's first FIX_SLOTS such pairs are handed to setop_taxid_fix_kernel instead (s_fix, s_nfix; their places
// keep A's taxid until then), only what does not fit is settled here.
struct FixLds {
    u32 n;
    u32 w[FIX_SLOTS], a[FIX_SLOTS], b[FIX_SLOTS];
};
template <bool ON> struct FixLdsOpt { FixLds t; };
template <> struct FixLdsOpt<false> { u32 t; };
template <int NTH>
__device__ __forceinline__ void tile_lca_dense(const TaxDev &T, const CladeLds &L, int tid, u32 n, const u64 *s_queue, u32 *s_tax,
                                               FixLds *fx) {
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    auto settle = [&](u32 w, u32 a, u32 b, u32 ca, u32 cb) {
        if (ca != cb && ca != 0 && cb != 0) {
            s_tax[w] = lca_clade_pair_lds(T, L, ca, cb);
            return;
        }
        if (fx) {
            const u32 k = atomicAdd(&fx->n, 1u);
            if (k < FIX_SLOTS) {
                fx->w[k] = w; fx->a[k] = a; fx->b[k] = b;
                return;
            }
        }
        s_tax[w] = lca_from_rows(T, a, b, a < T.size ? T.anc[a] : zero4, b < T.size ? T.anc[b] : zero4);
    };
    for (u32 i = (u32)tid; i < n; i += 2 * NTH) {
        const bool two = i + NTH < n;
        const u64 e0 = s_queue[i], e1 = s_queue[two ? i + NTH : i];
        const u32 w0 = (u32)(e0 >> 32), w1 = (u32)(e1 >> 32), b0 = (u32)e0, b1 = (u32)e1;
        const u32 a0 = s_tax[w0], a1 = s_tax[w1];
        const bool in0 = a0 < T.size && b0 < T.size, in1 = two && a1 < T.size && b1 < T.size;
        const u32 ca0 = T.clade8[in0 ? a0 : 0u], cb0 = T.clade8[in0 ? b0 : 0u];
        const u32 ca1 = T.clade8[in1 ? a1 : 0u], cb1 = T.clade8[in1 ? b1 : 0u];
        settle(w0, a0, b0, ca0, cb0);
        if (two) settle(w1, a1, b1, ca1, cb1);
    }
}

template <int OP, bool TAX, bool RANK, bool INTERIOR, bool CT, int VT, bool DEFER>
__device__ __forceinline__ void tile_merge_loop(const SetopArgs &p, const TileGeom &g, int pa, int pb,
                                                const u64 *s_keys, const u32 *s_tax, const u32 *s_rank,
                                                u64 (&ok)[VT], u32 (&ot)[VT], u32 &mask, u32 &amask, u32 &mmask, bool ct_keep,
                                                const CladeLds *cl, u32 (&tbm)[VT], u32 &need) {
    if constexpr (DEFER) {  // (chosen by the host: the taxonomy comes with one-byte clade codes, TaxDev::cpath)
        static_assert(TAX && !CT, "per-record taxids");
        amask = 0;
        mmask = 0;
        tile_merge_loop_deferred<OP, RANK, INTERIOR, VT>(p, g, pa, pb, s_keys, s_tax, s_rank, ok, ot, mask, tbm, need);
        return;
    }
    const int base_a = g.base_a, end_a = g.end_a, end_b = g.end_b;
    const int end_bx = end_b + (g.has_next_b ? 1 : 0);
    u64 ak = s_keys[pa], bk = s_keys[pb];
    u32 ar = 0, br = 0;
    if (RANK) { ar = s_rank[pa]; br = s_rank[pb]; }
    bool eq_prev = false;  // union: the pending B equals the A that precedes it in merge order
    if (OP == UKM_OP_UNION) {
        const bool pv = (pa > base_a) || g.has_prev_a;
        eq_prev = pv && (INTERIOR || pb < end_b) && key_eq<RANK>(s_keys[pa - 1], RANK ? s_rank[pa - 1] : 0, bk, br);
    }
    const bool mix = (p.flags & UKM_F_MIX_TAXID) != 0;
    const bool cmp = (p.flags & UKM_F_CMP_TAXID) != 0;
    // Files carry few distinct taxids over long stretches (one per genome, or one per clade after LCA
    // assignment), so consecutive matches of a thread mostly ask for the same pair: remember the last one.
    u32 memo_a = 0, memo_b = 0, memo_l = 0;  // LCA(0, 0) = 0
    const bool lds_pairs = TAX && p.tax.cpath != nullptr;  // (uniform) the clade-pair step out of LDS
    auto lca_memo = [&](u32 a, u32 b) -> u32 {
        if (a != memo_a || b != memo_b) {
            memo_l = lds_pairs ? lca_dev_lds(p.tax, *cl, a, b) : lca_dev(p.tax, a, b);
            memo_a = a;
            memo_b = b;
        }
        return memo_l;
    };
    mask = 0;
    amask = 0;
    mmask = 0;
#pragma unroll
    for (int s = 0; s < VT; s++) {
        bool take_a, take_b, match;
        if (INTERIOR) {
            take_a = key_le<RANK>(ak, ar, bk, br);
            take_b = !take_a;
            match = key_eq<RANK>(ak, ar, bk, br);  // implies take_a
        } else {
            const bool a_ok = pa < end_a, b_ok = pb < end_b;
            take_a = a_ok && (!b_ok || key_le<RANK>(ak, ar, bk, br));
            take_b = !take_a && b_ok;
            match = take_a && (pb < end_bx) && key_eq<RANK>(ak, ar, bk, br);
        }
        bool emit;
        u64 ek = ak;
        u32 et = 0;
        if (OP == UKM_OP_UNION) {
            emit = take_a || (take_b && !eq_prev);
            ek = take_a ? ak : bk;
            eq_prev = match;
        } else if (OP == UKM_OP_INTER) {
            emit = match;
        } else if (OP == UKM_OP_MERGE_INTERNAL) {
            emit = take_a || take_b;
            ek = take_a ? ak : bk;
        } else {
            emit = take_a && !match;
            if (CT) emit = take_a && (!match || ct_keep);
        }
        if (CT) {
            amask |= take_a ? (1u << s) : 0u;
            mmask |= match ? (1u << s) : 0u;
        }
        if (TAX) {
            const u32 ta = s_tax[pa], tb = s_tax[pb];
            if (OP == UKM_OP_UNION) {
                et = take_a ? ta : tb;
                if (match) et = lca_memo(ta, tb);
            } else if (OP == UKM_OP_INTER) {
                if (match) {
                    if (mix) et = (ta == 0) ? tb : ((tb == 0) ? ta : lca_memo(ta, tb));
                    else et = lca_memo(ta, tb);
                }
            } else if (OP == UKM_OP_MERGE_INTERNAL) {
                et = take_a ? ta : tb;
            } else {
                et = ta;
                if (match && cmp && (ta == tb || lca_memo(tb, ta) == ta)) emit = true;
            }
        }
        ok[s] = ek;
        ot[s] = et;
        mask |= emit ? (1u << s) : 0u;
        pa += take_a ? 1 : 0;
        pb += take_b ? 1 : 0;
        // one LDS read refills whichever cursor moved (when neither moved it re-reads bk)
        const int idx = take_a ? pa : pb;
        const u64 nk = s_keys[idx];
        ak = take_a ? nk : ak;
        bk = take_a ? bk : nk;
        if (RANK) {
            const u32 nr = s_rank[idx];
            ar = take_a ? nr : ar;
            br = take_a ? br : nr;
        }
    }
}

template <int OP, bool TAX, bool RANK, bool CT, int NTH, int VT, bool DEFER>
__device__ __forceinline__ void tile_merge(const SetopArgs &p, const TileGeom &g, int tid, const u64 *s_keys,
                                           const u32 *s_tax, const u32 *s_rank, u64 (&ok)[VT], u32 (&ot)[VT],
                                           u32 &mask, u32 &amask, u32 &mmask, bool ct_keep, int &ia0, int &ib0, const CladeLds *cl,
                                           u32 (&tbm)[VT], u32 &need) {
    const int na_t = g.na_t, nb_t = g.nb_t, total = na_t + nb_t;
    const int base_a = g.base_a, base_b = g.base_b;
    int diag = tid * VT;
    if (diag > total) diag = total;
    int lo = diag > nb_t ? diag - nb_t : 0;
    int hi = diag < na_t ? diag : na_t;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int ia = base_a + mid, ib = base_b + diag - 1 - mid;
        const bool le = key_le<RANK>(s_keys[ia], RANK ? s_rank[ia] : 0, s_keys[ib], RANK ? s_rank[ib] : 0);
        lo = le ? mid + 1 : lo;
        hi = le ? hi : mid;
    }
    const int pa = base_a + lo, pb = base_b + diag - lo;
    ia0 = lo;         // the thread's first A / B record, counted from the tile's first (source words, below)
    ib0 = diag - lo;
    // wave-uniform choice (tile geometry): no divergence
    if (total == NTH * VT && g.has_next_a && g.has_next_b)
        tile_merge_loop<OP, TAX, RANK, true, CT, VT, DEFER>(p, g, pa, pb, s_keys, s_tax, s_rank, ok, ot, mask, amask, mmask, ct_keep, cl, tbm, need);
    else
        tile_merge_loop<OP, TAX, RANK, false, CT, VT, DEFER>(p, g, pa, pb, s_keys, s_tax, s_rank, ok, ot, mask, amask, mmask, ct_keep, cl, tbm, need);
}

// compact the emitted items of this thread into LDS at its exclusive offset
template <bool TAX, int VT>
__device__ __forceinline__ void tile_compact(u32 excl, u32 mask, const u64 (&ok)[VT], const u32 (&ot)[VT],
                                             u64 *s_keys, u32 *s_tax) {
#pragma unroll
    for (int s = 0; s < VT; s++) {
        if (mask & (1u << s)) {
            const u32 w = excl + (u32)__popc(mask & ((1u << s) - 1u));
            s_keys[w] = ok[s];
            if (TAX) s_tax[w] = ot[s];
        }
    }
}

// LDS -> HBM: contiguous coalesced run of `count` records at out[base ...), 16 bytes per store
// where the global address allows it (the first/last record may go out alone).
// SETOP_FLUSH_NT: the cache policy of the 16-byte stores of plain keys (with per-record taxids they are non-temporal
// anyway, see tile_load).  0 = the default policy, 1 = nt.  An experiment switch like SETOP_DMA_NT, a compile-time
// constant for the same reason; the measurements behind the default are in profiles/xcd_order_notes.md.
#ifndef SETOP_FLUSH_NT
#define SETOP_FLUSH_NT 0
#endif
template <bool TAX, int NTH>
__device__ __forceinline__ void tile_flush(const SetopArgs &p, int tid, u64 base, u32 count, const u64 *s_keys,
                                           const u32 *s_tax) {
    if (base + count <= p.out_cap) {
        u64 *o = p.out + base;
        const int sh = (int)(((uintptr_t)o >> 3) & 1);  // 1: o[0] sits on an odd 8-byte slot
        const int npairs = ((int)count + sh + 1) >> 1;
        for (int m = tid; m < npairs; m += NTH) {
            const int i0 = 2 * m - sh, i1 = i0 + 1;
            const bool v0 = i0 >= 0, v1 = i1 < (int)count;
            const u64 k0 = s_keys[v0 ? i0 : 0], k1 = s_keys[v1 ? i1 : 0];
            if ((TAX || SETOP_FLUSH_NT) && v0 && v1) {  // (non-temporal beside the taxid look-ups: see tile_load)
                typedef u64 v2u64 __attribute__((ext_vector_type(2)));
                v2u64 w;
                w.x = k0;
                w.y = k1;
                __builtin_nontemporal_store(w, reinterpret_cast<v2u64 *>(o + i0));
            } else if (v0 && v1) *reinterpret_cast<ulonglong2 *>(o + i0) = make_ulonglong2(k0, k1);
            else if (v0) o[i0] = k0;
            else if (v1) o[i1] = k1;
        }
        if (TAX) {
            u32 *to = p.tout + base;
            for (u32 i = (u32)tid; i < count; i += NTH) __builtin_nontemporal_store(s_tax[i], to + i);
        }
    } else {  // capacity overflow: guarded stores; the host reports UKM_ERR_CAPACITY
        for (u32 i = (u32)tid; i < count; i += NTH) {
            const u64 pos = base + i;
            if (pos < p.out_cap) {
                p.out[pos] = s_keys[i];
                if (TAX) p.tout[pos] = s_tax[i];
            }
        }
    }
}

// Both streams carry one taxid per FILE (CT): the taxids of the tile's output.  inter: every record gets LCA(A's, B's)
// (mix-taxid rule included), diff: A's own -- a fill.  union / keep-everything merge: A's, B's or the LCA by where the
// record came from; the values go through the LDS words the compacted keys have just left (no LDS beyond the plain
// kernel's), so that the stores are as coalesced as the keys'.
template <int OP, int NTH, int VT>
__device__ __forceinline__ void tile_flush_ct(const SetopArgs &p, int tid, u64 base, u32 count, u32 excl, u32 mask, u32 amask,
                                              u32 mmask, u32 ct_lca, u32 *s_t32) {
    if (OP == UKM_OP_INTER || OP == UKM_OP_DIFF) {
        const u32 v = OP == UKM_OP_INTER ? ct_lca : p.cta;
        for (u32 i = (u32)tid; i < count; i += NTH)
            if (base + i < p.out_cap) p.tout[base + i] = v;
        return;
    }
    __syncthreads();  // every thread has stored its share of the compacted keys
#pragma unroll
    for (int s = 0; s < VT; s++) {
        if (mask & (1u << s)) {
            const u32 w = excl + (u32)__popc(mask & ((1u << s) - 1u));
            const bool m = OP == UKM_OP_UNION && ((mmask >> s) & 1u);
            s_t32[w] = m ? ct_lca : (((amask >> s) & 1u) ? p.cta : p.ctb);
        }
    }
    __syncthreads();
    for (u32 i = (u32)tid; i < count; i += NTH)
        if (base + i < p.out_cap) p.tout[base + i] = s_t32[i];
}
