// ukm_sort_kernels.h — the kernels of the radix sort's passes through HBM: radix_hist_kernel (the digit histograms of all
// passes, or of one, and the OR of all keys), radix_bases_kernel (a histogram's exclusive bases, on the stream between two
// passes) and onesweep_kernel (one scatter pass: PassArgs) with the hand-scheduled match_any8 its ranking rests on.
// Included by ukm_sort.hip alone, inside its anonymous namespace, after ukm_sort_plan.h (digit width RB, tile shapes).

constexpr int NT = 256;  // histogram kernel
constexpr int RADIX = 1 << RB;
constexpr u32 DMASK = RADIX - 1;
constexpr int MAX_PASSES = 8;

// ---- histogram of all digits -------------------------------------------------------------------
struct __attribute__((packed, aligned(8))) U2a8 {  // 16 bytes at 8-byte alignment
    u64 x, y;
};
__global__ __launch_bounds__(NT) void radix_hist_kernel(const u64 *k, u64 n, int passes, u64 *ghist, u64 *or_all, int shift0) {
    __shared__ u32 s_h[MAX_PASSES * RADIX];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < MAX_PASSES * RADIX; i += NT) s_h[i] = 0;
    __syncthreads();
    constexpr int U = 4;  // independent 16-byte loads in flight per thread (one 8-byte load per iteration was latency
                          // bound: 1.6 TB/s; four: 3.6 TB/s; four pairs: 4.3 TB/s.  Four copies of every bin, chosen by the lane, were slower: 0.206 against 0.185 ms)
    constexpr u64 STEP = (u64)NT * U * 2;
    const u64 per_block = ((n + gridDim.x - 1) / gridDim.x + STEP - 1) / STEP * STEP;
    const u64 beg = (u64)blockIdx.x * per_block;
    const u64 end = (beg + per_block < n) ? beg + per_block : n;
    u64 orv = 0;  // OR of every key this thread sees: tells the host which high digits are all zero
    for (u64 i0 = beg; i0 < end; i0 += STEP) {
        u64 key[2 * U];
        bool valid[2 * U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u64 i = i0 + ((u64)u * NT + tid) * 2;
            valid[2 * u] = i < end;
            valid[2 * u + 1] = i + 1 < end;
            if (i + 1 < end) {
                const U2a8 q = *reinterpret_cast<const U2a8 *>(k + i);  // (the caller's array may start on an odd 8-byte slot)
                key[2 * u] = q.x;
                key[2 * u + 1] = q.y;
            } else {
                key[2 * u] = k[valid[2 * u] ? i : end - 1];
                key[2 * u + 1] = key[2 * u];
            }
        }
#pragma unroll
        for (int u = 0; u < 2 * U; u++) {
            const u64 vm = __ballot(valid[u]);
            if (valid[u]) orv |= key[u];
            for (int p = 0; p < passes; p++) {
                const u32 d = (u32)(key[u] >> (shift0 + RB * p)) & DMASK;
                const u32 d0 = __builtin_amdgcn_readfirstlane(d);
                if (vm == ~0ull && __all(d == d0)) {
                    if (lane_id() == 0) atomicAdd(&s_h[p * RADIX + d0], 64u);
                } else if (valid[u]) {
                    atomicAdd(&s_h[p * RADIX + d], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < passes * RADIX; i += NT) {
        u32 v = s_h[i];
        if (v) atomicAdd((unsigned long long *)&ghist[i], (unsigned long long)v);
    }
    if (or_all) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) orv |= __shfl_xor(orv, d, 64);
        if (lane_id() == 0 && orv) atomicOr((unsigned long long *)or_all, (unsigned long long)orv);
    }
}

// ---- onesweep pass -------------------------------------------------------------------------------
template <typename SW> struct SWTraits;
template <> struct SWTraits<u32> {
    static constexpr u32 AGG = 1u << 30, INCL = 2u << 30, VAL = (1u << 30) - 1;
    static constexpr int SHIFT = 30;
};
template <> struct SWTraits<u64> {
    static constexpr u64 AGG = 1ull << 62, INCL = 2ull << 62, VAL = (1ull << 62) - 1;
    static constexpr int SHIFT = 62;
};

template <typename SW>
struct PassArgs {
    const u64 *kin;
    u64 *kout;
    const u32 *vin;
    u32 *vout;
    u64 n;
    int shift;
    SW *status;  // [ntiles][256]
    u32 *ticket;       // tile ids come from this counter, whatever the dispatch order
    const u64 *gbase;  // [256] exclusive digit bases of this pass
    u64 ntiles;
    u64 *next_hist;    // fused mode: [256] digit counts of the NEXT pass, accumulated while this pass scatters (or nullptr)
    int next_shift;
};

// exclusive digit bases of one pass from its histogram (fused mode: runs on the stream between two passes, so the
// host never sees the histograms)
__global__ void radix_bases_kernel(const u64 *hist, u64 *gbase) {
    __shared__ u64 s[RADIX];
    const int d = (int)threadIdx.x;
    s[d] = hist[d];
    __syncthreads();
    if (d == 0) {
        u64 sum = 0;
        for (int i = 0; i < RADIX; i++) {
            const u64 v = s[i];
            s[i] = sum;
            sum += v;
        }
    }
    __syncthreads();
    gbase[d] = s[d];
}

// "match any" on an 8-bit digit: on return (phi:plo) is the 64-bit mask of the lanes whose digit
// equals this lane's.  Per bit: sign-extended bit x (0 / -1), ballot m = (x != 0), peers &= ~(m ^ x)
// with gfx950's three-input v_bitop3_b32 (truth table 0x90 = a & ~(b ^ c)) on each 32-bit half:
// 4 VALU instructions per bit.  Hand-scheduled because a VALU read of an SGPR needs 2 wait states
// after the VALU write: three ballot registers rotate so that every v_cmp is at least 2
// instructions ahead of its first reader (the compiler's version spent s_nops or extra shifts
// here and the ranking made the kernel VALU bound: 85 -> 36 instructions per key).
__device__ __forceinline__ void match_any8(u32 d, u32 &plo, u32 &phi) {
    u32 x, y, z;
    plo = ~0u;
    phi = ~0u;
    asm("v_bfe_i32 %2, %5, 0, 1\n\t"
        "v_bfe_i32 %3, %5, 1, 1\n\t"
        "v_bfe_i32 %4, %5, 2, 1\n\t"
        "v_cmp_ne_u32_e64 vcc, 0, %2\n\t"
        "v_cmp_ne_u32_e64 s[80:81], 0, %3\n\t"
        "v_cmp_ne_u32_e64 s[82:83], 0, %4\n\t"
        "v_bitop3_b32 %0, %0, vcc_lo, %2 bitop3:0x90\n\t"
        "v_bitop3_b32 %1, %1, vcc_hi, %2 bitop3:0x90\n\t"
        "v_bfe_i32 %2, %5, 3, 1\n\t"
        "v_cmp_ne_u32_e64 vcc, 0, %2\n\t"
        "v_bitop3_b32 %0, %0, s80, %3 bitop3:0x90\n\t"
        "v_bitop3_b32 %1, %1, s81, %3 bitop3:0x90\n\t"
        "v_bfe_i32 %3, %5, 4, 1\n\t"
        "v_cmp_ne_u32_e64 s[80:81], 0, %3\n\t"
        "v_bitop3_b32 %0, %0, s82, %4 bitop3:0x90\n\t"
        "v_bitop3_b32 %1, %1, s83, %4 bitop3:0x90\n\t"
        "v_bfe_i32 %4, %5, 5, 1\n\t"
        "v_cmp_ne_u32_e64 s[82:83], 0, %4\n\t"
        "v_bitop3_b32 %0, %0, vcc_lo, %2 bitop3:0x90\n\t"
        "v_bitop3_b32 %1, %1, vcc_hi, %2 bitop3:0x90\n\t"
        "v_bfe_i32 %2, %5, 6, 1\n\t"
        "v_cmp_ne_u32_e64 vcc, 0, %2\n\t"
        "v_bitop3_b32 %0, %0, s80, %3 bitop3:0x90\n\t"
        "v_bitop3_b32 %1, %1, s81, %3 bitop3:0x90\n\t"
        "v_bfe_i32 %3, %5, 7, 1\n\t"
        "v_cmp_ne_u32_e64 s[80:81], 0, %3\n\t"
        "v_bitop3_b32 %0, %0, s82, %4 bitop3:0x90\n\t"
        "v_bitop3_b32 %1, %1, s83, %4 bitop3:0x90\n\t"
        "v_bitop3_b32 %0, %0, vcc_lo, %2 bitop3:0x90\n\t"
        "v_bitop3_b32 %1, %1, vcc_hi, %2 bitop3:0x90\n\t"
        "v_bitop3_b32 %0, %0, s80, %3 bitop3:0x90\n\t"
        "v_bitop3_b32 %1, %1, s81, %3 bitop3:0x90"
        : "+v"(plo), "+v"(phi), "=&v"(x), "=&v"(y), "=&v"(z)
        : "v"(d)
        : "vcc", "s80", "s81", "s82", "s83");  // ordinary SGPRs: the top ones (s100, s101 ...) are reserved by the compiler
}

static_assert(RB == 8, "match_any8 ranks 8-bit digits");

// Tile ids always come from an atomic counter: every predecessor of a running tile is running or done whatever the
// dispatch order, so the look-back below needs no watchdog and the host reads nothing back (the blockIdx form of
// ukm_setops.hip would cost a host round trip per pass for its flag).
#ifdef SORT_WAVES_PER_EU
#define SORT_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(SORT_WAVES_PER_EU, SORT_WAVES_PER_EU)))
#else
#define SORT_WAVES_ATTR
#endif
template <typename SW, bool PAIRS, int NT_, int VT_>
__global__ __launch_bounds__(NT_) SORT_WAVES_ATTR void onesweep_kernel(PassArgs<SW> p) {
    constexpr int NT = NT_, NW = NT_ / 64, VT = VT_, TILE = NT_ * VT_;  // NT >= RADIX: thread d < 256 owns digit d
    static_assert(NT_ >= RADIX && NT_ % 64 == 0, "workgroup must cover all digits");
    static_assert(64 * VT_ < 65536, "per-wave digit counts are 16-bit");
    using T = SWTraits<SW>;
    __shared__ u64 s_keys[TILE];
    __shared__ u32 s_vals[PAIRS ? TILE : 1];
    __shared__ unsigned short s_whist[NW][RADIX];  // per-wave digit counts (<= 64 * VT)
    __shared__ u32 s_dexcl[RADIX];
    __shared__ u64 s_gbase[RADIX];
    __shared__ u32 s_scan[NW + 1];
    __shared__ u32 s_tile;
    __shared__ u32 s_nh[RADIX];
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    if (tid == 0) s_tile = atomicAdd(p.ticket, 1u);
    if (tid < RADIX) s_nh[tid] = 0;
    for (int i = tid; i < NW * RADIX / 2; i += NT) reinterpret_cast<u32 *>(&s_whist[0][0])[i] = 0;
    __syncthreads();
    const u64 tile = (u64)s_tile;
    const u64 tbase = tile * (u64)TILE;
    const u32 valid_count = (u32)((p.n - tbase < (u64)TILE) ? (p.n - tbase) : (u64)TILE);

    // wave w owns keys [w*64*VT, (w+1)*64*VT) of the tile, striped across its lanes
    u64 key[VT];
    u32 val[VT];
    u32 rank[VT];
    const u32 wbase_idx = (u32)wave * 64 * VT + (u32)lane;
#pragma unroll
    for (int j = 0; j < VT; j++) {
        const u32 li = wbase_idx + j * 64;
        const bool v = li < valid_count;
        key[j] = v ? p.kin[tbase + li] : ~0ull;
        if (PAIRS) val[j] = v ? p.vin[tbase + li] : 0;
    }
    // Stable ranking inside the wave by "match any": after 8 ballots `peers` holds the lanes whose
    // digit equals this lane's.  Written on 32-bit halves with a sign-extended bit (0 / -1) and gfx950's
    // three-input v_bitop3_b32 (peers & ~(ballot ^ bit) in ONE instruction), so that a digit bit costs
    // v_bfe_i32 + v_cmp + 2 x v_bitop3: the 64-bit `bit ? m : ~m` form compiled to 9 VALU
    // instructions per bit and made the kernel VALU bound.
    const u32 lt_lo = lane < 32 ? ((1u << lane) - 1u) : ~0u;
    const u32 lt_hi = lane < 32 ? 0u : ((1u << (lane - 32)) - 1u);
#pragma unroll
    for (int j = 0; j < VT; j++) {
        const u32 li = wbase_idx + j * 64;
        // padding items take the highest digit; they sit at the end of the tile order, so they rank
        // after every real key of that digit and are dropped at write-out
        const u32 d = (li < valid_count) ? ((u32)(key[j] >> p.shift) & DMASK) : DMASK;
        u32 plo, phi;
        match_any8(d, plo, phi);
        const u32 pre = s_whist[wave][d];
        const u32 r = (u32)__popc(plo & lt_lo) + (u32)__popc(phi & lt_hi);
        const u32 tot = (u32)__popc(plo) + (u32)__popc(phi);
        rank[j] = pre + r;
        // fused mode: this key's digit of the NEXT pass is counted here, so that no separate pass over the keys is
        // needed for it (the pre-pass builds the first histogram only)
        if (p.next_hist && li < valid_count) atomicAdd(&s_nh[(u32)(key[j] >> p.next_shift) & DMASK], 1u);
        // every peer stores the same new count (same address, same value): no branch, so the 16 keys'
        // ranking stays one basic block that the scheduler can interleave
        s_whist[wave][d] = (unsigned short)(pre + tot);
    }
    __syncthreads();

    // thread d: exclusive scan over the waves, tile count of digit d
    const int d = tid & (RADIX - 1);
    const bool owner = tid < RADIX;  // workgroup-size independent: the first 256 threads own the digits
    u32 cnt = 0;
    if (owner) {
#pragma unroll
        for (int w = 0; w < NW; w++) {
            u32 c = s_whist[w][d];
            s_whist[w][d] = (unsigned short)cnt;
            cnt += c;
        }
    }
    u32 real_cnt = cnt;
    if (d == (int)DMASK) real_cnt -= (u32)TILE - valid_count;
    // publish the tile's count of digit d, then look back
    SW *st = p.status + tile * RADIX + d;
    if (owner) {
        if (tile == 0) __hip_atomic_store(st, (SW)(T::INCL | (SW)real_cnt), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else __hip_atomic_store(st, (SW)(T::AGG | (SW)real_cnt), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

    u32 tile_total;
    const u32 dex = block_excl_scan_u32<NT>(cnt, s_scan, &tile_total);  // contains barriers
    if (owner) s_dexcl[d] = dex;
    __syncthreads();

    // local reorder: tile becomes digit-sorted (stable) in LDS
#pragma unroll
    for (int j = 0; j < VT; j++) {
        const u32 li = wbase_idx + j * 64;
        const u32 dd = (li < valid_count) ? ((u32)(key[j] >> p.shift) & DMASK) : DMASK;
        const u32 pos = s_dexcl[dd] + s_whist[wave][dd] + rank[j];
        s_keys[pos] = key[j];
        if (PAIRS) s_vals[pos] = val[j];
    }

    // per-digit decoupled look-back: thread d walks back over the tiles' counts of digit d,
    // SORT_LB_W tiles per hop (independent loads in flight together; one hop is a ~1.5 us
    // device-scope round trip, so a one-tile-per-hop walk was latency bound)
    u64 excl = 0;
    if (tile > 0 && owner) {
        long long t = (long long)tile - 1;
        bool done = false;
        while (!done) {
            SW w[SORT_LB_W];
#pragma unroll
            for (int q = 0; q < SORT_LB_W; q++) {
                const long long tq = t - q;
                w[q] = (tq >= 0) ? __hip_atomic_load(p.status + (u64)tq * RADIX + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                 : (SW)T::INCL;
            }
            int used = 0;
#pragma unroll
            for (int q = 0; q < SORT_LB_W; q++) {
                if (!done && used == q) {
                    const u32 state = (u32)(w[q] >> T::SHIFT);
                    if (state != 0) {
                        excl += (u64)(w[q] & T::VAL);
                        used = q + 1;
                        if (state == 2) done = true;
                    }
                }
            }
            t -= used;
            // hit an unpublished tile: back off, then re-read from it (its workgroup is running: the wait always ends)
            if (!done && used < SORT_LB_W) __builtin_amdgcn_s_sleep(4);
        }
        __hip_atomic_store(st, (SW)(T::INCL | (SW)(excl + real_cnt)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (owner) s_gbase[d] = p.gbase[d] + excl - (u64)dex;
    if (p.next_hist && owner) {
        const u32 c = s_nh[d];  // (complete: at least one barrier lies between the counting and here)
        if (c) atomicAdd((unsigned long long *)&p.next_hist[d], (unsigned long long)c);
    }
    __syncthreads();

    for (u32 i = (u32)tid; i < valid_count; i += NT) {
        const u64 kk = s_keys[i];
        const u32 dd = (u32)(kk >> p.shift) & DMASK;
        const u64 pos = s_gbase[dd] + i;
        p.kout[pos] = kk;
        if (PAIRS) p.vout[pos] = s_vals[i];
    }
}
