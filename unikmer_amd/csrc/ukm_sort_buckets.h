// ukm_sort_buckets.h — the kernels of the radix sort's bucket route (LocalSortArgs, ls_*).
// ---- two passes over the TOP 16 bits, then every bucket sorted inside LDS -------------------------------------------
// A scatter pass costs ~0.43 ms per 1e8 keys whatever it moves (latency bound, above), and a 62-bit key takes eight of
// them.  Sorted by its top 16 bits alone (two passes: LSD over the two highest digits) the array falls into 65,536
// buckets of n / 65,536 keys on evenly spread keys (k-mer codes, hashes): 1.5 k keys = 12 KB at n = 1e8, which one
// 256-thread workgroup sorts by the remaining low bits entirely in LDS (the same ballot ranking as the global pass,
// ping-pong between two LDS buffers) and writes back in place.  Keys cross HBM three times instead of eight.
// Twelve instantiations (256 ... 4096 keys) serve the buckets by size class; buckets beyond 4096 keys are sorted by the
// general route afterwards; too many of those, narrow keys, or n beyond ~1.3e8 and the whole call takes the general
// route (the two passes only permuted the keys).
// (The plan, the size classes LS_CLASS_KPT and every threshold of this route: ukm_sort_plan.h.)
// Included by ukm_sort.hip alone, inside its anonymous namespace, after ukm_sort_kernels.h (match_any8, RADIX, DMASK).
constexpr int LS_NW = LS_NT / 64;

struct LocalSortArgs {
    const u64 *src;    // sorted by its top bits (the caller's array after two top passes, the scratch copy after three)
    const u32 *vsrc;   // taxids riding along (PAIRS) or nullptr
    u64 *keys;         // the caller's array: every bucket is written to its own segment
    u32 *vals;
    u64 n;
    const u64 *start;  // [2^topb + 1]
    int low_bits;      // bits below the bucket bits
    const u32 *ids;    // the buckets of this launch's size class
    int counting;      // 1: one counting step + a walk inside the bins (round 5); 0: digit passes only
    u64 *stat;         // [0] += 1 per bucket that fell back from the counting step
};

// start[b] = first index whose bucket value (key >> low_bits) is >= b (b = 0 .. 2^topb)
__global__ void ls_bounds_kernel(const u64 *keys, u64 n, int low_bits, int topb, u64 *start) {
    const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > (1u << topb)) return;
    u64 lo = 0, hi = n;
    if (b == (1u << topb)) {
        lo = n;
    } else {
        while (lo < hi) {
            const u64 mid = (lo + hi) >> 1;
            if ((keys[mid] >> low_bits) < (u64)b) lo = mid + 1; else hi = mid;
        }
    }
    start[b] = lo;
}

// A sample of 2^20 keys counted by bucket, then the buckets whose share of the sample says "beyond 4096 keys":
// run before the two passes on a context that has already met crowded keys (a wasted attempt costs two passes)
__global__ void ls_sample_kernel(const u64 *keys, u64 n, int low_bits, int topb, u32 *cnt, u32 nsamp) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsamp) return;
    const u64 pos = (u64)(((unsigned __int128)i * n) / nsamp);
    const u64 bb = keys[pos] >> low_bits;
    const u32 b = bb < (1u << topb) ? (u32)bb : (1u << topb) - 1;
    // one atomic per distinct bucket of the wave (crowded keys: 2^20 atomics on a few dozen addresses took ~1 ms)
    bool todo = true;
    while (todo) {
        const u32 b0 = (u32)__builtin_amdgcn_readfirstlane((int)b);
        const u64 same = __ballot(b == b0);
        if (b == b0) {
            if ((int)lane_id() == __ffsll((long long)same) - 1) atomicAdd(&cnt[b0], (u32)__popcll(same));
            todo = false;
        }
    }
}
__global__ void ls_sample_count_kernel(const u32 *cnt, u32 thr, u64 *out) {  // out[0] heavy buckets, out[1] samples in them
    const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 cb = cnt[b];
    const u64 m = __ballot(cb > thr);
    if (m == 0ull) return;
    u64 in_heavy = cb > thr ? cb : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) in_heavy += __shfl_xor(in_heavy, d, 64);
    if (lane_id() == 0) {
        atomicAdd((unsigned long long *)&out[0], (unsigned long long)__popcll(m));
        atomicAdd((unsigned long long *)&out[1], (unsigned long long)in_heavy);
    }
}

// size class of every bucket: cls[k] = number of buckets of class k (k = LS_NCLASS: beyond every class, their ids in
// cls[LS_NCLASS + 1 ...]); ids[k][...] = the buckets of class k
__global__ void ls_classify_kernel(const u64 *start, u64 *cls, u32 *ids, int topb, u32 *big_ids, u64 *big_size, u64 *stat) {
    const u32 b = blockIdx.x * blockDim.x + threadIdx.x;  // (the grid covers the buckets exactly)
    if (b == 0) cls[LS_NCLASS + 2] = (u64)atomicExch((unsigned long long *)stat, 0ull);  // the previous call's fall-backs
    const u64 m = start[b + 1] - start[b];
    int k = -1;  // ls_class_of(m) of ukm_sort_plan.h, written out: through the call the compiler lays this kernel out differently
    if (m > 0) {  // (a bucket of one key still has to reach the caller's array when the sorted-by-top-bits copy is the scratch)
        k = 0;
        while (k < LS_NCLASS && m > (u64)LS_NT * LS_CLASS_KPT[k]) k++;
    }
    // one atomic per wave and class (65,536 atomics on two or three addresses took 0.55 ms)
    const u64 lt = (1ull << lane_id()) - 1ull;
    for (int q = 0; q <= LS_NCLASS; q++) {
        const u64 mask = __ballot(k == q);
        if (mask == 0ull) continue;
        const int lead = __ffsll((long long)mask) - 1;
        u64 at = 0;
        if (lane_id() == lead) at = atomicAdd((unsigned long long *)&cls[q], (unsigned long long)__popcll(mask));
        at = __shfl(at, lead, 64) + (u64)__popcll(mask & lt);
        if (k == q) {
            if (q < LS_NCLASS) ids[(size_t)q << topb | at] = b;
            else if (at < (u64)LS_MAX_BIG) big_ids[at] = b;
        }
    }
    // keys in oversized buckets (cls[LS_NCLASS + 1]): one atomic per wave; big_size[b] = the bucket's size if it is one of
    // them, else 0: its exclusive scan is where every oversized bucket lies in the gathered array (bucket order)
    u64 big = k == LS_NCLASS ? m : 0;
    big_size[b] = big;
    if (__ballot(big != 0) != 0ull) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) big += __shfl_xor(big, d, 64);
        if (lane_id() == 0) atomicAdd((unsigned long long *)&cls[LS_NCLASS + 1], (unsigned long long)big);
    }
}

// the oversized buckets <-> one array in which they lie side by side in bucket order (BACK: the sorted array to the
// caller's).  blockIdx.x = entry of the list, blockIdx.y = one of gridDim.y parts of the bucket (a single code with
// millions of copies -- poly-A -- is one bucket)
template <bool BACK>
__global__ void ls_big_copy_kernel(const u32 *big_ids, const u64 *start, const u64 *big_off, const u64 *src, const u32 *vsrc,
                                   u64 *dst, u32 *vdst) {
    const u32 b = big_ids[blockIdx.x];
    const u64 s0 = start[b], m = start[b + 1] - s0, o = big_off[b];
    const u64 lo = m * blockIdx.y / gridDim.y, hi = m * (blockIdx.y + 1) / gridDim.y;
    for (u64 i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        if (BACK) {
            dst[s0 + i] = src[o + i];
            if (vsrc) vdst[s0 + i] = vsrc[o + i];
        } else {
            dst[o + i] = src[s0 + i];
            if (vsrc) vdst[o + i] = vsrc[s0 + i];
        }
    }
}

// Round 5: ONE counting step instead of the six digit passes.  The bucket's keys are spread over NBIN >= capacity bins
// by the bits right below the bucket bits (an LDS atomic per key: its arrival number inside the bin), the bin sizes are
// scanned, every key is put into its bin's range, and its place INSIDE the bin is the number of the bin's keys that
// precede it -- a walk over 1.4 keys on average for evenly spread low bits (k-mer codes, hashes), instead of five more
// passes of 8 ballots, two counter updates, four barriers and an LDS round trip each.  Equal keys are ordered by their
// place in the input (pairs: the sort stays stable; plain keys: any order).  A bucket with a bin of more than LS_BIN_MAX
// keys (a repeated k-mer, keys that differ in their lowest bits only) takes the digit passes as before.
constexpr u32 LS_BIN_MAX = 64;
template <int CAP> struct LsBins {
    static constexpr int NBIN = CAP <= 256 ? 256 : CAP <= 512 ? 512 : CAP <= 1024 ? 1024 : CAP <= 2048 ? 2048 : 4096;
    static constexpr int HB = CAP <= 256 ? 8 : CAP <= 512 ? 9 : CAP <= 1024 ? 10 : CAP <= 2048 ? 11 : 12;
};

template <int LS_KPT, bool PAIRS = false>
__global__ __launch_bounds__(LS_NT) void ls_sort_kernel(LocalSortArgs a) {
    constexpr int LS_CAP = LS_NT * LS_KPT;
    constexpr int NBIN = LsBins<LS_CAP>::NBIN, HB = LsBins<LS_CAP>::HB, BPT = NBIN / LS_NT;
    static_assert((NBIN + 1) * 4 <= LS_CAP * 8, "the bin counters live in the second key buffer");
    static_assert(LS_CAP <= 65536, "16-bit input positions");
    __shared__ __attribute__((aligned(16))) u64 s_buf[2][LS_CAP];
    __shared__ u32 s_vbuf[PAIRS ? 2 : 1][PAIRS ? LS_CAP : 1];
    __shared__ unsigned short s_wh[LS_NW][RADIX];
    __shared__ u32 s_dex[RADIX];
    __shared__ u32 s_scan[LS_NW + 1];
    static_assert(LS_NT == RADIX, "thread d owns digit d");
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const u32 b = a.ids[blockIdx.x];
    const u64 beg = a.start[b], end = a.start[b + 1];
    const u64 m64 = end - beg;
    const u32 m = (u32)m64;
    u64 key[LS_KPT];
    u32 val[PAIRS ? LS_KPT : 1];
    const u32 wbase = (u32)wave * 64 * LS_KPT + (u32)lane;
#pragma unroll
    for (int j = 0; j < LS_KPT; j++) {
        const u32 i = wbase + j * 64;
        key[j] = i < m ? a.src[beg + i] : ~0ull;  // padding: the highest digit in every pass, last in tile order
        if (PAIRS) val[j] = i < m ? a.vsrc[beg + i] : 0u;
    }
    if (a.counting && a.low_bits >= HB) {
        u32 *s_cnt = reinterpret_cast<u32 *>(&s_buf[1][0]);                         // [NBIN + 1]
        unsigned short *s_idx = reinterpret_cast<unsigned short *>(&s_vbuf[PAIRS ? 1 : 0][0]);  // (pairs) input position of the key at a place
        u64 *grp = &s_buf[0][0];
        const int bshift = a.low_bits - HB;
        for (int i = tid; i < NBIN + 1; i += LS_NT) s_cnt[i] = 0;
        __syncthreads();
        u32 pos[LS_KPT];
#pragma unroll
        for (int j = 0; j < LS_KPT; j++) {
            const u32 bin = (u32)(key[j] >> bshift) & (u32)(NBIN - 1);
            pos[j] = 0;
            if (wbase + j * 64 < m) pos[j] = atomicAdd(&s_cnt[bin], 1u);
        }
        __syncthreads();
        u32 c[BPT], sum = 0, mx = 0, sq = 0;
#pragma unroll
        for (int q = 0; q < BPT; q++) {
            c[q] = s_cnt[tid * BPT + q];
            sum += c[q];
            mx = c[q] > mx ? c[q] : mx;
            sq += c[q] * c[q];  // the walks below read (bin size)^2 keys per bin
        }
        u32 total = 0;
        u32 run = block_excl_scan_u32<LS_NT>(sum, s_scan, &total);
        const u32 wsq = wave_incl_scan_u32(sq);
        if (lane == 63) s_scan[wave] = wsq;
        int heavy = __syncthreads_or(mx > LS_BIN_MAX);
        u32 walk = 0;
#pragma unroll
        for (int w = 0; w < LS_NW; w++) walk += s_scan[w];
        heavy |= walk > LS_WALK_MAX * m + 512u;  // (workgroup-uniform) e.g. every key four times: the digit passes are cheaper
        if (heavy && tid == 0) atomicAdd((unsigned long long *)a.stat, 1ull);
        if (!heavy) {
#pragma unroll
            for (int q = 0; q < BPT; q++) {
                s_cnt[tid * BPT + q] = run;
                run += c[q];
            }
            if (tid == LS_NT - 1) s_cnt[NBIN] = run;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < LS_KPT; j++) {
                const u32 i = wbase + j * 64;
                if (i < m) {
                    const u32 bin = (u32)(key[j] >> bshift) & (u32)(NBIN - 1);
                    pos[j] += s_cnt[bin];
                    grp[pos[j]] = key[j];
                    if (PAIRS) s_idx[pos[j]] = (unsigned short)i;
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < LS_KPT; j++) {
                const u32 i = wbase + j * 64;
                if (i < m) {
                    const u32 bin = (u32)(key[j] >> bshift) & (u32)(NBIN - 1);
                    const u32 s = s_cnt[bin], e = s_cnt[bin + 1];
                    u32 r = s;
                    for (u32 t = s; t < e; t++) {
                        const u64 k2 = grp[t];
                        const bool first = PAIRS ? (u32)s_idx[t] < i : t < pos[j];
                        r += (k2 < key[j] || (k2 == key[j] && first)) ? 1u : 0u;
                    }
                    pos[j] = r;
                }
            }
            __syncthreads();  // every walk is over: the final order goes into the same buffer
#pragma unroll
            for (int j = 0; j < LS_KPT; j++) {
                if (wbase + j * 64 < m) {
                    grp[pos[j]] = key[j];
                    if (PAIRS) s_vbuf[0][pos[j]] = val[j];
                }
            }
            __syncthreads();
            for (u32 i = (u32)tid; i < m; i += LS_NT) {
                a.keys[beg + i] = grp[i];
                if (PAIRS) a.vals[beg + i] = s_vbuf[0][i];
            }
            return;
        }
    }
    const u32 lt_lo = lane < 32 ? ((1u << lane) - 1u) : ~0u;
    const u32 lt_hi = lane < 32 ? 0u : ((1u << (lane - 32)) - 1u);
    const int npass = (a.low_bits + RB - 1) / RB;
    int cur = 0;
    for (int p = 0; p < npass; p++) {
        const int shift = RB * p;
        for (int i = tid; i < LS_NW * RADIX / 2; i += LS_NT) reinterpret_cast<u32 *>(&s_wh[0][0])[i] = 0;
        __syncthreads();
        u32 rk[LS_KPT];
#pragma unroll
        for (int j = 0; j < LS_KPT; j++) {
            const u32 d = (u32)(key[j] >> shift) & DMASK;
            u32 plo, phi;
            match_any8(d, plo, phi);
            const u32 pre = s_wh[wave][d];
            rk[j] = pre + (u32)__popc(plo & lt_lo) + (u32)__popc(phi & lt_hi);
            s_wh[wave][d] = (unsigned short)(pre + (u32)__popc(plo) + (u32)__popc(phi));
        }
        __syncthreads();
        u32 cnt = 0;
#pragma unroll
        for (int w = 0; w < LS_NW; w++) {  // thread d: exclusive scan of digit d over the waves
            const u32 cw = s_wh[w][tid];
            s_wh[w][tid] = (unsigned short)cnt;
            cnt += cw;
        }
        u32 total = 0;
        const u32 dex = block_excl_scan_u32<LS_NT>(cnt, s_scan, &total);
        s_dex[tid] = dex;
        __syncthreads();
        u64 *dst = s_buf[cur];
        u32 *vdst = s_vbuf[PAIRS ? cur : 0];
#pragma unroll
        for (int j = 0; j < LS_KPT; j++) {
            const u32 d = (u32)(key[j] >> shift) & DMASK;
            const u32 pos = s_dex[d] + s_wh[wave][d] + rk[j];
            dst[pos] = key[j];
            if (PAIRS) vdst[pos] = val[j];
        }
        __syncthreads();
        if (p + 1 < npass) {
#pragma unroll
            for (int j = 0; j < LS_KPT; j++) {
                key[j] = dst[wbase + j * 64];
                if (PAIRS) val[j] = vdst[wbase + j * 64];
            }
        }
        cur ^= 1;  // (the next pass writes the other buffer: this one is still being read)
    }
    const u64 *res = s_buf[cur ^ 1];
    const u32 *vres = s_vbuf[PAIRS ? (cur ^ 1) : 0];
    for (u32 i = (u32)tid; i < m; i += LS_NT) {
        a.keys[beg + i] = res[i];
        if (PAIRS) a.vals[beg + i] = vres[i];
    }
}
