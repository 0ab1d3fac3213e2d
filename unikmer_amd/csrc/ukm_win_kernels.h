// ukm_win_kernels.h — the three kernels that turn bases into window values, each with its argument struct, its derived
// constants and its comment block: window_kernel (any input; WinArgs), nthash_strip_kernel (Scaled-MinHash sketch; StripArgs) and
// stripwin_kernel (every window of long records; SwArgs).  The host side that chooses among them is in ukm_encode.hip.
// Included by ukm_encode.hip alone, inside its anonymous namespace, after ukm_win_common.h.

struct WinArgs {
    const u8 *bases;
    const u64 *rec_off;  // [n_rec + 1]
    const u64 *out_off;  // [n_rec] exclusive scan of per-record window counts
    u64 n_rec;
    u64 total_bases;
    int k;
    int canonical;
    int circular;
    u64 max_hash;
    u64 *out;
    u64 out_cap;
    u64 *status;  // FILTER only
    u32 *ticket;  // FILTER only
    u64 *result;  // [0] total (FILTER), [1] flags: ENC_FLAG_ILLEGAL = illegal base inside an emitted window
    u64 ntiles;
    const u64 *tile_rec;  // [ntiles + 3]: record containing position min(t * WT, total_bases - 1)
};

// HASH: false = 2-bit codes, true = ntHash.  FILTER: Scaled filter + order-preserving compaction.
// TICKET (FILTER only): tile ids from an atomic counter instead of blockIdx.  The counter is ONE address
// that every workgroup hits: measured 3-4 ns per tile of pure serialisation (0.15 of 0.68 ms per 1e8 bases),
// so the default takes blockIdx and relies on in-order dispatch for look-back liveness, exactly like the
// set-op kernel (watchdog -> flag -> the host re-runs this ticketed instantiation).
template <bool HASH, bool FILTER, bool TICKET = false>
__global__ __launch_bounds__(NT) void window_kernel(WinArgs p) {
    __shared__ __attribute__((aligned(16))) u8 s_b[TBX + 16];
    __shared__ u8 s_info[TBX];                     // low 7 bits: min(bases left in record, 127); bit 7: record length >= k
    __shared__ u32 s_dl[FILTER ? 1 : TBX];         // (bases - windows) in front of the position's record, relative to s_r[2]
    __shared__ u64 s_P[HASH ? TBX + 1 : 1];        // XOR prefixes (ntHash)
    __shared__ u64 s_Q[HASH ? TBX + 1 : 1];
    __shared__ u32 s_pk[HASH ? 1 : TBX / 16 + 4];  // 2-bit packed bases, 16 per word (codes)
    __shared__ u32 s_bad[HASH ? 1 : TBX / 32 + 4]; // illegal-base bit per position (codes)
    __shared__ u64 s_wtot[2 * NWV];
    __shared__ u32 s_cnt[WPT * NWV + 1];
    __shared__ u64 s_r[3];
    __shared__ u64 s_misc[2];
    __shared__ BaseTables s_t;
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    base_tables_init(s_t, tid);  // visible after the first barrier below
    const u64 tile = lb_tile_id<TICKET>(p.ticket, &s_misc[0]);
    const u64 P0 = tile * (u64)WT;
    const int k = p.k;
    // ---- stage bases [P0, P0 + TBX) into LDS -----------------------------------------------------
    {
        const u64 lim = p.total_bases;
        if ((((uintptr_t)p.bases) & 3) == 0) {
            const u32 *b4 = (const u32 *)(p.bases + P0);  // P0 is a multiple of 2048
            for (int i = tid; i * 4 < TBX; i += NT) {
                const u64 g = P0 + (u64)i * 4;
                u32 w = 0;
                if (g + 4 <= lim) w = b4[i];
                else
                    for (int q = 0; q < 4; q++)
                        if (g + q < lim) w |= (u32)p.bases[g + q] << (8 * q);
                ((u32 *)s_b)[i] = w;
            }
        } else {
            for (int i = tid; i < TBX; i += NT) s_b[i] = (P0 + i < lim) ? p.bases[P0 + i] : 0;
        }
    }
    if (tid == 0) {
        s_r[0] = p.tile_rec[tile];          // record of P0
        s_r[1] = p.tile_rec[tile + 2] + 1;  // every position of the tile lies in a record <= this - 1
        // output index of a window = its base position - gap(record), gap = rec_off[r] - out_off[r]
        // (bases minus windows in front of the record; non-decreasing in r); s_r[2] = gap of the first record
        if (!FILTER) { const u64 r0 = p.tile_rec[tile]; s_r[2] = p.rec_off[r0] - p.out_off[r0]; }
    }
    if (!HASH) {
        for (int i = tid; i < TBX / 16 + 4; i += NT) s_pk[i] = 0;
        for (int i = tid; i < TBX / 32 + 4; i += NT) s_bad[i] = 0;
    }
    __syncthreads();

    // ---- phase 1: blocked over positions [tid*PPT, tid*PPT + PPT) -----------------------------------
    {
        const int m0 = tid * PPT;
        const u64 p_first = P0 + (u64)m0;
        const u64 r_first = s_r[0];
        u64 r = 0, rs = 0, re = 0;
        u32 dl = 0;
        const u64 gap0 = FILTER ? 0 : s_r[2];
        bool in_rec = false;
        if (p_first < p.total_bases && p.n_rec > 0) {
            const u64 hi = (s_r[1] + 1 < p.n_rec + 1) ? s_r[1] + 1 : p.n_rec + 1;
            const u64 ub = upper_bound_u64(p.rec_off, r_first, hi, p_first);  // a few steps, L2-resident
            if (ub > 0 && ub <= p.n_rec) {
                r = ub - 1;
                rs = p.rec_off[r];
                re = p.rec_off[r + 1];
                if (!FILTER) dl = (u32)(rs - p.out_off[r] - gap0);
                in_rec = true;
            }
        }
        u64 accP = 0, accQ = 0;
        u64 lp[PPT], lq[PPT];
        u32 pk_w0 = 0, pk_w1 = 0, bad_w0 = 0, bad_w1 = 0;  // codes only
        static_assert(PPT <= 16, "a thread's positions must span at most two packed words");
#pragma unroll
        for (int s = 0; s < PPT; s++) {
            const int m = m0 + s;
            const u64 pos = p_first + (u64)s;
            while (in_rec && pos >= re) {  // advance the record cursor (skips empty records)
                r++;
                if (r >= p.n_rec) { in_rec = false; break; }
                rs = re;
                re = p.rec_off[r + 1];
                if (!FILTER) dl = (u32)(rs - p.out_off[r] - gap0);
            }
            const bool live = in_rec && pos < p.total_bases && m < TBX;
            const u64 rem = live ? re - pos : 0;
            const u32 info = (u32)(rem > 127 ? 127 : rem) | ((live && (re - rs) >= (u64)k) ? 128u : 0u);
            if (m < TBX) {
                s_info[m] = (u8)info;
                if (!FILTER) s_dl[m] = dl;
            }
            const u32 c = (m < TBX) ? s_b[m] : 0;
            if (HASH) {
                // position m contributes ror(seed, m) to P and rol(cseed, m) to Q
                const u32 si = (u32)s_t.lut[c] >> 4;
                accP ^= ror64(s_t.seed[si], (u32)m);
                accQ ^= rol64(s_t.cseed[si], (u32)m);
                lp[s] = accP;
                lq[s] = accQ;
            } else {
                const u32 b = (u32)s_t.lut[c] & 15u;
                // first base of a k-mer is most significant: position m goes to bits [2*(15 - m%16)] of word m/16.
                // A thread's PPT consecutive positions touch at most two words: accumulate in registers and
                // issue one LDS atomic per touched word (not one per position)
                if (m < TBX) {
                    const u32 bits = (b & 3u) << (2 * (15 - (m & 15)));
                    if ((m >> 4) == (m0 >> 4)) pk_w0 |= bits; else pk_w1 |= bits;
                    const u32 bb = (b > 3) ? (1u << (m & 31)) : 0u;
                    if ((m >> 5) == (m0 >> 5)) bad_w0 |= bb; else bad_w1 |= bb;
                }
            }
        }
        if (!HASH) {
            if (pk_w0) atomicOr(&s_pk[m0 >> 4], pk_w0);
            if (pk_w1) atomicOr(&s_pk[(m0 >> 4) + 1], pk_w1);
            if (bad_w0) atomicOr(&s_bad[m0 >> 5], bad_w0);
            if (bad_w1) atomicOr(&s_bad[(m0 >> 5) + 1], bad_w1);
        }
        if (HASH) {
            // block-wide exclusive XOR scan of the per-thread totals
            const u64 iP = wave_incl_xor_scan_u64(accP), iQ = wave_incl_xor_scan_u64(accQ);
            if (lane == 63) { s_wtot[wave] = iP; s_wtot[NWV + wave] = iQ; }
            __syncthreads();
            u64 eP = iP ^ accP, eQ = iQ ^ accQ;
#pragma unroll
            for (int w = 0; w < NWV; w++)
                if (w < wave) { eP ^= s_wtot[w]; eQ ^= s_wtot[NWV + w]; }
            if (tid == 0) { s_P[0] = 0; s_Q[0] = 0; }
#pragma unroll
            for (int s = 0; s < PPT; s++)
                if (m0 + s < TBX) {
                    s_P[m0 + s + 1] = eP ^ lp[s];
                    s_Q[m0 + s + 1] = eQ ^ lq[s];
                }
        }
    }
    __syncthreads();

    // ---- phase 2: striped over windows i = tid + j*NT ---------------------------------------------------
    const u64 out0 = FILTER ? 0 : P0 - s_r[2];
    u64 hv[WPT];
    u32 keep = 0, illegal = 0;
    const u64 kmask = (k == 64) ? ~0ull : ((1ull << k) - 1);
#pragma unroll
    for (int j = 0; j < WPT; j++) {
        const int i = tid + j * NT;
        const u32 info = s_info[i];
        const bool long_enough = (info & 128u) != 0;
        const bool fits = (int)(info & 127u) >= k;
        bool emit = long_enough && fits;
        // the common case is computed unconditionally (no exec-mask branches around it)
        u64 f, rv;
        bool bad = false;
        if (HASH) {
            f = rol64(s_P[i + k] ^ s_P[i], (u32)(i + k - 1));
            rv = ror64(s_Q[i + k] ^ s_Q[i], (u32)i);
        } else {
            // 2k-bit field starting at packed bit offset 2i (big-endian within 32-bit words)
            const int w0 = i >> 4, sh = 2 * (i & 15);
            const u64 hi = ((u64)s_pk[w0] << 32) | s_pk[w0 + 1];
            const u64 lo = ((u64)s_pk[w0 + 2] << 32);
            const u64 x = (hi << sh) | ((lo >> 1) >> (63 - sh));  // 64 bits = 32 bases from position i (sh may be 0)
            f = x >> (64 - 2 * k);
            rv = revcomp2(f, k);
            // any illegal base among positions [i, i+k)?
            const int b0 = i >> 5, bs = i & 31;
            const u64 mlo = ((u64)s_bad[b0 + 1] << 32) | s_bad[b0];
            const u64 mhi = s_bad[b0 + 2];
            const u64 mbits = (mlo >> bs) | ((mhi << 1) << (63 - bs));
            bad = (mbits & kmask) != 0;
        }
        if (long_enough && !fits && p.circular) {  // wrapped window: recompute from the record (k-1 per record)
            const u64 pos = P0 + (u64)i;
            const u64 hi_r = (s_r[1] + 1 < p.n_rec + 1) ? s_r[1] + 1 : p.n_rec + 1;
            const u64 r = upper_bound_u64(p.rec_off, s_r[0], hi_r, pos) - 1;
            const u64 rs = p.rec_off[r], len = p.rec_off[r + 1] - rs;
            const u64 o = pos - rs;
            f = 0; rv = 0; bad = false;
            for (int q = 0; q < k; q++) {
                u64 z = o + (u64)q;
                if (z >= len) z -= len;
                const u32 cc = p.bases[rs + z];
                if (HASH) {
                    const u32 si = (u32)s_t.lut[cc] >> 4;
                    f ^= rol64(s_t.seed[si], (u32)(k - 1 - q));
                    rv ^= rol64(s_t.cseed[si], (u32)q);
                } else {
                    const u32 bb = (u32)s_t.lut[cc] & 15u;
                    if (bb > 3) bad = true;
                    f = (f << 2) | (u64)(bb & 3);
                    rv |= (u64)(3 - (bb & 3)) << (2 * q);
                }
            }
            emit = true;
        }
        if (bad && emit) illegal = 1;
        const u64 v = (p.canonical && rv < f) ? rv : f;
        if (FILTER) {
            hv[j] = v;
            if (emit && v <= p.max_hash) keep |= 1u << j;
        } else if (emit) {
            const u64 oi = out0 + (u64)i - (u64)s_dl[i];
            if (oi < p.out_cap) p.out[oi] = v;
        }
    }
    if (illegal) atomicOr((unsigned long long *)&p.result[1], (unsigned long long)ENC_FLAG_ILLEGAL);

    if (FILTER) {
        // survivors in window order: (round j, wave, lane)
        tile_place_kept<WPT, NWV, TICKET>(keep, tile, p.ntiles, p.status, p.result, s_cnt, &s_misc[1], tid, lane, wave,
                                          [&](int j, u64 pos) { if (pos < p.out_cap) p.out[pos] = hv[j]; });
    }
}

// ---- Scaled-MinHash sketch of reads: per-lane ROLLING ntHash over strips ------------------------------------
// The prefix-XOR kernel above spends ~160 lane-operations per window (per-position prefix words, a block
// scan, two 64-bit variable rotates per window) although with `--scale 1000` only one window in a thousand
// is ever written.  Here every lane rolls the hash along its own strip of L window starts:
//     fwd' = rol(fwd, 1) ^ rol(seed[out], k) ^ seed[in]
//     rev' = ror(rev, 1) ^ ror(seed[comp(out)], 1) ^ rol(seed[comp(in)], k - 1)          
// The hash of a window is a function of its k bytes only, so the rolling runs straight across record
// boundaries of the concatenated base array; whether a window lies inside one record is decided for the few
// values that pass `<= max_hash` (a binary search per CANDIDATE, not per position).  Per step: two byte
// extracts, two 16-byte LDS table reads (tables indexed by the raw byte: no base translation at all), four
// 32-bit funnel shifts, four 3-input XORs, two 32-bit compares: ~16 lane-operations per base.  Bases are read
// straight from global memory, 64 bytes per lane at a time (each lane walks its own strip; a lane's 64-byte
// piece is one cache line, fetched once).  A strip starts cold at its first window start, i.e. it processes
// L + k - 1 bases for L windows.
// Candidates are appended to an LDS list (owner lane, sequence number in the lane), ordered by (lane,
// sequence) = window order with one block scan, validated against the record table, compacted with
// ballots and placed with the library's look-back: the output keeps window order, as the reference's
// iterator does (count.go:361,373-375).  More candidates than the list holds (a tiny --scale, pathological
// repeats) -> flag, and the caller takes the prefix-XOR kernel.
// (ST_NT lanes per tile, ST_CAP candidate list entries per tile: ukm_encode.hip)
constexpr int ST_RND = ST_CAP / ST_NT;   // compaction rounds
constexpr int ST_NWV = ST_NT / 64;

struct StripArgs {
    const u8 *bases;
    const u64 *rec_off;
    u64 n_rec;
    u64 total_bases;
    int k;
    int canonical;
    int L;  // window starts per lane, multiple of 64
    u64 max_hash;
    u64 *out;
    u64 out_cap;
    u64 *status;
    u32 *ticket;
    u64 *result;  // [0] total, [1] flags: ENC_FLAG_OVERFLOW = candidate list overflow
    u64 ntiles;
    const u64 *tile_rec;
};

struct __attribute__((packed, aligned(4))) U4a4 {  // 16 bytes at 4-byte alignment
    u32 x, y, z, w;
};

// n dwords of the base array starting at byte offset `off` (may be negative or run past the end: such
// bytes read as 0).  Fast path: plain vector loads.
template <int N>
__device__ __forceinline__ void strip_load(const u8 *bases, long long off, u64 total, bool active, u32 (&w)[N]) {
    const bool fast = active && off >= 0 && (u64)off + 4ull * N <= total;
    if (fast) {
        const u8 *src = bases + off;
#pragma unroll
        for (int g = 0; g + 4 <= N; g += 4) {
            const U4a4 q = *reinterpret_cast<const U4a4 *>(src + 4 * g);
            w[g] = q.x; w[g + 1] = q.y; w[g + 2] = q.z; w[g + 3] = q.w;
        }
#pragma unroll
        for (int g = N & ~3; g < N; g++) w[g] = *reinterpret_cast<const u32 *>(src + 4 * g);
    } else {
        // byte by byte; the valid byte indices [ilo, ihi) as two ints so that nothing 64-bit is kept per byte
        const long long lo = -off, hi = (long long)total - off;
        const int ilo = lo < 0 ? 0 : (lo > 4 * N ? 4 * N : (int)lo);
        const int ihi = !active || hi < 0 ? 0 : (hi > 4 * N ? 4 * N : (int)hi);
        const u8 *src = bases + off;
#pragma unroll
        for (int g = 0; g < N; g++) {
            u32 x = 0;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (4 * g + q >= ilo && 4 * g + q < ihi) x |= (u32)src[4 * g + q] << (8 * q);
            w[g] = x;
        }
    }
}

template <bool TICKET>
__global__ __launch_bounds__(ST_NT) void nthash_strip_kernel(StripArgs p) {
    __shared__ __attribute__((aligned(16))) uint4 s_tin[256];   // [byte] = { seed, rol(cseed, k-1) }
    __shared__ __attribute__((aligned(16))) uint4 s_tout[256];  // [byte] = { rol(seed, k), ror(cseed, 1) }
    __shared__ u64 s_ch[ST_CAP];   // candidates in arrival order
    __shared__ u32 s_ci[ST_CAP];   // owner lane << 24 | sequence number << 11 | window index in the strip
    __shared__ unsigned short s_ord[ST_CAP];  // window order -> arrival order (an index, so that the list is not copied)
    __shared__ u32 s_base[ST_NT];
    __shared__ u32 s_scan[ST_NWV + 1];
    __shared__ u32 s_cnt[ST_RND * ST_NWV + 1];
    __shared__ u32 s_n;
    __shared__ u64 s_misc[2];
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const int k = p.k, L = p.L;
    {
        const u32 si = (u32)g_byte_table.v[tid] >> 4;  // 0..3 = A C G T/U, 4 = anything else (zero seed)
        const u64 f = si == 0 ? SEED_A : si == 1 ? SEED_C : si == 2 ? SEED_G : si == 3 ? SEED_T : 0ull;
        const u64 cs = si == 0 ? SEED_T : si == 1 ? SEED_G : si == 2 ? SEED_C : si == 3 ? SEED_A : 0ull;
        const u64 a = f, b = rol64(cs, (u32)(k - 1)), c2 = rol64(f, (u32)k), d = ror64(cs, 1);
        s_tin[tid] = make_uint4((u32)a, (u32)(a >> 32), (u32)b, (u32)(b >> 32));
        s_tout[tid] = make_uint4((u32)c2, (u32)(c2 >> 32), (u32)d, (u32)(d >> 32));
        if (tid == 0) s_n = 0;
    }
    const u64 tile = lb_tile_id<TICKET>(p.ticket, &s_misc[0]);
    __syncthreads();
    const u64 P0 = tile * (u64)ST_NT * (u64)L;
    const u64 s0 = P0 + (u64)tid * (u64)L;  // first window start of this lane
    const bool active = s0 < p.total_bases;
    const u32 mh_hi = (u32)(p.max_hash >> 32);
    const bool canon = p.canonical != 0;
    const u32 rmask = canon ? 0u : 0xFFFFFFFFu;  // forward hashes only: the reverse strand never passes the coarse test
    u32 flo = 0, fhi = 0, rlo = 0, rhi = 0;  // fwd / rev hash of the k bases ending at the current position
    u32 myseq = 0;
    const int nsteps = L + k - 1;
    const int kp = (int)((0u - (u32)k) & 3u);  // byte phase of the `out` stream inside its dwords
    for (int c0 = 0; c0 < nsteps; c0 += 64) {
        u32 iw[16], ow[17];
        strip_load<16>(p.bases, (long long)(s0 + (u64)c0), p.total_bases, active, iw);
        // out bytes of this chunk = base[s0 + c0 - k ...]; the dword-aligned window that holds them
        const long long ooff = (long long)(s0 + (u64)c0) - (long long)k;
        strip_load<17>(p.bases, ooff - (long long)kp, p.total_bases, active, ow);
        if (c0 == 0) {
            // a strip starts cold: the first k steps have no outgoing base (byte 0 has a zero table entry)
#pragma unroll
            for (int g = 0; g < 17; g++) {
                const int b0 = 4 * g - kp;        // out-stream step of the dword's first byte
                const int nz = k - b0;            // bytes of this dword that belong to steps < k
                const u32 m = nz <= 0 ? 0xFFFFFFFFu : (nz >= 4 ? 0u : (0xFFFFFFFFu << (8 * nz)));
                ow[g] &= m;
            }
        }
#pragma unroll
        for (int g = 0; g < 16; g++) {
            // the four out bytes of steps 4g .. 4g+3
            const u32 o4 = __builtin_amdgcn_alignbyte(ow[g + 1], ow[g], (u32)kp);
            const u32 i4 = iw[g];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int i = c0 + 4 * g + q;  // step: the base at s0 + i enters
                const uint4 ein = s_tin[(i4 >> (8 * q)) & 0xFFu];
                const uint4 eout = s_tout[(o4 >> (8 * q)) & 0xFFu];
                // fwd = rol(fwd, 1) ^ seed[in] ^ rol(seed[out], k)
                const u32 nflo = xor3(__builtin_amdgcn_alignbit(flo, fhi, 31), ein.x, eout.x);
                const u32 nfhi = xor3(__builtin_amdgcn_alignbit(fhi, flo, 31), ein.y, eout.y);
                // rev = ror(rev, 1) ^ rol(cseed[in], k - 1) ^ ror(cseed[out], 1)
                const u32 nrlo = xor3(__builtin_amdgcn_alignbit(rhi, rlo, 1), ein.z, eout.z);
                const u32 nrhi = xor3(__builtin_amdgcn_alignbit(rlo, rhi, 1), ein.w, eout.w);
                flo = nflo; fhi = nfhi; rlo = nrlo; rhi = nrhi;
                // Coarse test on the high words with ONE vector compare; everything else — also the uniform range
                // check of the step index — only inside the rare hit.  (Written as `hit && i >= k - 1 && i < nsteps`
                // the compiler evaluated the scalar range checks and a short-circuit branch for the second strand on
                // EVERY step: 27 scalar instructions per step against 19 vector ones, and a CU issues one scalar
                // instruction per cycle: the kernel was bound by its scalar unit.)
                const u32 hmin = fhi < (rhi | rmask) ? fhi : (rhi | rmask);
                if (__builtin_expect(hmin <= mh_hi, 0)) {
                    int ii = i;
                    asm volatile("" : "+s"(ii));  // keeps the range check inside the branch
                    if (ii >= k - 1 && ii < nsteps) {
                    const u64 f = ((u64)fhi << 32) | flo, rv = ((u64)rhi << 32) | rlo;
                    const u64 h = (canon && rv < f) ? rv : f;
                    const u32 w = (u32)(i - (k - 1));  // window index inside the strip
                    if (h <= p.max_hash && s0 + (u64)w + (u64)k <= p.total_bases) {
                        const u32 e = atomicAdd(&s_n, 1u);
                        if (e < (u32)ST_CAP) {
                            s_ch[e] = h;
                            s_ci[e] = ((u32)tid << 24) | ((myseq & 0x1FFFu) << 11) | w;
                        }
                        myseq++;
                    }
                    }
                }
            }
        }
    }
    __syncthreads();
    const u32 n_all = s_n;
    const u32 n = n_all < (u32)ST_CAP ? n_all : (u32)ST_CAP;
    if (n_all > (u32)ST_CAP && tid == 0) atomicOr((unsigned long long *)&p.result[1], (unsigned long long)ENC_FLAG_OVERFLOW);
    // window order = (owner lane, sequence number)
    {
        u32 tot;
        const u32 excl = block_excl_scan_u32<ST_NT>(myseq, s_scan, &tot);
        s_base[tid] = excl;
    }
    __syncthreads();
    for (u32 e = (u32)tid; e < n; e += ST_NT) {
        const u32 ci = s_ci[e];
        const u32 owner = ci >> 24, seq = (ci >> 11) & 0x1FFFu, w = ci & 0x7FFu;
        const u32 slot = s_base[owner] + seq;
        (void)w;
        if (slot < (u32)ST_CAP) s_ord[slot] = (unsigned short)e;
    }
    __syncthreads();
    // is the window inside one record?  (records shorter than k never hold one)
    u64 hv[ST_RND];
    u32 keep = 0;
    {
        const u64 r_lo = p.tile_rec[tile];
        u64 r_hi = p.tile_rec[tile + 1] + 2;
        r_hi = r_hi < p.n_rec + 1 ? r_hi : p.n_rec + 1;
#pragma unroll
        for (int m = 0; m < ST_RND; m++) {
            const u32 slot = (u32)tid + (u32)m * ST_NT;
            hv[m] = 0;
            if (slot < n && n_all <= (u32)ST_CAP) {
                const u32 e = s_ord[slot];
                const u32 ci = s_ci[e];
                const u64 pos = P0 + (u64)(ci >> 24) * (u64)L + (u64)(ci & 0x7FFu);
                const u64 ub = upper_bound_u64(p.rec_off, r_lo, r_hi, pos);  // first record starting behind pos
                if (ub > 0 && ub <= p.n_rec && pos + (u64)k <= p.rec_off[ub]) {
                    keep |= 1u << m;
                    hv[m] = s_ch[e];
                }
            }
        }
    }
    tile_place_kept<ST_RND, ST_NWV, TICKET>(keep, tile, p.ntiles, p.status, p.result, s_cnt, &s_misc[1], tid, lane, wave,
                                            [&](int m, u64 pos) { if (pos < p.out_cap) p.out[pos] = hv[m]; });
}

// ---- every window of long records: per-lane rolling 2-bit codes / ntHash over strips ----------------------------
// window_kernel above stages 2048 positions per tile and re-derives every window from per-position prefix
// words: ~45 (codes) to ~160 (ntHash) lane-operations per window, 30 % of the HBM roofline.  For inputs made of
// long records (genomes, contigs: count.go's per-record loop over a chromosome) every lane instead rolls along
// its own strip of L positions:  code' = ((code << 2) | c) & mask,  rc' = (rc >> 2) | ((3 - c) << (2k - 2)),
// or the ntHash recurrence of nthash_strip_kernel.  A lane owns the windows that END inside its strip, so
// step i of the unrolled loop always fills slot i & 15 of the lane's LDS row whatever k is.  Every 16 steps
// the wave turns its 64 rows x 16 values around: eight lanes write one row's 128 bytes with 16-byte stores.
// Neighbouring lanes work 8L bytes apart, so what matters is that every row is one whole, ALIGNED cache line
// of the output (measured: rows that straddle lines cost 2.3 x; on 150-bp reads, k = 31: rows on 128 / 64 / 32 /
// 16 / 8-byte boundaries 0.206 / 0.230 / 0.30 / 0.33 / 0.35 ms per 1e8 windows): every lane starts its strip `sh`
// (< 16) positions early so that the output index of its row starts is a multiple of 16 in the record it starts
// in; the tile's first lane skips what belongs to the previous tile, every wave runs 16 steps longer.
// All record logic (is the window inside one record, where does it go) happens once per row, not per window:
// a row that lies inside one record gets its output index published; a row that touches a record or strip
// boundary (rare for long records) is written by its owner lane value by value.
// Not for circular records; more than SW_REC records under one tile -> flag, the caller runs window_kernel.
// (SW_NT lanes per tile, SW_REC records one tile may touch, the ablation knob SW_ABL: ukm_encode.hip)
constexpr int SW_NWV = SW_NT / 64;
constexpr int SW_B = 16;      // values per row = one 128-byte line
constexpr int SW_ROW = 17;    // u64 per LDS row: 16 values + 1 pad (bank spread)

struct SwArgs {
    const u8 *bases;
    const u64 *rec_off;   // [n_rec + 1]
    const u64 *out_off;   // [n_rec + 1] exclusive scan of the per-record window counts
    u64 n_rec;
    u64 total_bases;
    int k;
    int canonical;
    int L;                // positions per lane, multiple of 64
    u64 *out;
    u64 *result;          // [1] flags: ENC_FLAG_ILLEGAL in an emitted window, ENC_FLAG_OVERFLOW of the record table
    const u64 *tile_rec;  // [ntiles + 3]
    // ukm_count (round 6): the sort that follows wants the 256-bin histogram of digit (value >> fshift) & 255 of everything this
    // launch writes -- counted here (one LDS atomic per value, 256 global atomics per workgroup) it saves the sort's own
    // pre-pass over the values; null: not wanted
    u64 *fhist;
    int fshift;
};

template <bool HASH>
__global__ __launch_bounds__(SW_NT) __attribute__((amdgpu_waves_per_eu(HASH ? 3 : 4, HASH ? 3 : 4))) void stripwin_kernel(SwArgs p) {
    __shared__ __attribute__((aligned(16))) uint4 s_tin[HASH ? 256 : 1];
    __shared__ __attribute__((aligned(16))) uint4 s_tout[HASH ? 256 : 1];
    __shared__ u8 s_lut[HASH ? 1 : 256];
    __shared__ u64 s_ro[SW_REC + 2];
    __shared__ u32 s_gap[SW_REC + 2];  // gap of a record minus the gap of the tile's first record (< tile positions + k per record)
    __shared__ u64 s_row[SW_NWV][64 * SW_ROW];
    __shared__ u64 s_desc[SW_NWV][64];
    __shared__ u32 s_fh[128];  // fhist: two 16-bit counters per word (a tile writes at most SW_NT x L <= 65,535 values: the host checks)
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const int k = p.k, L = p.L;
    if (p.fhist && tid < 128) s_fh[tid] = 0;
    if constexpr (HASH) {
        const u32 si = (u32)g_byte_table.v[tid] >> 4;
        const u64 f = si == 0 ? SEED_A : si == 1 ? SEED_C : si == 2 ? SEED_G : si == 3 ? SEED_T : 0ull;
        const u64 cs = si == 0 ? SEED_T : si == 1 ? SEED_G : si == 2 ? SEED_C : si == 3 ? SEED_A : 0ull;
        const u64 a = f, b = rol64(cs, (u32)(k - 1)), c2 = rol64(f, (u32)k), d = ror64(cs, 1);
        s_tin[tid] = make_uint4((u32)a, (u32)(a >> 32), (u32)b, (u32)(b >> 32));
        s_tout[tid] = make_uint4((u32)c2, (u32)(c2 >> 32), (u32)d, (u32)(d >> 32));
    } else {
        s_lut[tid] = g_byte_table.v[tid] & 0xF;
    }
    const u64 tile = blockIdx.x;
    const u64 TS = (u64)SW_NT * (u64)L;
    const u64 P0 = tile * TS;
    const u64 r0 = p.tile_rec[tile];
    const u64 r1 = p.tile_rec[tile + 1];
    const u64 nr = r1 - r0 + 1;  // records r0 .. r1 may hold positions of the tile
    if (nr > (u64)SW_REC) {
        if (tid == 0) atomicOr((unsigned long long *)&p.result[1], (unsigned long long)ENC_FLAG_OVERFLOW);
        return;
    }
    const u64 gap_first = p.rec_off[r0] - p.out_off[r0];  // (uniform: scalar loads)
    for (u64 j = (u64)tid; j <= nr; j += SW_NT) {
        const u64 ro = p.rec_off[r0 + j];
        s_ro[j] = ro;
        s_gap[j] = (u32)((ro - p.out_off[r0 + j]) - gap_first);
    }
    __syncthreads();
    // output index of the window that ends at e (inside record r) = e + 1 - k - gap[r].  Every lane starts its strip
    // `sh` (< 16) positions in front of its nominal start b = P0 + tid * L so that this index is a multiple of 16 at
    // each of its row starts, FOR THE RECORD THAT HOLDS b: the lane's rows are then whole output lines until it walks
    // into the next record (reads: 8 % of the rows of 64-position strips; one shift per tile, the first version, left
    // every record but the tile's first one at the alignment its gap happens to have).  The boundaries between lanes
    // move with the shifts (s_bnd); the tile's own boundaries stay where they are.
    const u64 b_nom = P0 + (u64)tid * (u64)L;
    u32 sh = 0, jb = 0;
    bool active = b_nom < p.total_bases;
    if (active) {
        active = false;
        u32 lo = 0, hi = (u32)nr + 1;  // first index with s_ro > b_nom (records of length 0 are skipped)
        while (lo < hi) {
            const u32 mid = (lo + hi) >> 1;
            if (s_ro[mid] <= b_nom) lo = mid + 1; else hi = mid;
        }
        if (lo >= 1 && lo <= (u32)nr) {
            active = true;
            jb = lo - 1;
            sh = (u32)(b_nom + 1 - (u64)k - (gap_first + (u64)s_gap[jb])) & (u32)(SW_B - 1);
        }
    }
    u32 *s_bnd = reinterpret_cast<u32 *>(&s_desc[0][0]);  // first END position of every lane, relative to the tile
    s_bnd[tid] = tid == 0 ? 0u : (u32)tid * (u32)L - sh;  // (tid >= 1: L >= 64 > sh)
    __syncthreads();
    const long long s0 = (long long)b_nom - (long long)sh;                  // first END position of this lane's rows
    const u64 e_lo = P0 + (u64)s_bnd[tid];                                  // the lane emits END positions [e_lo, e_hi)
    const u64 e_hi = P0 + (tid == SW_NT - 1 ? TS : (u64)s_bnd[tid + 1]);
    __syncthreads();  // (s_bnd lives in the descriptor words)
    u32 j = 0;
    u64 rec_start = ~0ull, rec_end = 0, gap = 0;
    bool dead = !active;
    if (active) {
        u32 lo = jb + 1;
        if (e_lo < s_ro[jb]) {  // the shift reached into the previous record
            lo = 0;
            u32 hi = jb + 1;
            while (lo < hi) {
                const u32 mid = (lo + hi) >> 1;
                if (s_ro[mid] <= e_lo) lo = mid + 1; else hi = mid;
            }
        }
        if (lo == 0 || lo > (u32)nr) dead = true;
        else { j = lo - 1; rec_start = s_ro[j]; rec_end = s_ro[j + 1]; gap = gap_first + (u64)s_gap[j]; }
        if (dead) { rec_start = ~0ull; rec_end = 0; }
    }
    const bool canon = p.canonical != 0;
    const int WU = k <= 32 ? 32 : 64;     // warm-up steps in front of the strip (>= k)
    const int i_start = 64 - WU;          // step i reads the base at s0 - 64 + i
    // a strip is up to 15 positions longer than L (its own shift, its neighbour's none): the wave runs one more row
    // only if one of its lanes needs it (long records: every lane has the same shift, only the tile's last wave does)
    const bool longer = active && e_hi > (u64)s0 + (u64)L;
    const int nsteps = 64 + L + (__ballot(longer) != 0ull ? SW_B : 0);
    u64 fwd = 0, rc = 0, hist = 0;
    u32 flo = 0, fhi = 0, rlo = 0, rhi = 0;
    const u64 kmask = k >= 32 ? ~0ull : ((1ull << (2 * k)) - 1);
    const u32 rcs = (u32)(2 * k - 2);
    const u32 ipa = (u32)(s0 - 64) & 3u;                    // byte phase of the in / out streams in their dwords
    const u32 opa = (u32)(s0 - 64 - (long long)k) & 3u;
    u64 *row = &s_row[wave][lane * SW_ROW];
    bool illegal = false;
#define SW_NEXT_RECORD()                                                                  \
    do {                                                                                  \
        if (j + 1 >= (u32)nr) { dead = true; rec_start = ~0ull; rec_end = 0; }            \
        else { j++; rec_start = rec_end; rec_end = s_ro[j + 1]; gap = gap_first + (u64)s_gap[j]; } \
    } while (0)
    for (int c0 = 0; c0 < nsteps; c0 += 64) {
        u32 iw[17];
        u32 ow[HASH ? 17 : 1];
        const long long cpos = s0 + (long long)c0 - 64;
        strip_load<17>(p.bases, cpos - (long long)ipa, p.total_bases, active, iw);
        if constexpr (HASH) {
            u32 t17[17];
            strip_load<17>(p.bases, cpos - (long long)k - (long long)opa, p.total_bases, active, t17);
#pragma unroll
            for (int g = 0; g < 17; g++) ow[g] = t17[g];
        }
#pragma unroll
        for (int g = 0; g < 16; g++) {
            if (c0 == 0 && 4 * g < i_start) continue;
            if (c0 + 4 * g >= nsteps) continue;
            u32 o4 = 0;
            if constexpr (HASH) {
                o4 = __builtin_amdgcn_alignbyte(ow[g + 1], ow[g], opa);
                if (c0 == 0) {
                    // cold start: steps < i_start + k have no outgoing base (byte 0 has a zero table entry)
                    const int nz = i_start + k - 4 * g;
                    const u32 m = nz <= 0 ? 0xFFFFFFFFu : (nz >= 4 ? 0u : (0xFFFFFFFFu << (8 * nz)));
                    o4 &= m;
                }
            }
            const u32 i4 = __builtin_amdgcn_alignbyte(iw[g + 1], iw[g], ipa);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                u64 v;
                if constexpr (HASH) {
                    const uint4 ein = s_tin[(i4 >> (8 * q)) & 0xFFu];
                    const uint4 eout = s_tout[(o4 >> (8 * q)) & 0xFFu];
                    const u32 nflo = xor3(__builtin_amdgcn_alignbit(flo, fhi, 31), ein.x, eout.x);
                    const u32 nfhi = xor3(__builtin_amdgcn_alignbit(fhi, flo, 31), ein.y, eout.y);
                    const u32 nrlo = xor3(__builtin_amdgcn_alignbit(rhi, rlo, 1), ein.z, eout.z);
                    const u32 nrhi = xor3(__builtin_amdgcn_alignbit(rlo, rhi, 1), ein.w, eout.w);
                    flo = nflo; fhi = nfhi; rlo = nrlo; rhi = nrhi;
                    const u64 f = ((u64)fhi << 32) | flo, rv = ((u64)rhi << 32) | rlo;
                    v = (canon && rv < f) ? rv : f;
                } else {
                    const u32 e = s_lut[(i4 >> (8 * q)) & 0xFFu];
                    const u32 code = e & 3u;
                    hist = (hist << 1) | (u64)(e >> 2);
                    fwd = ((fwd << 2) | (u64)code) & kmask;
                    rc = (rc >> 2) | ((u64)(code ^ 3u) << rcs);
                    v = (canon && rc < fwd) ? rc : fwd;
                }
                row[(4 * g + q) & (SW_B - 1)] = v;
            }
            __builtin_amdgcn_sched_barrier(0);  // keep the scheduler from hoisting a whole chunk's table reads
            if ((g & 3) == 3 && c0 > 0) {
                // ---- one row: END positions e0 .. e0 + 15 ----
                const long long e0s = s0 + (long long)(c0 - 64 + 4 * (g - 3));
                const u64 e0 = (u64)e0s;
                if (k >= 17) {
                    // A window needs k - 1 >= 16 bases in front of its END inside its record, so a row of 16 END
                    // positions holds valid windows of AT MOST ONE record, and they form one run [qlo, qhi) of the
                    // row: rows cut by a record end, a record start or the strip's own limits go through the same
                    // cooperative 16-byte stores as whole rows, with the run packed into the descriptor (round 3; on
                    // 150-bp reads every wave used to spend every row step in a divergent value-by-value loop).
                    u64 dsc = ~0ull;
                    if (!dead && e0s + (SW_B - 1) >= (long long)e_lo && e0s < (long long)e_hi) {
                        const u64 ef = e0s < (long long)e_lo ? e_lo : e0;  // first END of the row this lane may emit
                        while (!dead && ef >= rec_end) SW_NEXT_RECORD();
                        if (!dead) {
                            u64 lo_e = rec_start + (u64)k - 1;
                            lo_e = lo_e < ef ? ef : lo_e;
                            u64 hi_e = e0 + SW_B;
                            hi_e = hi_e < rec_end ? hi_e : rec_end;
                            hi_e = hi_e < e_hi ? hi_e : e_hi;
                            if (lo_e < hi_e) {
                                const u32 qlo = (u32)(lo_e - e0), qhi = (u32)(hi_e - e0);
                                const u64 d = (e0 + 1 - (u64)k - gap) & ((1ull << 55) - 1);  // output index of slot 0 (mod 2^55)
                                dsc = d | ((u64)qlo << 55) | ((u64)qhi << 59);
                                if (!HASH) {
                                    // illegal base inside an emitted window: history bits 16 - qhi .. 14 - qlo + k
                                    const u32 cntb = (u32)k + qhi - qlo - 1;
                                    const u64 hm = (cntb >= 64 ? ~0ull : ((1ull << cntb) - 1)) << (SW_B - qhi);
                                    if ((hist & hm) != 0) illegal = true;
                                }
                            }
                        }
                    }
                    s_desc[wave][lane] = dsc;
                } else {
                bool ok = false;
                if (!dead && e0s >= (long long)e_lo) {
                    while (!dead && e0 >= rec_end) SW_NEXT_RECORD();
                    ok = !dead && e0 + (SW_B - 1) < rec_end && e0 + (SW_B - 1) < e_hi && e0 + 1 >= rec_start + (u64)k;
                }
                s_desc[wave][lane] = ok ? (((e0 + 1 - (u64)k - gap) & ((1ull << 55) - 1)) | ((u64)SW_B << 59)) : ~0ull;
                if (!HASH && ok && (hist & ((1ull << (k + SW_B - 1)) - 1)) != 0) illegal = true;
                if (!ok && !dead && e0s + (SW_B - 1) >= (long long)e_lo && e0s < (long long)e_hi) {
                    // k <= 16: a row can hold windows of several records: the owner writes what is valid, value by value
                    for (int q = 0; q < SW_B; q++) {
                        const long long es = e0s + q;
                        if (es < (long long)e_lo || es >= (long long)e_hi) continue;
                        const u64 e = (u64)es;
                        while (!dead && e >= rec_end) SW_NEXT_RECORD();
                        if (!dead && e + 1 >= rec_start + (u64)k) {
                            p.out[e + 1 - (u64)k - gap] = row[q];
                            if (!HASH && ((hist >> (SW_B - 1 - q)) & ((1ull << k) - 1)) != 0) illegal = true;
                        }
                    }
                }
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int m = 0; m < 8; m++) {
                    const int strip = m * 8 + (lane >> 3), pr = lane & 7;
                    const u64 dd = s_desc[wave][strip];
                    if (dd != ~0ull && (SW_ABL != 1 || dd == 12345ull)) {
                        // descriptor: output index of slot 0 (55 bits) | first valid slot (4 bits) | end of the run (5 bits)
                        const u32 qlo = (u32)(dd >> 55) & 15u, qhi = (u32)(dd >> 59);
                        const u32 q0 = 2u * (u32)pr, q1 = q0 + 1;
                        const bool w0 = q0 >= qlo && q0 < qhi, w1 = q1 >= qlo && q1 < qhi;
                        const u64 *src = &s_row[wave][strip * SW_ROW + 2 * pr];
                        const u64 v0 = src[0], v1 = src[1];
                        // (each slot's index is reduced on its own: slot 0 of a row that starts in front of its
                        //  record's first window has a "negative" index, and -1 + 1 must come out as 0)
                        const u64 i0 = (dd + q0) & ((1ull << 55) - 1), i1 = (dd + q1) & ((1ull << 55) - 1);
                        if (w0 && w1) {
                            U4a4 st;
                            st.x = (u32)v0; st.y = (u32)(v0 >> 32); st.z = (u32)v1; st.w = (u32)(v1 >> 32);
                            *reinterpret_cast<U4a4 *>(p.out + i0) = st;
                        } else if (w0) {
                            p.out[i0] = v0;
                        } else if (w1) {
                            p.out[i1] = v1;
                        }
                        if (p.fhist) {  // (uniform)
                            const u32 d0 = (u32)(v0 >> p.fshift) & 255u, d1 = (u32)(v1 >> p.fshift) & 255u;
                            if (w0) atomicAdd(&s_fh[d0 >> 1], (d0 & 1u) ? 65536u : 1u);
                            if (w1) atomicAdd(&s_fh[d1 >> 1], (d1 & 1u) ? 65536u : 1u);
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
#undef SW_NEXT_RECORD
    if (!HASH && illegal) atomicOr((unsigned long long *)&p.result[1], (unsigned long long)ENC_FLAG_ILLEGAL);
    if (p.fhist) {
        __syncthreads();
        if (tid < 128) {
            const u32 w = s_fh[tid];
            if (w & 0xFFFFu) atomicAdd((unsigned long long *)&p.fhist[2 * tid], (unsigned long long)(w & 0xFFFFu));
            if (w >> 16) atomicAdd((unsigned long long *)&p.fhist[2 * tid + 1], (unsigned long long)(w >> 16));
        }
    }
}
