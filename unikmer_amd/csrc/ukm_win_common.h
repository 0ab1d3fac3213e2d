// ukm_win_common.h — what the window kernels share: the tile constants, the base / seed tables, the flags of result word
// [1], the small device helpers (rotates, upper bound, the wave's XOR scan, revcomp), the ordered compaction that ends the
// three filtering kernels (tile_place_kept), and the two one-thread-per-item kernels window_count_kernel and
// tile_first_rec_kernel.
// Included by ukm_encode.hip alone, inside its anonymous namespace, in front of ukm_win_kernels.h and ukm_win_minimizer.h.

// (ENC_NT, ENC_WT and the other build knobs and table sizes of the unit: the block at the head of ukm_encode.hip)
constexpr int NT = ENC_NT;
constexpr int WT = ENC_WT;      // window start positions per tile
constexpr int TBX = WT + 64;    // base positions staged per tile (k <= 64)
constexpr int WPT = WT / NT;    // windows per thread (striped)
constexpr int PPT = (TBX + NT - 1) / NT;  // positions per thread in the blocked phase (NT * PPT >= TBX)
constexpr int NWV = NT / 64;

// kmers v0.1.0 base table; 4 = illegal base
constexpr u32 base2bit(u32 c) {
    switch (c) {
    case 'A': case 'a': case 'N': case 'n': case 'M': case 'm': case 'V': case 'v':
    case 'H': case 'h': case 'R': case 'r': case 'D': case 'd': case 'W': case 'w': return 0;
    case 'C': case 'c': case 'S': case 's': case 'B': case 'b': case 'Y': case 'y': return 1;
    case 'G': case 'g': case 'K': case 'k': return 2;
    case 'T': case 't': case 'U': case 'u': return 3;
    default: return 4;
    }
}

#define SEED_A 0x3c8bfbb395c60474ULL
#define SEED_C 0x3193c18562a02b4cULL
#define SEED_G 0x20323ed082572324ULL
#define SEED_T 0x295549f54be24456ULL

// a ^ b ^ c in one instruction (gfx950's three-input v_bitop3_b32, truth table 0x96)
__device__ __forceinline__ u32 xor3(u32 a, u32 b, u32 c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }

// branch-free rotates: for s = 0 both shifts are by 0 and x | x = x
__device__ __forceinline__ u64 rol64(u64 x, u32 s) { return (x << (s & 63)) | (x >> ((0u - s) & 63)); }
__device__ __forceinline__ u64 ror64(u64 x, u32 s) { return (x >> (s & 63)) | (x << ((0u - s) & 63)); }

// The switches above compile to chains of exec-mask branches (measured: 2050 SALU + 1100 VALU
// instructions per wave per tile, instruction-issue bound).  Every workgroup therefore builds a
// 256-entry byte table once (one entry per thread) and the per-base work becomes LDS lookups:
// low nibble = 2-bit code (4 = illegal base), high nibble = ntHash seed index (A0 C1 G2 T3, 4 = the
// zero seed of every other byte); seeds come from two 5-entry tables (forward / complement).
constexpr u32 nt_index(u32 c) {
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': case 'U': case 'u': return 3;
    default: return 4;
    }
}
struct ByteTable {
    u8 v[256];
};
constexpr ByteTable make_byte_table() {
    ByteTable t{};
    for (u32 c = 0; c < 256; c++) t.v[c] = (u8)(base2bit(c) | (nt_index(c) << 4));
    return t;
}
__device__ const ByteTable g_byte_table = make_byte_table();  // built at compile time

struct BaseTables {
    u8 lut[256];
    u64 seed[8];   // [0..4] forward seeds
    u64 cseed[8];  // [0..4] seeds of the complement
};
__device__ __forceinline__ void base_tables_init(BaseTables &t, int tid) {
    static_assert(NT >= 256, "one table entry per thread");
    if (tid < 256) t.lut[tid] = g_byte_table.v[tid];
    if (tid < 5) {
        const u64 f = tid == 0 ? SEED_A : tid == 1 ? SEED_C : tid == 2 ? SEED_G : tid == 3 ? SEED_T : 0ull;
        const u64 c = tid == 0 ? SEED_T : tid == 1 ? SEED_G : tid == 2 ? SEED_C : tid == 3 ? SEED_A : 0ull;
        t.seed[tid] = f;
        t.cseed[tid] = c;
    }
}

enum : u64 { ENC_FLAG_ILLEGAL = 1, ENC_FLAG_TIMEOUT = 2, ENC_FLAG_OVERFLOW = 4 };  // result word [1] of every kernel here

// cnt[n_rec] = 0, so the exclusive scan over n_rec + 1 entries ends with the total
__global__ void window_count_kernel(const u64 *rec_off, u64 n_rec, int k, int circular, u64 *cnt) {
    u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_rec) return;
    if (r == n_rec) { cnt[r] = 0; return; }
    u64 len = rec_off[r + 1] - rec_off[r];
    cnt[r] = (len < (u64)k) ? 0 : (circular ? len : len - (u64)k + 1);
}

// first index i in [lo, hi) with a[i] > x
__device__ __forceinline__ u64 upper_bound_u64(const u64 *a, u64 lo, u64 hi, u64 x) {
    while (lo < hi) {
        u64 mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One thread per tile boundary: the record that contains the tile's first position.  Doing the
// two ~27-step binary searches inside the tile kernel stalled every workgroup for ~25 us.
__global__ void tile_first_rec_kernel(const u64 *rec_off, u64 n_rec, u64 total_bases, u64 ntiles, u64 tile_size,
                                      u64 *tile_rec) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles + 3) return;
    u64 pos = t * tile_size;
    if (pos > total_bases - 1) pos = total_bases - 1;
    tile_rec[t] = upper_bound_u64(rec_off, 0, n_rec + 1, pos) - 1;
}

// The ordered compaction that ends window_kernel<.., FILTER>, nthash_strip_kernel and minimizer_kernel.  Every thread of
// the NW waves holds R candidates, candidate j of thread tid being item tid + j * (64 * NW) of the tile; bit j of `keep`
// says that it survived.  Survivors keep the tile's item order (round j, wave, lane): ballot ranks per round, a 64-lane scan
// of the R * NW per-(round, wave) counts in s_cnt[R * NW + 1], the tile's base from the library's look-back (lb_tile_base;
// `slot` is its LDS word), then store(j, position) for every survivor -- the store checks out_cap itself.  The last tile
// writes the total to result[0].
template <int R, int NW, bool TICKET, typename Store>
__device__ __forceinline__ void tile_place_kept(u32 keep, u64 tile, u64 ntiles, u64 *status, u64 *result, u32 *s_cnt,
                                                u64 *slot, int tid, int lane, int wave, Store store) {
    static_assert(R * NW <= 64, "one lane per (round, wave) count");
    u32 before[R];
#pragma unroll
    for (int j = 0; j < R; j++) {
        const u64 m = __ballot((keep >> j) & 1u);
        before[j] = (u32)__popcll(m & ((1ull << lane) - 1));
        if (lane == 0) s_cnt[j * NW + wave] = (u32)__popcll(m);
    }
    __syncthreads();
    if (tid < 64) {
        constexpr int NG = R * NW;
        const u32 c = lane < NG ? s_cnt[lane] : 0;
        const u32 incl = wave_incl_scan_u32(c);
        if (lane < NG) s_cnt[lane] = incl - c;
        if (lane == 63) s_cnt[NG] = incl;
    }
    __syncthreads();
    const u32 tile_total = s_cnt[R * NW];
    const u64 base = lb_tile_base<TICKET>(status, tile, (u64)tile_total, &result[1], ENC_FLAG_TIMEOUT, slot, tid, lane);
#pragma unroll
    for (int j = 0; j < R; j++)
        if ((keep >> j) & 1u) store(j, base + s_cnt[j * NW + wave] + before[j]);
    if (tid == 0 && tile == ntiles - 1) result[0] = base + tile_total;
}

// 64-bit XOR inclusive scan across the wave (DPP row shifts / broadcasts, cf. wave_incl_scan_u32)
__device__ __forceinline__ u32 dpp_xor_step(u32 v, const int ctrl_id) {
    switch (ctrl_id) {
    case 0: return v ^ (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);
    case 1: return v ^ (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);
    case 2: return v ^ (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);
    case 3: return v ^ (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);
    case 4: return v ^ (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);
    default: return v ^ (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);
    }
}
__device__ __forceinline__ u64 wave_incl_xor_scan_u64(u64 v) {
    u32 lo = (u32)v, hi = (u32)(v >> 32);
#pragma unroll
    for (int s = 0; s < 6; s++) { lo = dpp_xor_step(lo, s); hi = dpp_xor_step(hi, s); }
    return ((u64)hi << 32) | lo;
}

// reverse the 2-bit groups of the low 2k bits of ~code (revcomp of kmers v0.1.0)
__device__ __forceinline__ u64 revcomp2(u64 code, int k) {
    u64 x = ~code;
    x = ((u64)__builtin_bitreverse32((u32)x) << 32) | (u64)__builtin_bitreverse32((u32)(x >> 32));  // bit reversal
    x = ((x & 0xAAAAAAAAAAAAAAAAull) >> 1) | ((x & 0x5555555555555555ull) << 1);                     // restore pair order
    return x >> (64 - 2 * k);
}
