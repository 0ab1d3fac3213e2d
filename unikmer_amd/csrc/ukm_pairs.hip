// ukm_pairs.hip — ukm_pair_counts: how many distinct codes every two of many streams share, as one call.
//
// The formulation is a bit matrix, so the cost does not depend on how much the streams overlap:
//   1. the records of all streams as (code, stream index), sorted by code (ukm_dev_sort on the tagged concatenation);
//   2. a column = the rank of a distinct code in that sequence (run heads, one exclusive scan); columns are walked in blocks
//      of W consecutive columns (ukm_pairs.h: plan_blocks), each a contiguous range of the sorted records;
//   3. per block: zero the bit matrix B[stream][column - block start], set its bits (atomicOr on 32-bit words: OR commutes),
//      then pair_popc_kernel adds popc(B[i][w] & B[j][w]) over the block's words to C[i][j] (64-bit atomicAdd: integer
//      addition commutes) -- a binary B x B^T, tiled like a GEMM;
//   4. out_sizes[j] = the popcount of row j, summed over the blocks.
// The plain arithmetic (plan, stride, tile maps, grid checks) is ukm_pairs.h.
#include <algorithm>
#include <vector>

#include "ukm_internal.h"
#include "ukm_pairs.h"

using namespace ukm_pairs;

namespace {

constexpr int NT = 256;
// LDS image of one side of a K tile: word-major, lds[w][position], 64 positions and 4 words of padding per word row, so
// that the 16-byte rows of a 4 x 4 register transpose land on different banks (68 = 4 mod 64) and every read stays 16-byte
// aligned (272 bytes per word row).
constexpr u32 LDS_ROW = TILE + 4;
static_assert(TILE == 64 && KT_WORDS == 64 && NT == 256, "one 4 x 4 block of (row, word) per thread and side fills a K tile; 16 x 16 threads own 4 x 4 pairs each");
static_assert((LDS_ROW * 4) % 16 == 0, "16-byte LDS rows");

// tags[p] = the stream record p of the concatenation came from: the last i with off[i] <= p
__global__ __launch_bounds__(NT) void pair_tag_kernel(const u64 *off, u32 nstreams, u64 n, u32 *tags) {
    const u64 stride = (u64)gridDim.x * NT;
    for (u64 p = (u64)blockIdx.x * NT + threadIdx.x; p < n; p += stride) {
        u32 lo = 0, hi = nstreams - 1;
        while (lo < hi) {
            const u32 mid = lo + (hi - lo + 1) / 2;
            if (off[mid] <= p) lo = mid;
            else hi = mid - 1;
        }
        tags[p] = lo;
    }
}

// head[p] = 1 where a run of equal codes begins, head[n] = 0: the exclusive scan e of these n + 1 words gives record p the
// column e[p + 1] - 1, and e[n] is the number of columns
__global__ __launch_bounds__(NT) void pair_heads_kernel(const u64 *keys, u64 n, u64 *head) {
    const u64 stride = (u64)gridDim.x * NT;
    for (u64 p = (u64)blockIdx.x * NT + threadIdx.x; p <= n; p += stride) head[p] = p < n && (p == 0 || keys[p] != keys[p - 1]) ? 1 : 0;
}

// starts[b] = the first record whose column is >= b * w, b = 0 .. nblocks (starts[nblocks] = n)
__global__ __launch_bounds__(NT) void pair_block_starts_kernel(const u64 *e, u64 n, u64 w, u64 nblocks, u64 *starts) {
    const u64 b = (u64)blockIdx.x * NT + threadIdx.x;
    if (b > nblocks) return;
    const u64 want = b * w + 1;  // column c >= b * w  <=>  e[p + 1] >= b * w + 1
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (e[mid + 1] >= want) hi = mid;
        else lo = mid + 1;
    }
    starts[b] = lo;
}

// bit (stream, column - c0) of the block's matrix for the records [p0, p1); a code repeated inside a stream sets its bit again
__global__ __launch_bounds__(NT) void pair_setbits_kernel(const u32 *tags, const u64 *e, u64 p0, u64 p1, u64 c0, u64 cols, u32 nstreams,
                                                          u32 stride, u32 *bm) {
    const u64 step = (u64)gridDim.x * NT;
    for (u64 p = p0 + (u64)blockIdx.x * NT + threadIdx.x; p < p1; p += step) {
        const u64 c = e[p + 1] - 1 - c0;
        const u32 s = tags[p];
        if (c < cols && s < nstreams) atomicOr(&bm[(u64)s * stride + (c >> 5)], 1u << (c & 31));
    }
}

// sizes[s] += the set bits of row s: one workgroup per row, the only writer of sizes[s] in this launch
__global__ __launch_bounds__(NT) void pair_rowpop_kernel(const u32 *bm, u32 stride, u32 words, u64 *sizes) {
    __shared__ u32 s_part[NT / 64];
    const uint4 *row = reinterpret_cast<const uint4 *>(bm + (u64)blockIdx.x * stride);
    u32 v = 0;
    for (u32 q = threadIdx.x; q < words / 4; q += NT) {
        const uint4 x = row[q];
        v += __popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w);
    }
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 t = 0;
        for (int i = 0; i < NT / 64; i++) t += s_part[i];
        sizes[blockIdx.x] += t;
    }
}

// The hot path.  A workgroup owns the tile (ti, tj) of 64 x 64 stream pairs and kt_per_slice K tiles of the block's words.
// Position p of a side's LDS image holds stream (p >> 2) + 16 * (p & 3) of the tile, so that
//   * a thread (ty, tx) reads its four rows and its four columns of word w as ONE 16-byte LDS read each: positions
//     4 ty .. 4 ty + 3 are rows ty, ty + 16, ty + 32, ty + 48 (a broadcast over the 16 tx of a row of threads; the 16
//     column reads of a lane group are 256 contiguous bytes, every bank once);
//   * for a fixed accumulator the 16 tx lanes add to 16 consecutive 64-bit counts: 128-byte segments for the atomics.
// Each pair-word costs one v_and and one v_bcnt_u32_b32 with its accumulate operand; 16 of them per 32 bytes read from LDS.
// The next K tile's global loads are issued before the current one is computed.
template <bool TRI>
__global__ __launch_bounds__(NT) void pair_popc_kernel(const u32 *__restrict__ bm, u32 stride, u32 ntiles, u32 nt_cols, u32 ktiles,
                                                       u32 kt_per_slice, u64 *C, u32 nrows, u32 nstreams) {
    __shared__ __attribute__((aligned(16))) u32 s_i[KT_WORDS * LDS_ROW];
    __shared__ __attribute__((aligned(16))) u32 s_j[KT_WORDS * LDS_ROW];
    const u32 tile = blockIdx.x % ntiles, slice = blockIdx.x / ntiles;
    u32 ti, tj;
    if (TRI) tri_tile(tile, nt_cols, &ti, &tj);
    else rect_tile(tile, nt_cols, &ti, &tj);
    const u32 kt0 = slice * kt_per_slice;
    const u32 kt1 = min(kt0 + kt_per_slice, ktiles);
    const u32 tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    // loading role: rows ty, ty + 16, ty + 32, ty + 48 of each side, words 4 tx .. 4 tx + 3 of the K tile (coalesced along words)
    const u32 *gi = bm + (u64)(ti * TILE + ty) * stride + 4 * tx;
    const u32 *gj = bm + (u64)(tj * TILE + ty) * stride + 4 * tx;
    uint4 ri[4], rj[4];
    auto load = [&](u32 kt) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            ri[q] = *reinterpret_cast<const uint4 *>(gi + (u64)(16 * q) * stride + (u64)kt * KT_WORDS);
            rj[q] = *reinterpret_cast<const uint4 *>(gj + (u64)(16 * q) * stride + (u64)kt * KT_WORDS);
        }
    };
    u32 acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[r][c] = 0;
    if (kt0 < kt1) load(kt0);
    for (u32 kt = kt0; kt < kt1; kt++) {
        __syncthreads();  // the reads of the previous K tile are done
        // 4 x 4 transpose in registers: word 4 tx + e of the four rows becomes one 16-byte row at positions 4 ty .. 4 ty + 3
        uint4 *wi = reinterpret_cast<uint4 *>(s_i + (4 * tx) * LDS_ROW + 4 * ty);
        uint4 *wj = reinterpret_cast<uint4 *>(s_j + (4 * tx) * LDS_ROW + 4 * ty);
        wi[0 * (LDS_ROW / 4)] = make_uint4(ri[0].x, ri[1].x, ri[2].x, ri[3].x);
        wi[1 * (LDS_ROW / 4)] = make_uint4(ri[0].y, ri[1].y, ri[2].y, ri[3].y);
        wi[2 * (LDS_ROW / 4)] = make_uint4(ri[0].z, ri[1].z, ri[2].z, ri[3].z);
        wi[3 * (LDS_ROW / 4)] = make_uint4(ri[0].w, ri[1].w, ri[2].w, ri[3].w);
        wj[0 * (LDS_ROW / 4)] = make_uint4(rj[0].x, rj[1].x, rj[2].x, rj[3].x);
        wj[1 * (LDS_ROW / 4)] = make_uint4(rj[0].y, rj[1].y, rj[2].y, rj[3].y);
        wj[2 * (LDS_ROW / 4)] = make_uint4(rj[0].z, rj[1].z, rj[2].z, rj[3].z);
        wj[3 * (LDS_ROW / 4)] = make_uint4(rj[0].w, rj[1].w, rj[2].w, rj[3].w);
        __syncthreads();
        if (kt + 1 < kt1) load(kt + 1);
        const uint4 *ai = reinterpret_cast<const uint4 *>(s_i) + ty;
        const uint4 *bj = reinterpret_cast<const uint4 *>(s_j) + tx;
        // One word row per trip: 2 LDS reads, 16 v_and, 16 v_bcnt with the sum as accumulate operand.  Unrolled, the compiler
        // regroups the sums of several rows into three-operand adds and the popcounts lose that operand (2.5 instructions per
        // pair-word instead of 2, and 146 registers instead of 120); the read latency is covered by the other waves of the SIMD.
#pragma unroll 1
        for (u32 w = 0; w < KT_WORDS; w++) {
            const uint4 a = ai[w * (LDS_ROW / 4)];
            const uint4 b = bj[w * (LDS_ROW / 4)];
            const u32 av[4] = {a.x, a.y, a.z, a.w};
            const u32 bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) acc[r][c] += __popc(av[r] & bv[c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const u32 i = ti * TILE + ty + 16 * r;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const u32 j = tj * TILE + tx + 16 * c;
            if (i < nrows && j < nstreams && acc[r][c])
                atomicAdd(reinterpret_cast<unsigned long long *>(C) + (u64)i * nstreams + j, (unsigned long long)acc[r][c]);
        }
    }
}

// the triangle schedule wrote the tiles with tj >= ti: C[i][j] = C[j][i] for i > j
__global__ __launch_bounds__(NT) void pair_mirror_kernel(u64 *C, u64 n) {
    const u64 total = n * n, step = (u64)gridDim.x * NT;
    for (u64 x = (u64)blockIdx.x * NT + threadIdx.x; x < total; x += step) {
        const u64 i = x / n, j = x % n;
        if (i > j) C[x] = C[j * n + i];
    }
}

unsigned grid_for(const ukm_ctx *c, u64 n) { return (unsigned)std::max<u64>(1, std::min<u64>((n + NT - 1) / NT, (u64)c->num_cu * 16)); }

// four events of the call's own: [0, 1] around a step, [2, 3] around the pair kernel of a block
struct StepEvents {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    int create() {
        for (auto &x : e) UKM_HIP(hipEventCreate(&x));
        return UKM_OK;
    }
    ~StepEvents() {
        for (auto x : e)
            if (x) (void)hipEventDestroy(x);
    }
    // the time between two recorded events, in microseconds; waits for the second
    static int us(hipEvent_t a, hipEvent_t b, double *out) {
        float ms = 0.f;
        UKM_HIP(hipEventSynchronize(b));
        UKM_HIP(hipEventElapsedTime(&ms, a, b));
        *out = (double)ms * 1000.0;
        return UKM_OK;
    }
};

int pair_counts_body(ukm_ctx *c, const uint64_t *const *keys, const uint64_t *lens, u32 nstreams, u32 nrows, u64 *C, u64 *sizes) {
    StepEvents ev;
    UKM_TRY(ev.create());
    const bool tri = nrows == nstreams;
    UKM_HIP(hipMemsetAsync(C, 0, (size_t)nrows * nstreams * sizeof(u64), c->stream));
    UKM_HIP(hipMemsetAsync(sizes, 0, (size_t)nstreams * sizeof(u64), c->stream));
    std::vector<u64> off((size_t)nstreams + 1, 0);
    for (u32 i = 0; i < nstreams; i++) {
        if (lens[i] && !keys[i]) UKM_FAIL(UKM_ERR_INVALID, "ukm_pair_counts: stream %u: keys is NULL", i);
        off[i + 1] = off[i] + lens[i];
    }
    const u64 n = off[nstreams];
    c->stat_pair_columns = c->stat_pair_blocks = 0;
    c->stat_pair_sort_us = c->stat_pair_bits_us = c->stat_pair_kernel_us = 0;
    c->kernel_ms_sum = 0.f;
    c->kernel_ms_sum_valid = true;
    if (n == 0) return UKM_OK;

    // ---- step 1: (code, stream) records sorted by code ----
    (void)hipEventRecord(ev.e[0], c->stream);
    u64 *k = nullptr, *off_dev = nullptr, *head = nullptr, *e = nullptr;
    u32 *tags = nullptr;
    UKM_TRY(ws_alloc_t(c, n, &k));
    UKM_TRY(ws_alloc_t(c, n, &tags));
    UKM_TRY(ws_alloc_t(c, (size_t)nstreams + 1, &off_dev));
    for (u32 i = 0; i < nstreams; i++)  // host or device, at any 8-byte alignment
        if (lens[i]) UKM_HIP(hipMemcpyAsync(k + off[i], keys[i], lens[i] * sizeof(u64), hipMemcpyDefault, c->stream));
    UKM_HIP(hipMemcpyAsync(off_dev, off.data(), off.size() * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(pair_tag_kernel, dim3(grid_for(c, n)), dim3(NT), 0, c->stream, off_dev, nstreams, n, tags);
    UKM_HIP(hipGetLastError());
    {
        WsMark mark = ws_mark(c);
        const int rc = ukm_dev_sort(c, k, tags, n, 64);
        ws_release(c, mark);
        UKM_TRY(rc);
    }
    // ---- step 2: columns ----
    UKM_TRY(ws_alloc_t(c, n + 1, &head));
    UKM_TRY(ws_alloc_t(c, n + 1, &e));
    hipLaunchKernelGGL(pair_heads_kernel, dim3(grid_for(c, n + 1)), dim3(NT), 0, c->stream, k, n, head);
    UKM_HIP(hipGetLastError());
    UKM_TRY(ukm_dev_exclusive_scan_u64(c, head, e, n + 1, nullptr));
    u64 ncols = 0;
    UKM_TRY(ukm_read_u64(c, e + n, &ncols));
    (void)hipEventRecord(ev.e[1], c->stream);
    const Plan plan = plan_blocks(ncols, nstreams, ukm_env_int(c, "UKM_PAIR_BLOCK_COLS", 0));
    if (ncols == 0 || ncols > n) UKM_FAIL(UKM_ERR_HIP, "ukm_pair_counts: %llu columns from %llu records", (unsigned long long)ncols, (unsigned long long)n);
    if (!grids_ok(nstreams, nrows, plan.alloc_cols) || (plan.nblocks + 1 + NT - 1) / NT > MAX_GRID)
        UKM_FAIL(UKM_ERR_INVALID, "ukm_pair_counts: %llu column blocks of %llu columns in one call", (unsigned long long)plan.nblocks, (unsigned long long)plan.w);
    c->stat_pair_columns = ncols;
    c->stat_pair_blocks = plan.nblocks;
    u64 *starts_dev = nullptr;
    UKM_TRY(ws_alloc_t(c, plan.nblocks + 1, &starts_dev));
    hipLaunchKernelGGL(pair_block_starts_kernel, dim3((unsigned)((plan.nblocks + 1 + NT - 1) / NT)), dim3(NT), 0, c->stream, e, n, plan.w, plan.nblocks, starts_dev);
    UKM_HIP(hipGetLastError());
    std::vector<u64> starts(plan.nblocks + 1);
    UKM_HIP(hipMemcpyAsync(starts.data(), starts_dev, starts.size() * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    UKM_HIP(hipStreamSynchronize(c->stream));
    double us = 0;
    UKM_TRY(StepEvents::us(ev.e[0], ev.e[1], &us));
    c->stat_pair_sort_us = (u64)us;

    // ---- step 3: block by block ----
    const u32 stride = (u32)row_stride_words(plan.alloc_cols);
    const size_t bm_bytes = (size_t)bitmap_bytes(nstreams, plan.alloc_cols);
    u32 *bm = nullptr;
    UKM_TRY(ws_alloc(c, bm_bytes, (void **)&bm));
    const u32 nt_cols = tiles_of(nstreams);
    const u32 ntiles = (u32)tile_count(nrows, nstreams);
    double bits_us = 0, kernel_us = 0;
    for (u64 b = 0; b < plan.nblocks; b++) {
        const u64 c0 = plan.begin(b), cols = plan.end(b, ncols) - c0;
        const u64 p0 = starts[b], p1 = starts[b + 1];
        if (p0 > p1 || p1 > n || cols == 0 || cols > plan.alloc_cols) UKM_FAIL(UKM_ERR_HIP, "ukm_pair_counts: block %llu out of range", (unsigned long long)b);
        (void)hipEventRecord(ev.e[0], c->stream);
        UKM_HIP(hipMemsetAsync(bm, 0, bm_bytes, c->stream));
        hipLaunchKernelGGL(pair_setbits_kernel, dim3(grid_for(c, p1 - p0)), dim3(NT), 0, c->stream, tags, e, p0, p1, c0, cols, nstreams, stride, bm);
        UKM_HIP(hipGetLastError());
        (void)hipEventRecord(ev.e[1], c->stream);
        const u32 ktiles = (u32)((cols + KT_COLS - 1) / KT_COLS);
        const KSplit ks = ksplit(ntiles, ktiles);
        const dim3 grid((unsigned)((u64)ntiles * ks.nslices));
        (void)hipEventRecord(ev.e[2], c->stream);
        if (tri) hipLaunchKernelGGL(pair_popc_kernel<true>, grid, dim3(NT), 0, c->stream, bm, stride, ntiles, nt_cols, ktiles, ks.kt_per_slice, C, nrows, nstreams);
        else hipLaunchKernelGGL(pair_popc_kernel<false>, grid, dim3(NT), 0, c->stream, bm, stride, ntiles, nt_cols, ktiles, ks.kt_per_slice, C, nrows, nstreams);
        UKM_HIP(hipGetLastError());
        (void)hipEventRecord(ev.e[3], c->stream);
        // ---- step 4: sizes ----
        hipLaunchKernelGGL(pair_rowpop_kernel, dim3(nstreams), dim3(NT), 0, c->stream, bm, stride, ktiles * KT_WORDS, sizes);
        UKM_HIP(hipGetLastError());
        UKM_TRY(StepEvents::us(ev.e[0], ev.e[1], &us));
        bits_us += us;
        UKM_TRY(StepEvents::us(ev.e[2], ev.e[3], &us));  // (the events are recorded again for the next block: wait here)
        kernel_us += us;
    }
    if (tri && nstreams > 1) {
        hipLaunchKernelGGL(pair_mirror_kernel, dim3(grid_for(c, (u64)nstreams * nstreams)), dim3(NT), 0, c->stream, C, (u64)nstreams);
        UKM_HIP(hipGetLastError());
    }
    c->stat_pair_bits_us = (u64)bits_us;
    c->stat_pair_kernel_us = (u64)kernel_us;
    c->kernel_ms_sum = (float)(kernel_us / 1000.0);
    return UKM_OK;
}

}  // namespace

extern "C" int ukm_pair_counts(ukm_ctx *ctx, const uint64_t *const *keys, const uint64_t *lens, int nstreams, int nrows, uint32_t flags,
                               uint64_t *out_counts, uint64_t *out_sizes) {
    if (!ctx) UKM_FAIL(UKM_ERR_INVALID, "ukm_pair_counts: ctx is NULL");
    if (nstreams < 1 || (u64)nstreams > MAX_STREAMS) UKM_FAIL(UKM_ERR_INVALID, "ukm_pair_counts: nstreams %d outside 1 .. %llu", nstreams, (unsigned long long)MAX_STREAMS);
    if (nrows < 1 || nrows > nstreams) UKM_FAIL(UKM_ERR_INVALID, "ukm_pair_counts: nrows %d outside 1 .. nstreams (%d)", nrows, nstreams);
    if (flags != 0) UKM_FAIL(UKM_ERR_INVALID, "ukm_pair_counts: flags must be 0 (got %u)", flags);
    if (!keys || !lens || !out_counts) UKM_FAIL(UKM_ERR_INVALID, "ukm_pair_counts: NULL argument");
    CallScope s;
    UKM_TRY(ukm_begin(ctx, &s));
    int rc = [&]() -> int {
        u64 *C = nullptr, *sizes = nullptr;
        UKM_TRY(ukm_out_t(ctx, out_counts, (size_t)nrows * nstreams, &C));
        UKM_TRY(ukm_out_t(ctx, out_sizes, (size_t)nstreams, &sizes));
        if (!sizes) UKM_TRY(ws_alloc_t(ctx, (size_t)nstreams, &sizes));
        return pair_counts_body(ctx, keys, lens, (u32)nstreams, (u32)nrows, C, sizes);
    }();
    return ukm_finish(&s, rc);
}
