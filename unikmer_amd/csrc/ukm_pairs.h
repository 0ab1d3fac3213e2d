// ukm_pairs.h — the plain arithmetic of ukm_pair_counts (ukm_pairs.hip): the column-block plan, the bitmap's row stride,
// the map from a linear tile index to a tile of stream pairs, the K split and the grid checks.  No HIP type and no
// library header: tests/pairs_units.cpp includes this file alone and runs it under the host sanitizers.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define UKM_PAIRS_HD __host__ __device__
#else
#define UKM_PAIRS_HD
#endif

namespace ukm_pairs {

constexpr uint32_t TILE = 64;                    // streams on each side of a workgroup's tile of pairs
constexpr uint32_t KT_WORDS = 64;                // 32-bit bitmap words of one row in a K tile
constexpr uint64_t KT_COLS = 32ull * KT_WORDS;   // columns (distinct codes) of a K tile
constexpr uint64_t MAX_STREAMS = 65536;
constexpr uint64_t BITMAP_MAX_BYTES = 1ull << 30;  // the bit matrix of one column block under the default plan
// A thread of pair_popc_kernel sums popcounts into 32-bit registers over the K slice of ONE launch, which is at most one
// column block: a block narrower than 2^32 columns cannot overflow them.
constexpr uint64_t MAX_BLOCK_COLS = 1ull << 31;
static_assert(MAX_BLOCK_COLS < (1ull << 32), "32-bit popcount sums: one launch sees fewer than 2^32 bits of a row");
static_assert(MAX_BLOCK_COLS % KT_COLS == 0 && KT_COLS % 1024 == 0, "a row of whole K tiles is a whole number of 128-byte lines");
constexpr uint64_t MAX_GRID = 0x7fffffffull;     // workgroups of a one-dimensional launch
constexpr uint32_t TARGET_WGS = 2048;            // workgroups a pair launch aims at: 8 per CU

UKM_PAIRS_HD inline uint64_t round_up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }
UKM_PAIRS_HD inline uint32_t tiles_of(uint64_t streams) { return (uint32_t)((streams + TILE - 1) / TILE); }
// rows of the bit matrix: whole tiles, so that the pair kernel loads without a row check (the padding rows stay zero)
UKM_PAIRS_HD inline uint64_t padded_rows(uint64_t nstreams) { return round_up(nstreams, TILE); }
// words from one row of the bit matrix to the next, for a matrix `cols` columns wide: whole K tiles, hence whole 128-byte lines
UKM_PAIRS_HD inline uint64_t row_stride_words(uint64_t cols) { return round_up(cols ? cols : 1, KT_COLS) / 32; }
UKM_PAIRS_HD inline uint64_t bitmap_bytes(uint64_t nstreams, uint64_t cols) { return padded_rows(nstreams) * row_stride_words(cols) * 4; }

// columns per block: the option (a developer and test knob, rounded up to whole K tiles) or the widest block whose bit
// matrix, padded rows included, stays within BITMAP_MAX_BYTES; at least one K tile, at most MAX_BLOCK_COLS
inline uint64_t block_cols(uint64_t nstreams, long long option) {
    uint64_t w = option > 0 ? round_up((uint64_t)option, KT_COLS) : BITMAP_MAX_BYTES * 8 / padded_rows(nstreams) / KT_COLS * KT_COLS;
    if (w < KT_COLS) w = KT_COLS;
    if (w > MAX_BLOCK_COLS) w = MAX_BLOCK_COLS;
    return w;
}

// Block b holds columns [b * w, min((b + 1) * w, ncols)): consecutive ranks of the sorted distinct codes.
struct Plan {
    uint64_t w = KT_COLS;    // columns per block
    uint64_t nblocks = 0;    // 0 when there is no column
    uint64_t alloc_cols = 0; // width the bit matrix is allocated for: w, or less when all columns fit a narrower one
    uint64_t begin(uint64_t b) const { return b * w; }
    uint64_t end(uint64_t b, uint64_t ncols) const { return (b + 1) * w < ncols ? (b + 1) * w : ncols; }
};
inline Plan plan_blocks(uint64_t ncols, uint64_t nstreams, long long option) {
    Plan p;
    p.w = block_cols(nstreams, option);
    p.nblocks = (ncols + p.w - 1) / p.w;
    p.alloc_cols = ncols < p.w ? round_up(ncols ? ncols : 1, KT_COLS) : p.w;
    return p;
}

// ---- tiles of stream pairs ---------------------------------------------------------------------------------------------
// Triangle (nrows == nstreams): the tiles (ti, tj) with tj >= ti of an nt x nt grid, row by row.  Row ti starts at
// tri_row_start(ti, nt) and holds nt - ti tiles.
UKM_PAIRS_HD inline uint64_t tri_count(uint32_t nt) { return (uint64_t)nt * (nt + 1) / 2; }
UKM_PAIRS_HD inline uint64_t tri_row_start(uint32_t ti, uint32_t nt) { return (uint64_t)ti * (2ull * nt - ti + 1) / 2; }
UKM_PAIRS_HD inline void tri_tile(uint64_t lin, uint32_t nt, uint32_t *ti, uint32_t *tj) {
    uint32_t lo = 0, hi = nt - 1;  // the last row whose start is <= lin
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (tri_row_start(mid, nt) <= lin) lo = mid;
        else hi = mid - 1;
    }
    *ti = lo;
    *tj = lo + (uint32_t)(lin - tri_row_start(lo, nt));
}
// Rectangle (nrows < nstreams): every tile of ntr row tiles x ntc column tiles, row by row.
UKM_PAIRS_HD inline void rect_tile(uint64_t lin, uint32_t ntc, uint32_t *ti, uint32_t *tj) {
    *ti = (uint32_t)(lin / ntc);
    *tj = (uint32_t)(lin % ntc);
}
inline uint64_t tile_count(uint64_t nrows, uint64_t nstreams) {
    return nrows == nstreams ? tri_count(tiles_of(nstreams)) : (uint64_t)tiles_of(nrows) * tiles_of(nstreams);
}

// ---- K split -----------------------------------------------------------------------------------------------------------
// A launch covers `ktiles` K tiles with ntiles x nslices workgroups, each taking kt_per_slice consecutive K tiles of one
// tile of pairs.  Few tiles (few streams): the K range is cut so that about TARGET_WGS workgroups run, but not into slices
// shorter than 4 K tiles, whose 4096 atomic adds per workgroup would outweigh their popcounts.
struct KSplit {
    uint32_t kt_per_slice = 1, nslices = 1;
};
inline KSplit ksplit(uint64_t ntiles, uint64_t ktiles) {
    KSplit s;
    if (ktiles == 0) ktiles = 1;
    uint64_t want = ntiles >= TARGET_WGS ? 1 : TARGET_WGS / (ntiles ? ntiles : 1);
    const uint64_t most = ktiles / 4 ? ktiles / 4 : 1;
    if (want > most) want = most;
    s.kt_per_slice = (uint32_t)((ktiles + want - 1) / want);
    s.nslices = (uint32_t)((ktiles + s.kt_per_slice - 1) / s.kt_per_slice);
    return s;
}

// every one-dimensional grid of the call, for nstreams streams, nrows rows and blocks of `cols` columns
inline bool grids_ok(uint64_t nstreams, uint64_t nrows, uint64_t cols) {
    const uint64_t ntiles = tile_count(nrows, nstreams);
    const KSplit s = ksplit(ntiles, (cols + KT_COLS - 1) / KT_COLS);
    return ntiles * s.nslices <= MAX_GRID   // pair_popc_kernel
           && nstreams <= MAX_GRID;         // pair_rowpop_kernel: one workgroup per row
}

}  // namespace ukm_pairs
