// pairs_units.cpp — the plain arithmetic of ukm_pair_counts (unikmer_amd/csrc/ukm_pairs.h) as a stand-alone program, built
// with -fsanitize=address,undefined by tests/test_pairs_cpu.py.  Prints OK and exits 0, or says what failed and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <set>
#include <vector>

#include "ukm_pairs.h"

using namespace ukm_pairs;

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
            exit(1);                                      \
        }                                                 \
    } while (0)

static void tile_maps() {
    for (uint32_t nt = 1; nt <= 70; nt++) {
        // triangle: a bijection from [0, nt (nt + 1) / 2) onto {(ti, tj): ti <= tj < nt}
        std::set<std::pair<uint32_t, uint32_t>> seen;
        for (uint64_t lin = 0; lin < tri_count(nt); lin++) {
            uint32_t ti = ~0u, tj = ~0u;
            tri_tile(lin, nt, &ti, &tj);
            CHECK(ti <= tj && tj < nt, "nt %u lin %llu -> (%u, %u)", nt, (unsigned long long)lin, ti, tj);
            CHECK(seen.insert({ti, tj}).second, "nt %u: (%u, %u) twice", nt, ti, tj);
        }
        CHECK(seen.size() == (size_t)nt * (nt + 1) / 2, "nt %u", nt);
        // rectangle: a bijection onto ntr x nt for every number of row tiles
        for (uint32_t ntr = 1; ntr <= nt; ntr++) {
            std::set<std::pair<uint32_t, uint32_t>> rs;
            for (uint64_t lin = 0; lin < (uint64_t)ntr * nt; lin++) {
                uint32_t ti = ~0u, tj = ~0u;
                rect_tile(lin, nt, &ti, &tj);
                CHECK(ti < ntr && tj < nt, "rect %u x %u lin %llu -> (%u, %u)", ntr, nt, (unsigned long long)lin, ti, tj);
                CHECK(rs.insert({ti, tj}).second, "rect %u x %u: (%u, %u) twice", ntr, nt, ti, tj);
            }
            CHECK(rs.size() == (size_t)ntr * nt, "rect %u x %u", ntr, nt);
        }
    }
    // tile_count for every nrows: the triangle only for the full matrix
    for (uint64_t n : {1ull, 63ull, 64ull, 65ull, 130ull, 4480ull})
        for (uint64_t r = 1; r <= n; r += (n > 200 ? 97 : 1))
            CHECK(tile_count(r, n) == (r == n ? tri_count(tiles_of(n)) : (uint64_t)tiles_of(r) * tiles_of(n)), "tile_count(%llu, %llu)", (unsigned long long)r, (unsigned long long)n);
    CHECK(tiles_of(1) == 1 && tiles_of(64) == 1 && tiles_of(65) == 2 && tiles_of(65536) == 1024, "tiles_of");
}

static void block_plan() {
    for (uint64_t ns : {1ull, 64ull, 65ull, 65536ull}) {
        const uint64_t w = block_cols(ns, 0);
        CHECK(w % KT_COLS == 0 && w >= KT_COLS && w <= MAX_BLOCK_COLS, "nstreams %llu: w %llu", (unsigned long long)ns, (unsigned long long)w);
        CHECK(ns * w / 8 <= BITMAP_MAX_BYTES, "nstreams %llu: %llu bytes", (unsigned long long)ns, (unsigned long long)(ns * w / 8));
        CHECK(bitmap_bytes(ns, w) <= BITMAP_MAX_BYTES, "nstreams %llu: padded matrix %llu bytes", (unsigned long long)ns, (unsigned long long)bitmap_bytes(ns, w));
        CHECK(row_stride_words(w) * 4 % 128 == 0 && row_stride_words(w) * 32 >= w, "stride of %llu columns", (unsigned long long)w);
        // the default is the widest: one K tile more would break the bound (unless the cap on a launch's bits decided)
        CHECK(w == MAX_BLOCK_COLS || bitmap_bytes(ns, w + KT_COLS) > BITMAP_MAX_BYTES, "nstreams %llu: w %llu is not the widest", (unsigned long long)ns, (unsigned long long)w);
    }
    CHECK(block_cols(65536, 0) == 131072, "65536 streams: %llu", (unsigned long long)block_cols(65536, 0));
    // the option overrides the default, rounded up to whole K tiles and kept inside the limits
    CHECK(block_cols(130, 2048) == 2048 && block_cols(130, 1) == 2048 && block_cols(130, 2049) == 4096, "option");
    CHECK(block_cols(130, 1ll << 40) == MAX_BLOCK_COLS, "option above the cap");
    CHECK(block_cols(130, 0) != 2048 && block_cols(130, -5) == block_cols(130, 0), "unset option");
    for (uint64_t cols : {1ull, 31ull, 32ull, 33ull, 2047ull, 2048ull, 2049ull, 100000ull}) {
        CHECK(row_stride_words(cols) % KT_WORDS == 0 && row_stride_words(cols) * 32 >= cols && row_stride_words(cols) * 32 < cols + KT_COLS, "stride(%llu)", (unsigned long long)cols);
    }
    // every column falls into exactly one block
    for (long long opt : {0ll, 2048ll, 4096ll, 10000ll})
        for (uint64_t ncols : {0ull, 1ull, 2047ull, 2048ull, 2049ull, 4096ull, 10239ull, 10240ull, 10241ull, 50001ull}) {
            const Plan p = plan_blocks(ncols, 130, opt);
            CHECK(p.w == block_cols(130, opt), "plan w");
            CHECK(p.alloc_cols % KT_COLS == 0 && p.alloc_cols <= p.w && p.alloc_cols >= KT_COLS, "alloc_cols %llu", (unsigned long long)p.alloc_cols);
            std::vector<int> hit(ncols, 0);
            uint64_t prev_end = 0;
            for (uint64_t b = 0; b < p.nblocks; b++) {
                CHECK(p.begin(b) == prev_end && p.end(b, ncols) > p.begin(b), "block %llu of %llu columns", (unsigned long long)b, (unsigned long long)ncols);
                CHECK(p.end(b, ncols) - p.begin(b) <= p.alloc_cols, "block wider than the matrix");
                for (uint64_t c = p.begin(b); c < p.end(b, ncols); c++) hit[c]++;
                prev_end = p.end(b, ncols);
            }
            CHECK(prev_end == ncols, "blocks end at %llu of %llu", (unsigned long long)prev_end, (unsigned long long)ncols);
            for (uint64_t c = 0; c < ncols; c++) CHECK(hit[c] == 1, "column %llu in %d blocks", (unsigned long long)c, hit[c]);
        }
}

static void k_split_and_grids() {
    for (uint64_t ntiles : {1ull, 3ull, 6ull, 136ull, 2048ull, 524800ull})
        for (uint64_t ktiles : {1ull, 2ull, 3ull, 4ull, 5ull, 63ull, 64ull, 4096ull, 1048576ull}) {
            const KSplit s = ksplit(ntiles, ktiles);
            CHECK(s.kt_per_slice >= 1 && s.nslices >= 1, "ksplit");
            CHECK((uint64_t)s.kt_per_slice * s.nslices >= ktiles, "slices cover %llu K tiles", (unsigned long long)ktiles);
            CHECK((uint64_t)s.kt_per_slice * (s.nslices - 1) < ktiles, "no empty slice");
            CHECK(s.nslices == 1 || s.kt_per_slice >= 4, "a slice of %u K tiles", s.kt_per_slice);
            CHECK((uint64_t)s.kt_per_slice * KT_COLS <= MAX_BLOCK_COLS, "a slice under 2^32 bits");
        }
    for (uint64_t ns : {1ull, 64ull, 65ull, 130ull, 65536ull})
        for (uint64_t nr : {(uint64_t)1, ns})
            CHECK(grids_ok(ns, nr, block_cols(ns, 0)), "grids of %llu x %llu", (unsigned long long)nr, (unsigned long long)ns);
    CHECK(ksplit(tile_count(65536, 65536), MAX_BLOCK_COLS / KT_COLS).nslices * tile_count(65536, 65536) <= MAX_GRID, "largest triangle");
}

// The device passes restated on the host with the header's stride, plan and tile maps: set bits block by block, add popcounts
// tile by tile (the triangle's tiles only, then the mirror), against a naive double loop over sets.
static void restatement() {
    std::mt19937_64 rng(7);
    for (int round = 0; round < 40; round++) {
        const uint32_t ns = 1 + (uint32_t)(rng() % 140);
        const uint32_t nrows = (round % 3 == 0) ? ns : 1 + (uint32_t)(rng() % ns);
        const uint64_t pool = 1 + rng() % 6000;
        std::vector<std::set<uint64_t>> sets(ns);
        for (auto &s : sets) {
            const uint64_t m = rng() % 60;
            for (uint64_t i = 0; i < m; i++) s.insert(rng() % pool);
        }
        std::set<uint64_t> all;
        for (auto &s : sets) all.insert(s.begin(), s.end());
        const std::vector<uint64_t> codes(all.begin(), all.end());
        const uint64_t ncols = codes.size();
        const Plan plan = plan_blocks(ncols, ns, round % 2 ? 2048 : 0);
        const uint64_t stride = row_stride_words(plan.alloc_cols);
        std::vector<uint64_t> C((size_t)nrows * ns, 0), sizes(ns, 0);
        const bool tri = nrows == ns;
        for (uint64_t b = 0; b < plan.nblocks; b++) {
            std::vector<uint32_t> bm((size_t)(padded_rows(ns) * stride), 0);
            CHECK(bm.size() * 4 == bitmap_bytes(ns, plan.alloc_cols), "bitmap size");
            for (uint32_t s = 0; s < ns; s++)
                for (uint64_t code : sets[s]) {
                    const uint64_t col = (uint64_t)(std::lower_bound(codes.begin(), codes.end(), code) - codes.begin());
                    if (col < plan.begin(b) || col >= plan.end(b, ncols)) continue;
                    const uint64_t c = col - plan.begin(b);
                    bm.at((size_t)(s * stride + (c >> 5))) |= 1u << (c & 31);
                }
            const uint32_t ktiles = (uint32_t)((plan.end(b, ncols) - plan.begin(b) + KT_COLS - 1) / KT_COLS);
            const uint64_t ntiles = tile_count(nrows, ns);
            const KSplit ks = ksplit(ntiles, ktiles);
            for (uint64_t wg = 0; wg < ntiles * ks.nslices; wg++) {
                uint32_t ti, tj;
                if (tri) tri_tile(wg % ntiles, tiles_of(ns), &ti, &tj);
                else rect_tile(wg % ntiles, tiles_of(ns), &ti, &tj);
                const uint32_t kt0 = (uint32_t)(wg / ntiles) * ks.kt_per_slice, kt1 = std::min(kt0 + ks.kt_per_slice, ktiles);
                for (uint32_t i = ti * TILE; i < (ti + 1) * TILE; i++)
                    for (uint32_t j = tj * TILE; j < (tj + 1) * TILE; j++) {
                        uint32_t acc = 0;
                        for (uint64_t w = (uint64_t)kt0 * KT_WORDS; w < (uint64_t)kt1 * KT_WORDS; w++)
                            acc += (uint32_t)__builtin_popcount(bm.at((size_t)(i * stride + w)) & bm.at((size_t)(j * stride + w)));
                        if (i < nrows && j < ns) C[(size_t)i * ns + j] += acc;
                    }
            }
            for (uint32_t s = 0; s < ns; s++)
                for (uint64_t w = 0; w < (uint64_t)ktiles * KT_WORDS; w++) sizes[s] += (uint64_t)__builtin_popcount(bm.at((size_t)(s * stride + w)));
        }
        if (tri)
            for (uint32_t i = 0; i < ns; i++)
                for (uint32_t j = 0; j < i; j++) C[(size_t)i * ns + j] = C[(size_t)j * ns + i];
        for (uint32_t i = 0; i < nrows; i++)
            for (uint32_t j = 0; j < ns; j++) {
                uint64_t want = 0;
                for (uint64_t code : sets[i]) want += sets[j].count(code);
                CHECK(C[(size_t)i * ns + j] == want, "round %d: C[%u][%u] = %llu, want %llu", round, i, j, (unsigned long long)C[(size_t)i * ns + j], (unsigned long long)want);
            }
        for (uint32_t s = 0; s < ns; s++) CHECK(sizes[s] == sets[s].size(), "round %d: size of %u", round, s);
    }
}

int main() {
    tile_maps();
    block_plan();
    k_split_and_grids();
    restatement();
    printf("OK\n");
    return 0;
}
