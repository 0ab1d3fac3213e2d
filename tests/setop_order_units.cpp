// The block -> tile map of a TABLE pass (unikmer_amd/csrc/ukm_setop_order.h) as a stand-alone program: built by
// tests/test_setop_order_cpu.py with the host compiler under the address and undefined-behaviour sanitizers.  Prints "OK".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ukm_setop_order.h"

namespace o = ukm_setop_order;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: ntiles=%llu: %s\n", __FILE__, __LINE__, (unsigned long long)ntiles, #c); exit(1); } } while (0)

static void check(uint64_t ntiles) {
    const uint64_t grid = o::grid_of(ntiles, 1), chunk = o::chunk_of(ntiles);
    CHECK(grid % o::XCDS == 0);
    CHECK(grid == o::XCDS * chunk);
    CHECK(grid >= ntiles && grid - ntiles < o::XCDS);
    std::vector<uint32_t> seen(grid, 0);  // by tile, the idle ones included: tile_of stays below the grid
    uint64_t run = 0, idle = 0;
    for (uint64_t b = 0; b < grid; b++) {
        const uint64_t t = o::tile_of(b, ntiles, 1);
        CHECK(t < grid);
        seen[t]++;
        // what the kernel does with it: `if (tile >= p.ntiles ...) return;`
        if (t < ntiles) run++;
        else idle++;
        // die b % XCDS walks its chunk in order: its next block runs the next tile
        if (b + o::XCDS < grid) CHECK(o::tile_of(b + o::XCDS, ntiles, 1) == t + 1);
        // ... and its chunk is [x * chunk, (x + 1) * chunk)
        CHECK(t / chunk == b % o::XCDS);
    }
    for (uint64_t t = 0; t < grid; t++) CHECK(seen[t] == 1);  // every tile exactly once; no tile >= ntiles twice either
    CHECK(run == ntiles);                                     // no block runs a tile in [ntiles, grid)
    CHECK(idle == grid - ntiles && idle < o::XCDS);
    // the knob off: the identity, one block per tile
    CHECK(o::grid_of(ntiles, 0) == ntiles);
    for (uint64_t b = 0; b < ntiles; b++) CHECK(o::tile_of(b, ntiles, 0) == b);
}

int main() {
    for (uint64_t ntiles = 1; ntiles <= 4200; ntiles++) check(ntiles);
    check(205593);  // 2 x 1e9 codes in tiles of 9728
    // the widest launch the host asks for: the arithmetic stays in 64 bits
    {
        const uint64_t ntiles = 0xFFFFFFF8ull;
        CHECK(o::grid_of(ntiles, 1) == ntiles);
        CHECK(o::tile_of(ntiles - 1, ntiles, 1) == ntiles - 1);
        CHECK(o::grid_of(0xFFFFFFF9ull, 1) == 0x100000000ull);  // (the host falls back to the identity there)
    }
    printf("OK\n");
    return 0;
}
