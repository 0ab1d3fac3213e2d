// ukm_setop_order.h — which tile a workgroup of a TABLE pass of the 2-way set operation runs (ukm_setop_kernels.h:
// setop_tile_kernel<TABLE>, launch_table).  Plain arithmetic: no HIP type and no library header; tests/setop_order_units.cpp
// includes this file alone and runs it under the host sanitizers.
//
// The hardware deals the workgroups of a grid round-robin over the XCDS dies of the part, each with an L2 of its own: block
// b runs on die b % XCDS.  With tile = block, tiles t and t + 1 never share an L2, although they share the 128-byte lines
// their input ranges and their output ranges begin and end in, and the lines of mp[] and base[].  Here die x takes the
// `chunk` CONSECUTIVE tiles [x * chunk, (x + 1) * chunk), in order: blocks b and b + XCDS run tiles t and t + 1.
//     chunk = ceil(ntiles / XCDS)      grid = XCDS * chunk      tile(b) = (b % XCDS) * chunk + b / XCDS
// No two blocks share both b % XCDS and b / XCDS, so the map is injective; every tile below ntiles has exactly one block
// (b = (t % chunk) * XCDS + t / chunk), and the at most XCDS - 1 blocks whose tile is >= ntiles idle.  Where a block really
// runs decides the speed alone: the tiles of a TABLE pass are independent of each other.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define UKM_ORDER_HD __host__ __device__
#else
#define UKM_ORDER_HD
#endif

namespace ukm_setop_order {

constexpr uint64_t XCDS = 8;  // MI355X: 8 dies of 32 CUs

UKM_ORDER_HD inline uint64_t chunk_of(uint64_t ntiles) { return (ntiles + XCDS - 1) / XCDS; }
// workgroups of the launch; xcd_order == 0: the identity, one block per tile
UKM_ORDER_HD inline uint64_t grid_of(uint64_t ntiles, uint32_t xcd_order) { return xcd_order ? XCDS * chunk_of(ntiles) : ntiles; }
// the tile of block b < grid_of(ntiles, xcd_order); a value >= ntiles: the block has none
UKM_ORDER_HD inline uint64_t tile_of(uint64_t b, uint64_t ntiles, uint32_t xcd_order) {
    return xcd_order ? (b % XCDS) * chunk_of(ntiles) + b / XCDS : b;
}

}  // namespace ukm_setop_order
