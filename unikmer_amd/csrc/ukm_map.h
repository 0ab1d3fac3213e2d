// ukm_map.h — what ukm_map.hip (ukm_locate / ukm_map) needs from its neighbours.
#pragma once

#include "ukm_internal.h"

// Every window of every record (canonical 2-bit codes, or ntHash v1 without a Scaled filter when hash) into out[out_cap],
// through the route run_windows picks (ukm_encode.hip).  *win_off (arena, [n_rec + 1]) = index of every record's first
// window, win_off[n_rec] = *n_out; null when there are no records or no bases.  All pointers are device pointers.
int ukm_dev_windows(ukm_ctx *c, bool hash, const u8 *bases, const u64 *rec_off, u64 n_rec, int k, int canonical, int circular,
                    u64 *out, u64 out_cap, u64 *n_out, u64 total_bases, const u64 **win_off);
