// ukm_map.h — what ukm_map.hip (ukm_locate / ukm_map) needs from its neighbours.
#pragma once

#include "ukm_internal.h"

// Every window of every record (canonical 2-bit codes, or ntHash v1 without a Scaled filter when hash) into out[out_cap],
// through the route run_windows picks (ukm_encode.hip; the kernels: ukm_win_kernels.h).  *win_off (arena, [n_rec + 1]) =
// index of every record's first window, win_off[n_rec] = *n_out; null when there are no records or no bases.  All pointers
// are device pointers.
int ukm_dev_windows(ukm_ctx *c, bool hash, const u8 *bases, const u64 *rec_off, u64 n_rec, int k, int canonical, int circular,
                    u64 *out, u64 out_cap, u64 *n_out, u64 total_bases, const u64 **win_off);

// The first step of every entry point over (bases, rec_off) (ukm_encode.hip), n_rec >= 1; the caller's pointers may be host or
// device pointers.  Stages rec_off[n_rec + 1], takes *total_bases = rec_off[n_rec] and rec_off[0] from the host array or reads
// them back from the device, fails with UKM_ERR_INVALID "<name>: rec_off[0] must be 0", then stages the bases.
int ukm_dev_stage_records(ukm_ctx *c, const char *name, const u8 *bases, const u64 *rec_off, u64 n_rec, const u64 **rec_off_dev,
                          const u8 **bases_dev, u64 *total_bases);
