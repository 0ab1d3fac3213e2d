// ukm_map.h — what ukm_map.hip (ukm_locate / ukm_map) needs from its neighbours, and what ukm_screen.hip shares with it.
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

// ---- host steps of ukm_map.hip that ukm_screen.hip shares (one definition: ukm_map.hip) -------------------------------------
// The size of the sorted array from which a call sorts its (code, window) pairs first (ukm_map_sorted_route; the measurements
// behind the first two: DESIGN.md 4.14).  ukm_screen's is INHERITED from ukm_map, not measured for that call.
constexpr u64 MAP_SORTED_MIN_KEYS = 1ull << 24, LOCATE_SORTED_MIN_KEYS = 1ull << 23, SCREEN_SORTED_MIN_KEYS = 1ull << 24;
// option "map_sorted" 0 / 1 when it is set, else n_keys >= min_keys
bool ukm_map_sorted_route(const ukm_ctx *c, u64 n_keys, u64 min_keys);
// log2 of the codes per prefix of the directory the calls build over their sorted array (developer knob UKM_MAP_DIR_SLACK)
int ukm_map_dir_slack(const ukm_ctx *c);

// the windows of a call's records, in the context's arena
struct MapWindows {
    const u64 *rec_off = nullptr;  // device
    const u64 *win_off = nullptr;  // device, [n_rec + 1]; null when there are no bases
    u64 *w = nullptr;
    u64 n = 0;
};
// Stage (bases, rec_off) -- host or device pointers, n_rec >= 1 -- and produce every window.  UKM_ERR_INVALID with 2^32 or
// more windows ("split the records"), otherwise the errors of the window kernels.
int ukm_dev_make_windows(ukm_ctx *c, const char *name, const u8 *bases, const u64 *rec_off, u64 n_rec, int k, int canonical, int circular,
                         int hashed, MapWindows *W);
// (w, *wi) = every window and its index, sorted by code (stably: equal codes by window); *wi comes from the arena
int ukm_dev_sort_windows(ukm_ctx *c, u64 *w, u64 n, int key_bits, u32 **wi);
