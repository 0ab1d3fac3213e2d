// ukm_punion.h — internal: `union` of many heavily overlapping sorted sets by LDS hash probes (ukm_punion.hip)
#pragma once
#include "ukm_route.h"

// developer / test knob UKM_PUNION: 0 = never, 1 = whenever the shape allows it (size thresholds ignored),
// 2 = as 1 and without the hit-rate guard.  Unset: the library's own choice.
int ukm_punion_mode(const ukm_ctx *c);
// UKM_PUNION_TAX=0: records with TaxIds never take this path
int ukm_punion_tax_mode(const ukm_ctx *c);
// The three entries keep the route contract of ukm_route.h.  A stream whose in.taxids[j] is null and whose
// in.file_taxids[j] is set carries that ONE taxid (the .unik header's global taxid): it loads no taxid and looks no
// pre-order number up.
// Union; declines low overlap, an unsorted stream, a miss buffer overflow (the caller's k-way merge answers).  The
// result's TaxId is the LCA over every record of a code.  overlap_known: the caller has just sampled the overlap itself.
int ukm_dev_probe_union(ukm_ctx *c, const UkmStreams &in, bool overlap_known, const UkmOut &o, bool *declined);
// `common` below the number of files through the same tables with a record count per entry; in.keys[0] = the first file
// as a sorted duplicate-free set (first_once), or -- !first_once -- every record of every file counts (`merge -d`).
int ukm_dev_probe_common(ukm_ctx *c, const UkmStreams &in, u32 threshold, bool first_once, const UkmOut &o, bool *declined);
// Keep-everything merge of many files that share most of their codes, by placement (pl_merge_kernel):
// developer knob UKM_PLACE: 0 = never, 1 = whenever the shape allows it.
int ukm_place_mode(const ukm_ctx *c);
int ukm_dev_place_merge(ukm_ctx *c, const UkmStreams &in, const UkmOut &o, bool *declined);
