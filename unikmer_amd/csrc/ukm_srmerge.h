// ukm_srmerge.h — internal entry of the single-pass many-stream merge / union (ukm_srmerge.hip)
#pragma once
#include "ukm_internal.h"
#include "ukm_kway.h"  // UKM_KWAY_UNION / UKM_KWAY_MERGE

// developer / test knob UKM_SRMERGE: 0 = never, 1 = whenever the shape allows it (size thresholds ignored).
// Unset: the library's own choice (many streams, enough records).
int ukm_srmerge_mode(const ukm_ctx *c);
// The route contract of ukm_route.h, as ukm_dev_kway.  Declines too few / too many streams, an unsorted stream and one
// code with more copies than a tile holds: the caller's multi-level merge answers.
// threshold > 1 with UKM_KWAY_UNION: only the codes that have at least that many records (`common` below the number of
// files: common.go:331-335), TaxId as for the union.
int ukm_dev_srmerge(ukm_ctx *c, const UkmStreams &in, int op, u32 threshold, const UkmOut &o, bool *declined);
