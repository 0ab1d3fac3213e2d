// ukm_fold.h — internal: `inter` / `diff` over many sorted streams as one range-partitioned launch (ukm_fold.hip)
#pragma once
#include "ukm_route.h"

bool ukm_fold_enabled(const ukm_ctx *c);  // UKM_NO_FOLD=1 switches it off (developer knob)
// the route contract of ukm_route.h; op: UKM_OP_INTER / UKM_OP_DIFF
int ukm_dev_range_fold(ukm_ctx *c, const UkmStreams &in, int op, u32 flags, const UkmOut &o, bool *declined);
