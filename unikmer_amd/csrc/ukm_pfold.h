// ukm_pfold.h — internal: `inter` / `diff` over many sorted sets by LDS hash probes (ukm_pfold.hip)
#pragma once
#include "ukm_route.h"

bool ukm_pfold_enabled(const ukm_ctx *c);  // UKM_NO_PFOLD=1 switches it off (developer knob)
// The route contract of ukm_route.h, arguments as ukm_dev_range_fold (ukm_fold.h).  Declines inter --mix-taxid, a
// duplicate or all-ones code, an unsorted stream and a shape it does not fit: the caller tries the range fold next.
int ukm_dev_probe_fold(ukm_ctx *c, const UkmStreams &in, int op, u32 flags, const UkmOut &o, bool *declined);
