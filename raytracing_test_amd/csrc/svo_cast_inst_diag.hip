// svo_cast_inst_diag.hip — the k_cast instances of the diagnostics (SVO_CAST_STATS / SVO_CAST_TIMELINE) of the primary casts and the shading pass
#include "svo_cast_kernel.h"

SVO_CAST_DIAGNOSTICS(SVO_CAST_INSTANCE)
