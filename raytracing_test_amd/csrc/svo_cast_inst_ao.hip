// svo_cast_inst_ao.hip — the k_cast instances of the primary casts with hemisphere AO (and their diagnostics: see svo_cast_kernel.h)
#include "svo_cast_kernel.h"

SVO_CAST_AO(SVO_CAST_INSTANCE)
