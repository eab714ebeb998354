// svo_cast_inst_primary.hip — the k_cast instances of the primary casts (hit records or wire records)
#include "svo_cast_kernel.h"

SVO_CAST_PRIMARY(SVO_CAST_INSTANCE)
