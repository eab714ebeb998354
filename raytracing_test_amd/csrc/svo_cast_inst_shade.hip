// svo_cast_inst_shade.hip — the k_cast instances of the shading pass that can write hit records
#include "svo_cast_kernel.h"

SVO_CAST_SHADING(SVO_CAST_INSTANCE)
