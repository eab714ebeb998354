// svo_cast_inst_shade_norec.hip — the k_cast instances of the shading pass without hit records (octants only)
#include "svo_cast_kernel.h"

SVO_CAST_SHADING_NOREC(SVO_CAST_INSTANCE)
