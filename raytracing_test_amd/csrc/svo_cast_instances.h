// svo_cast_instances.h — the k_cast instances that exist (svo_cast_kernel.h), as lists: no HIP, so the host-only test
// program reads them too (tests/sanitize/host_sanitize.cpp: svo::cast_instance, svo_plan.h, picks listed instances only).
#pragma once

// By family, as X(STATS, STAMPS, AO, SHADE, WIDE, SEG, DIRS, NOREC) lists: each svo_cast_inst_*.hip defines one family,
// svo_cast_kernel.h declares them all, svo_cast.hip's launch table holds them all.
// The AO family holds every instance that casts AO rays, its diagnostics included and first: the last instance of a
// translation unit to use a shared function (ao_count_plan, the AO rays' trace) has it inlined by moving its body
// instead of copying it, which changes that instance's register allocation — so the instances stay in the order the
// single translation unit once held them in, where that one was a plain AO instance (tools/isa_identity.py)
#define SVO_CAST_OCTANTS(X, AO, SHADE, SEG, NOREC)                                                                       \
    X(false, false, AO, SHADE, false, SEG, 1, NOREC) X(false, false, AO, SHADE, false, SEG, 2, NOREC)                    \
    X(false, false, AO, SHADE, false, SEG, 3, NOREC) X(false, false, AO, SHADE, false, SEG, 4, NOREC)                    \
    X(false, false, AO, SHADE, false, SEG, 5, NOREC) X(false, false, AO, SHADE, false, SEG, 6, NOREC)                    \
    X(false, false, AO, SHADE, false, SEG, 7, NOREC) X(false, false, AO, SHADE, false, SEG, 8, NOREC)
#define SVO_CAST_GENERIC(X, STATS, STAMPS, AO)  /* no octant: wide / narrow nodes, with / without segments */           \
    X(STATS, STAMPS, AO, false, true, true, 0, false) X(STATS, STAMPS, AO, false, false, true, 0, false)                 \
    X(STATS, STAMPS, AO, false, true, false, 0, false) X(STATS, STAMPS, AO, false, false, false, 0, false)
#define SVO_CAST_SHADE_GENERIC(X, STATS, STAMPS) \
    X(STATS, STAMPS, false, true, true, true, 0, false) X(STATS, STAMPS, false, true, false, true, 0, false)
#define SVO_CAST_PRIMARY(X) \
    SVO_CAST_OCTANTS(X, false, false, true, false) SVO_CAST_OCTANTS(X, false, false, false, false) SVO_CAST_GENERIC(X, false, false, false)
#define SVO_CAST_AO(X)                                                                                 \
    SVO_CAST_OCTANTS(X, true, false, true, false) SVO_CAST_OCTANTS(X, true, false, false, false)       \
    SVO_CAST_GENERIC(X, true, true, true) SVO_CAST_GENERIC(X, false, false, true)
#define SVO_CAST_SHADING(X) SVO_CAST_OCTANTS(X, false, true, true, false) SVO_CAST_SHADE_GENERIC(X, false, false)
#define SVO_CAST_SHADING_NOREC(X) SVO_CAST_OCTANTS(X, false, true, true, true) SVO_CAST_OCTANTS(X, false, true, false, true)
#define SVO_CAST_DIAGNOSTICS(X)                                                                        \
    SVO_CAST_SHADE_GENERIC(X, true, true) SVO_CAST_GENERIC(X, true, true, false)                       \
    SVO_CAST_SHADE_GENERIC(X, false, true) SVO_CAST_GENERIC(X, false, true, false)
// every family, for a table over all of them
#define SVO_CAST_ALL(X) SVO_CAST_PRIMARY(X) SVO_CAST_AO(X) SVO_CAST_SHADING(X) SVO_CAST_SHADING_NOREC(X) SVO_CAST_DIAGNOSTICS(X)
