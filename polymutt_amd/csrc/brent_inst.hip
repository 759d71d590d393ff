// brent_inst.hip -- part PM_BRENT_PART of the k_brent instantiations (brent_variants.h), one object per part so the
// Makefile compiles the Brent kernel's variants in parallel; engine.hip launches them through extern declarations.
#include "engine_dev.h"
#include "brent_variants.h"

#ifndef PM_BRENT_PART
#error "compile with -DPM_BRENT_PART=<0 .. PM_BRENT_PARTS-1>"
#endif
#define PM_BRENT_X(part, ...) template __global__ void k_brent<__VA_ARGS__>(DevArgs, int);
#define PM_BRENT_LIST_(k) PM_BRENT_VARIANTS_##k
#define PM_BRENT_LIST(k) PM_BRENT_LIST_(k)
PM_BRENT_LIST(PM_BRENT_PART)
