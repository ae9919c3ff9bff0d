// The resident schedule's launch with the multiplexed (MUX = 1) and LargeStepCache (MUX = 2) large steps: a TU of its own, like step_large_mux.hip
#ifndef LMC_NO_RNG_JUMP_LDS
#define LMC_RNG_JUMP_LDS  // drng.h: the PCG jump constants of this launch live in LDS
#endif
#include "step_resident.h"

using namespace lmcd;

void LaunchStepResidentMux(const DScene &S, const DCache *cache, const ChainArrays &A, const Film &film, const StepParams &P, int maxSteps, int lanes,
                           unsigned long long *guard, bool glossy, int mux, int bvhStackNeed, hipStream_t s) {
    if (mux == 1) LaunchResidentForm<1>(S, cache, A, film, P, maxSteps, lanes, guard, glossy, bvhStackNeed, s);
    else
        LaunchResidentForm<2>(S, cache, A, film, P, maxSteps, lanes, guard, glossy, bvhStackNeed, s);
}
