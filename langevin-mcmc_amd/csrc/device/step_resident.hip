// The resident schedule's launch (kernel and the reasoning: step_resident.h); the bidirectional large-step forms, the other two in step_resident_mux.hip
#ifndef LMC_NO_RNG_JUMP_LDS
#define LMC_RNG_JUMP_LDS  // drng.h: the PCG jump constants of this launch live in LDS
#endif
#include "step_resident.h"

using namespace lmcd;

void LaunchStepResidentMux(const DScene &S, const DCache *cache, const ChainArrays &A, const Film &film, const StepParams &P, int maxSteps, int lanes,
                           unsigned long long *guard, bool glossy, int mux, int bvhStackNeed, hipStream_t s);  // step_resident_mux.hip

void LaunchStepResident(const DScene &S, const DCache *cache, const ChainArrays &A, const Film &film, const StepParams &P, int maxSteps, int lanes,
                        unsigned long long *guard, bool glossy, int mux, int bvhStackNeed, hipStream_t s) {
    if (lanes != 16 && lanes != 32 && lanes != 64) throw std::runtime_error("resident launch: 16, 32 or 64 chains per wave");
    if (mux == 0) LaunchResidentForm<0>(S, cache, A, film, P, maxSteps, lanes, guard, glossy, bvhStackNeed, s);
    else
        LaunchStepResidentMux(S, cache, A, film, P, maxSteps, lanes, guard, glossy, mux, bvhStackNeed, s);
}
