// k_step<false, true, true, true>: see step_kernel.h.  The generic small-step launch runs during cache warm-up only, so
// it is compiled once, with the glossy BSDF code in (the material dispatch is a run-time test on DMaterial::type; a
// Lambertian-only scene just never takes the other branches).
#include "step_kernel.h"

using namespace lmcd;

template <class FILM>
static void LaunchStepSmallGradT(const DScene &S, const DCache *cache, const ChainArrays &A, const FILM &film, const StepParams &P, const int *list, const int *listCount,
                         const NextLists &next, float *gradBuf, int gradStride, bool glossy, int gridBlocks, hipStream_t s) {
    (void)glossy;
    const StepKernArgs<FILM> K{S, cache, A, film, P, list, listCount, gradBuf, gradStride, 0};
    LaunchKernArgs(k_step<FILM, false, true, true, true>, dim3(gridBlocks), dim3(256), 0, s, K);
}
#ifndef LMC_FILM_LAYERS_TU
void LaunchStepSmallGrad(const DScene &S, const DCache *cache, const ChainArrays &A, const Film &film, const StepParams &P, const int *list, const int *listCount,
                         const NextLists &next, float *gradBuf, int gradStride, bool glossy, int gridBlocks, hipStream_t s) {
    DispatchFilm(film, [&](const auto &f) { LaunchStepSmallGradT(S, cache, A, f, P, list, listCount, next, gradBuf, gradStride, glossy, gridBlocks, s); });
}
#else  // the layered MLT film's unit includes this file and instantiates the launch with its own type
void LaunchStepSmallGradLayers(const DScene &S, const DCache *cache, const ChainArrays &A, const ChainFilmLayers &film, const StepParams &P, const int *list, const int *listCount,
                         const NextLists &next, float *gradBuf, int gradStride, bool glossy, int gridBlocks, hipStream_t s) {
    LaunchStepSmallGradT(S, cache, A, film, P, list, listCount, next, gradBuf, gradStride, glossy, gridBlocks, s);
}
#endif
