// Test probe (host/shade_probes.cpp lmc_shade_probe): the texture look-up and the three BSDFs of dshade.h -- EvalTex, BsdfEvaluate<G>, BsdfSample<G> as
// they stand -- on caller-given material records and bitmaps, one case per lane in 64-thread blocks.  Built with the flags of kernels.hip: no
// contraction, no fast math, so that the results are the bits the host build of the same source gives (tests/helpers/dshade_host.cpp).
// The stand-in DScene holds only materials, bitmaps and texPool.  A lane beyond n writes nothing.
#include "shade_probe.h"
#include "kernels.h"

using namespace lmcd;

template <bool GLOSSY>
__global__ void __launch_bounds__(64) k_shade_probe(DScene S, int op, int n, const int *ints, const float *in, int *ok, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ShadeProbeCase<GLOSSY>(S, op, ints + (size_t)i * SHADE_INT_WORDS, in + (size_t)i * SHADE_IN_WORDS, ok + i, out + (size_t)i * SHADE_OUT_WORDS);
}

void LaunchShadeProbe(const DScene &S, int op, bool glossy, int n, const int *ints, const float *in, int *ok, float *out, hipStream_t s) {
    if (n <= 0) return;
    const dim3 grid((n + 63) / 64), block(64);
    if (glossy) hipLaunchKernelGGL(k_shade_probe<true>, grid, block, 0, s, S, op, n, ints, in, ok, out);
    else
        hipLaunchKernelGGL(k_shade_probe<false>, grid, block, 0, s, S, op, n, ints, in, ok, out);
}
