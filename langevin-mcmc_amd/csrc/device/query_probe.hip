// Test probe (host/probes.cpp lmc_lean_query_probe): the lean small step's cache look-up -- dsmall.h PrepareGaussianLean and GaussianDim as they
// stand, called the way SmallStepLean calls them for a proposal -- on caller-given cache rows and chain states, one query per lane, with the LDS laid
// out as the lean launch lays it out (LdsView, the query in L.Q).  Next to it the generic kernel's CacheQuery (dchain.h) on the same query.
// The stand-in ChainArrays of N = nq hold only the words the two functions touch: pathWeight, chV1, chV2, chLastPss.
#include "dsmall.h"
#include "kernels.h"

using namespace lmcd;

__global__ void __launch_bounds__(64) k_lean_query_probe(DScene S, const DCache *cache, ChainArrays A, StepParams P, int dim, int nq, const float *q, const int *queried,
                                                         const float *ssScore, LeanQueryProbeOut out, int stackWords) {
    extern __shared__ float lds[];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const LdsView L{lds + threadIdx.x, (int)blockDim.x, stackWords};
    for (int k = 0; k < dim; k++) L.Q(k) = q[(size_t)i * dim + k];
    const DCacheDim &C = cache->d[dim];
    const float ss = ssScore[i];
    const int flags = queried[i] ? F_QUERIED : 0;
    StepStats st;
    VSource vs;
    const GradState gs{nullptr, 0, 0, ss, true, nullptr, 0, 0};
    PrepareGaussianLean<false>(S, *cache, A, P, i, dim, 1.0f, flags, L, vs, st, gs);
    if (vs.mode == VS_REUSE) StageReuseVectors(A, i, dim, L);
    float logDet = 0.f;
    float *og = out.gauss + (size_t)i * (3 * dim + 1);
#pragma unroll 1
    for (int k = 0; k < dim; k++) {
        const GaussK g = GaussianDim(S, C, A, i, dim, k, vs, ss, L, logDet, true);
        og[k] = g.mean, og[dim + k] = g.covL, og[2 * dim + k] = g.invCov;
    }
    if (LogDetIsClosedForm(vs, ss)) logDet = ClosedFormLogDet(S, vs, dim);
    og[3 * dim] = logDet;
    int *oi = out.ints + (size_t)i * LEAN_PROBE_INTS;
    oi[0] = vs.mode, oi[1] = vs.nMatches, oi[7] = st.cacheQueries, oi[8] = st.cacheHits;
#pragma unroll
    for (int m = 0; m < 5; m++) {
        const bool have = vs.mode == VS_BLEND && m < vs.nMatches;
        oi[2 + m] = have ? vs.idx[m] : -1;
        out.w[(size_t)i * 5 + m] = have ? vs.w[m] : 0.f;
    }
    // the generic kernel's query (dstep.h InitGaussianFor -> dchain.h CacheQuery) of the same point
    float pss[MAXPSS], v1[MAXPSS], v2[MAXPSS];
    for (int k = 0; k < MAXPSS; k++) pss[k] = k < dim ? q[(size_t)i * dim + k] : 0.f, v1[k] = v2[k] = 0.f;
    const bool hit = CacheQuery(C, dim, pss, v1, v2);
    oi[9] = hit ? 1 : 0;
    for (int k = 0; k < dim; k++) out.generic[(size_t)i * 2 * dim + k] = hit ? v1[k] : 0.f, out.generic[(size_t)i * 2 * dim + dim + k] = hit ? v2[k] : 0.f;
}

void LaunchLeanQueryProbe(const DScene &S, const DCache *cache, const ChainArrays &A, const StepParams &P, int dim, int nq, const float *q, const int *queried,
                          const float *ssScore, const LeanQueryProbeOut &out, hipStream_t s) {
    const int stackWords = LeanStackWords(0);
    const size_t ldsBytes = (size_t)64 * LeanLdsWordsPerThread(stackWords) * sizeof(float);
    hipLaunchKernelGGL(k_lean_query_probe, dim3((nq + 63) / 64), dim3(64), ldsBytes, s, S, cache, A, P, dim, nq, q, queried, ssScore, out, stackWords);
}
