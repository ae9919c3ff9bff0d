// The resident schedule (lmc_set_option "resident_steps" = K, host/context.cpp RunResident): once the gradient caches are frozen no chain
// reads anything another chain writes (mlt.cpp:60-196; the pushes of mlt.cpp:120-127 stop with the last cache filling), so a chain may run
// its own loop.  One launch advances every chain by up to K complete mutations -- large and small steps, splats, accept / reject, outlier
// reset, its own sample budget -- with no host round trip and no other launch in between: one lane per slot of ChainArrays, the step kind
// taken from the previous step's QueueNext, the RNG loaded once and stored once, the counters reduced once.  Lanes never wait for each
// other across workgroups (no grid barrier, no spin, no cooperative launch) and every lane stops after at most K steps.
//
// The step is StepChain<large + small> without the gradient program (WITH_GRAD = false): with every cache of the context's dims ready,
// InitGaussianFor never reaches its gradient branch and no accepted large step pushes to the cache.  The kernel counts every step that
// WOULD have needed either (guard[1]; lmc_get_option "resident_guard"), so that the claim is checked on every run instead of assumed.
#pragma once
#include <stdexcept>

#include "step_kernel.h"

namespace lmcd {

// lanes: active chains per 64-lane wave (64 / 32 / 16); the other lanes of the wave idle.  Blocks of one wave.
// guard: [0] chain-steps run by resident launches, [1] steps that would have needed the gradient program or pushed to the cache
template <class FILM, bool GLOSSY, bool QUANT, int MUX, bool LDS_STACK>
__global__ void __launch_bounds__(256, LMC_STEP_WAVES) k_step_resident(DScene S, const DCache *cache, ChainArrays A, FILM film, StepParams P, int maxSteps, int lanes,
                                                                       unsigned long long *guard) {
    LMC_RNG_JUMP_INIT();
    LMC_MAT_LDS_INIT(S);
    extern __shared__ int ldsStack[];
    StepStats st;
    int misses = 0;
    const int lane = threadIdx.x;
    const int i = blockIdx.x * lanes + lane;
    if (lane < lanes && i < (int)A.N) {
        unsigned char nk = A.nextKind[i] & 3;
        if (nk != NEXT_DONE) {
            Rng rng = LoadChainRng(A, P.chainBegin, S.opt.seedOffset, i);
            GradWork gw{nullptr, 0, 0};
#pragma unroll 1
            for (int k = 0; k < maxSteps && nk != NEXT_DONE; k++) {
                const int kind = nk == NEXT_LARGE ? KIND_LARGE : KIND_SMALL;
                if (kind == KIND_SMALL && S.opt.mala) {  // the state's dim: a small step keeps the technique
                    const int c = __float_as_int(A.curContrib[i]), l = __float_as_int(A.curContrib[A.N + i]);
                    if (NeedsGradient(*cache, P, c, l)) misses++;
                }
                if constexpr (LDS_STACK) {
                    LdsStackT<GLOSSY, QUANT> stk{ldsStack + threadIdx.x, (int)blockDim.x, 0};
                    StepChain<true, true, false, MUX>(S, *cache, A, film, P, i, kind, rng, gw, st, stk);
                } else {
                    LocalStackT<GLOSSY, QUANT> stk;
                    StepChain<true, true, false, MUX>(S, *cache, A, film, P, i, kind, rng, gw, st, stk);
                }
                if (A.pushDim[i]) misses++;
                nk = QueueNext(S, *cache, A, P, i, rng) & 3;  // every step ends with it: nextKind is valid when lock step resumes
            }
            StoreChainRng(A, i, rng);
        }
    }
    __shared__ int sStats[9];
    BlockReduceStats(st, A.counters, A.weightSum, sStats);
    int steps = st.steps;
    for (int off = 32; off > 0; off >>= 1) steps += __shfl_down(steps, off), misses += __shfl_down(misses, off);
    if (threadIdx.x == 0) {
        if (steps) atomicAdd(&guard[0], (unsigned long long)steps);
        if (misses) atomicAdd(&guard[1], (unsigned long long)misses);
    }
}

// the instantiations of one large-step form (MUX: 0 bidirectional, 1 multiplexed, 2 LargeStepCache) for the scene's material set, node format and
// stack need; the MUX = 0 forms are compiled in step_resident.hip, the other two in step_resident_mux.hip (the two TUs compile in parallel)
template <int MUX, class FILM>
void LaunchResidentFormT(const DScene &S, const DCache *cache, const ChainArrays &A, const FILM &film, const StepParams &P, int maxSteps, int lanes,
                        unsigned long long *guard, bool glossy, int bvhStackNeed, hipStream_t s) {
    constexpr int threads = 64;  // one wave per block
    RequireJumpLdsBlock(threads);
    const int blocks = (int)((A.N + lanes - 1) / lanes);
    if (blocks <= 0 || maxSteps <= 0) return;
#define LMC_LAUNCH_RESIDENT(G, Q, L, lds) \
    hipLaunchKernelGGL((k_step_resident<FILM, G, Q, MUX, L>), dim3(blocks), dim3(threads), lds, s, S, cache, A, film, P, maxSteps, lanes, guard)
    if (bvhStackNeed <= BVH_LDS_STACK) {  // the traversal stack in LDS, sized by the scene's own need (as the large-step launch)
        const size_t lds = (size_t)threads * ((bvhStackNeed + 7) / 8 * 8) * sizeof(int);
        // the scene's node format (host/context.cpp UploadScene); the multiplexed / cache large steps walk the exact nodes, as in lock step
        const bool quant = MUX == 0 && S.qnodes != nullptr;
        if (glossy && quant) LMC_LAUNCH_RESIDENT(true, MUX == 0, true, lds);
        else if (glossy) LMC_LAUNCH_RESIDENT(true, false, true, lds);
        else if (quant) LMC_LAUNCH_RESIDENT(false, MUX == 0, true, lds);
        else
            LMC_LAUNCH_RESIDENT(false, false, true, lds);
        return;
    }
    // a tree deeper than the LDS stack: private stack, compiled once with the glossy code in (a Lambertian scene never takes those branches)
    LMC_LAUNCH_RESIDENT(true, false, false, 0);
#undef LMC_LAUNCH_RESIDENT
}
template <int MUX>
void LaunchResidentForm(const DScene &S, const DCache *cache, const ChainArrays &A, const Film &film, const StepParams &P, int maxSteps, int lanes,
                        unsigned long long *guard, bool glossy, int bvhStackNeed, hipStream_t s) {
    DispatchFilm(film, [&](const auto &f) { LaunchResidentFormT<MUX>(S, cache, A, f, P, maxSteps, lanes, guard, glossy, bvhStackNeed, s); });
}

}  // namespace lmcd
