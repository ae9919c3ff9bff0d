// The hot launch: plain small steps (dsmall.h) of the chains on the smallPlain list.  Everything indexed at run time
// lives in LDS (dsmall.h: 52 words per thread on the torus) and the path is streamed through registers.  Private memory: the kernel reports
// 2.9-3.4 KB per lane, which is (hipcc -S, round 4) the frames of the out-of-line functions -- the kd-tree search that 0.015 % of the queries
// reach, the once-per-2^32-draws table advance of the RNG, the trigonometry -- plus, in the body itself, 79 scratch loads and 83 scratch stores:
// the caller-saved registers around those (cold) call sites and, in the cache-query path, the 12-word query vector handed to the search by
// address with the LDS addresses it is filled from.  The steady-state step executes the query-path ones only (two queries per step).
// USE_LDS_STACK = false is the fallback for scenes whose LBVH is deeper than the 32-entry LDS traversal stack.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#ifndef LMC_NO_RNG_JUMP_LDS
#define LMC_RNG_JUMP_LDS  // drng.h: the PCG jump constants of this launch live in LDS
#endif
#include "dsmall.h"
#include "step_kernel.h"

using namespace lmcd;

template <class FILM, bool USE_LDS_STACK, bool GLOSSY, bool PROF = false, bool LIGHTLESS = false, bool QUANT = false>
#ifndef LMC_LEAN_K
#define LMC_LEAN_K 1
#endif
#ifndef LMC_LEAN_TIGHT
#define LMC_LEAN_TIGHT 1  // the Lambertian lightless instantiations take the register-saving forms (dscene.h Stk::kTight); 0: A/B build, the former forms at two waves
#endif
// Waves per SIMD of the Lambertian instantiations without light sub-paths (the headline's launch; quantised and exact nodes, float and fixed-point film): three, since
// they take the register-saving forms of Stk::kTight (dscene.h) and need 159 .. 162 registers with nothing spilled (profiles/r14_lean_tight_resources.txt):
// headline +10 % in every one of three alternated runs (profiles/r14_lean_tight_ab.md).
// -DLMC_LEAN_WAVES=2 is the A/B build: it puts them back at two as well.  -DLMC_LEAN_TIGHT=0 (216 registers) does so too: at three waves that form spills 89.
#ifndef LMC_LEAN_WAVES_LAMBERTIAN_LIGHTLESS
#if defined(LMC_LEAN_WAVES)
#define LMC_LEAN_WAVES_LAMBERTIAN_LIGHTLESS LMC_LEAN_WAVES
#elif !LMC_LEAN_TIGHT
#define LMC_LEAN_WAVES_LAMBERTIAN_LIGHTLESS 2
#else
#define LMC_LEAN_WAVES_LAMBERTIAN_LIGHTLESS 3
#endif
#endif
#ifndef LMC_LEAN_WAVES
#define LMC_LEAN_WAVES 2  // waves per SIMD the register allocation aims at
#endif
#ifndef LMC_LEAN_WAVES_GLOSSY_LIGHTLESS
// ... of the glossy instantiation without light sub-paths (full-material scenes lit by their environment map: BASELINE configs[2]): three.  Measured
// (profiles/r05_ao_ab_waves_per_simd.jsonl): that workload +4 %; the glossy instantiation WITH light sub-paths (veach-door) loses 3 % at three waves and the
// Lambertian one 5 % (it has no registers to give), so they stay at two.
#define LMC_LEAN_WAVES_GLOSSY_LIGHTLESS 3
#endif
__global__ void __launch_bounds__(256, (GLOSSY && LIGHTLESS)               ? LMC_LEAN_WAVES_GLOSSY_LIGHTLESS
                                       : (!GLOSSY && LIGHTLESS && !PROF) ? LMC_LEAN_WAVES_LAMBERTIAN_LIGHTLESS
                                                                         : LMC_LEAN_WAVES) k_step_small(StepKernArgs<FILM> /* read through KernArgs (step_kernel.h) */) {
    extern __shared__ float lds[];
    const StepKernArgs<FILM> &K = KernArgs<StepKernArgs<FILM>>();
    const DScene &S = K.S;
    const DCache *cache = K.cache;
    const ChainArrays &A = K.A;
    const FILM &film = K.film;
    const StepParams &P = K.P;
    const int *list = K.list, *listCount = K.listCount;
    const int stackWords = K.stackWords;
    if ((int)(blockIdx.x * blockDim.x) >= *listCount) return;  // a block past the end of the work list: nothing to set up, nothing to do
    LMC_RNG_JUMP_INIT();
    LMC_MAT_LDS_INIT(S);
    StepStats st;
    const int total = *listCount;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const LdsView L{lds + threadIdx.x, (int)blockDim.x, stackWords};
    typename std::conditional<PROF, WaveProf, NoProf>::type prof;
    if constexpr (PROF) prof.Start();
    // One chain per thread, no grid-stride loop: the launch function sizes the grid to cover every slot a list can name.  Around a loop the compiler hoists every
    // launch-uniform value of the body (addresses of the chain arrays, scene constants) in front of it and keeps them alive, or spilled, through the whole
    // step: the loop alone cost the flagship instantiation 31 VGPRs and all of its VGPR spills.
    if (const int j = tid; j < total) {
        int i = list[j];
        Rng rng = LoadChainRng(A, P.chainBegin, S.opt.seedOffset, i);
#if LMC_LEAN_K > 1  // A/B build (DESIGN.md "K small steps of a chain per launch"): the chain stays in its lane for up to K consecutive plain small steps
#pragma unroll 1
        for (int rep = 0;; rep++) {
#endif
        constexpr bool TIGHT = !GLOSSY && LIGHTLESS && !PROF && LMC_LEAN_TIGHT;
        if (USE_LDS_STACK) {
            LdsStackT<GLOSSY, QUANT, TIGHT> stk{reinterpret_cast<int *>(L.base), L.stride, 0};
            SmallStepLean<false, LIGHTLESS>(S, *cache, A, film, P, i, rng, L, stk, st, prof);
        } else {
            LocalStackT<GLOSSY, QUANT, TIGHT> stk;
            SmallStepLean<false, LIGHTLESS>(S, *cache, A, film, P, i, rng, L, stk, st, prof);
        }
        if constexpr (TIGHT) LMC_PIN1(i);  // the chain's addresses are formed again behind the step instead of living through it (dscene.h Stk::kTight)
        const unsigned char nk = QueueNext(S, *cache, A, P, i, rng);
#if LMC_LEAN_K > 1
            if (rep + 1 >= LMC_LEAN_K || (nk & 3) != NEXT_SMALL_PLAIN) break;
        }
#else
        (void)nk;
#endif
        StoreChainRng(A, i, rng);
        prof.Mark(PR_QUEUE);
    }
    if constexpr (PROF) {  // one lane per wave adds the wave's region totals (A.prof: PR_COUNT cycle sums + the number of waves)
        if ((threadIdx.x & 63) == 0) {
            for (int r = 0; r < PR_COUNT; r++) atomicAdd(&A.prof[r], prof.acc[r]);
            atomicAdd(&A.prof[PR_COUNT], 1ull);
        }
    }
    if (!LMC_EXP(P.expFlags, 8)) BlockReduceStats(st, A.counters, A.weightSum, reinterpret_cast<int *>(lds));
}

// Which instantiation of k_step_small a launch takes: ONE place decides, the launch function and the query of the ABI (lmc_lean_info) read it.
//   lds: the traversal stack in LDS (ldsStack = false, LMC_LEAN_LDS=0 of host/context.cpp, is the private-stack fallback on a tree that would fit);
//   prof: the region-timing instantiations (LDS stack only, exact nodes, with light sub-paths);  quant: the scene's choice of nodes (host/context.cpp
//   UploadScene), LDS stack only;  tight: dscene.h Stk::kTight
#ifndef LMC_FILM_LAYERS_TU  // (step_small_plain_layers.hip includes this file for the kernel and its launch function; it takes the same forms)
LeanForm LeanFormOf(const DScene &S, int bvhDepth, bool glossy, bool ldsStack, bool profile) {
    LeanForm f{};
    f.lds = ldsStack && bvhDepth <= BVH_LDS_STACK;
    f.glossy = glossy;
    f.prof = profile && f.lds;
    f.lightless = f.lds && !f.prof && S.opt.leanLightless != 0;
    f.quant = S.qnodes != nullptr && f.lds && !profile;
    f.tight = !glossy && f.lightless && LMC_LEAN_TIGHT;
    return f;
}
#endif
static std::atomic<bool> g_leanLogged{false};  // LMC_LEAN_LOG: one line per process

template <class FILM>
static void LaunchStepSmallPlainT(const DScene &S, const DCache *cache, const ChainArrays &A, const FILM &film, const StepParams &P, const int *list, const int *listCount,
                          const NextLists &next, int bvhDepth, bool glossy, bool ldsStack, int blockThreads, bool profile, hipStream_t s) {
    RequireJumpLdsBlock(blockThreads);
    const int gridBlocks = (A.N + blockThreads - 1) / blockThreads;  // the kernel runs one chain per thread: the grid covers every slot a list can name
    const int stackWords = LeanStackWords(bvhDepth);  // bvhDepth: the tree's stack need (host/accel.cpp)
    size_t ldsBytes = (size_t)blockThreads * LeanLdsWordsPerThread(stackWords) * sizeof(float);
    if (const char *e = getenv("LMC_EXP_LDS_EXTRA")) ldsBytes += (size_t)atoi(e);  // measurement aid: lowers the occupancy without touching the code
    const LeanForm f = LeanFormOf(S, bvhDepth, glossy, ldsStack, profile);
    const StepKernArgs<FILM> K{S, cache, A, film, P, list, listCount, nullptr, 0, stackWords};
    // LMC_LEAN_LOG (measurement, stderr, the first lean launch of the process): the blocks of this launch a CU holds, as the runtime computes it from the kernel's
    // registers and its static + dynamic LDS (the Lambertian lightless instantiations, compiled for three waves per SIMD: eleven one-wave blocks on the torus, LDS-bound).
    const bool log = getenv("LMC_LEAN_LOG") != nullptr && !g_leanLogged.exchange(true);
#define LMC_LAUNCH_SMALL(...)                                                                                                                                      \
    do {                                                                                                                                                           \
        if (log) {                                                                                                                                                 \
            int blocks = -1;                                                                                                                                       \
            hipFuncAttributes fa{};                                                                                                                                \
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_step_small<FILM, __VA_ARGS__>, blockThreads, ldsBytes);                                  \
            (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_step_small<FILM, __VA_ARGS__>));                                                      \
            fprintf(stderr, "[lean] k_step_small<%s>: stack need %d -> %d + %d LDS words per thread, %zu dynamic + %zu static bytes per block of %d, %d registers, " \
                            "%zu scratch bytes per lane: %d blocks per CU\n",                                                                                      \
                    #__VA_ARGS__, bvhDepth, stackWords, LeanLdsWordsPerThread(stackWords) - stackWords, ldsBytes, (size_t)fa.sharedSizeBytes, blockThreads,        \
                    fa.numRegs, (size_t)fa.localSizeBytes, blocks);                                                                                                \
        }                                                                                                                                                          \
        LaunchKernArgs(k_step_small<FILM, __VA_ARGS__>, dim3(gridBlocks), dim3(blockThreads), ldsBytes, s, K);                                                     \
    } while (0)
    if (f.prof) {
        if (glossy) LMC_LAUNCH_SMALL(true, true, true);
        else
            LMC_LAUNCH_SMALL(true, false, true);
    } else if (f.lds && !glossy && f.lightless) {
        if (f.quant) LMC_LAUNCH_SMALL(true, false, false, true, true);
        else
            LMC_LAUNCH_SMALL(true, false, false, true);
    } else if (f.lds && glossy && f.lightless) {
        if (f.quant) LMC_LAUNCH_SMALL(true, true, false, true, true);
        else
            LMC_LAUNCH_SMALL(true, true, false, true);
    } else if (f.lds && !glossy) {
        if (f.quant) LMC_LAUNCH_SMALL(true, false, false, false, true);
        else
            LMC_LAUNCH_SMALL(true, false);
    } else if (f.lds && glossy) {
        if (f.quant) LMC_LAUNCH_SMALL(true, true, false, false, true);
        else
            LMC_LAUNCH_SMALL(true, true);
    } else if (!glossy)
        LMC_LAUNCH_SMALL(false, false);
    else
        LMC_LAUNCH_SMALL(false, true);
#undef LMC_LAUNCH_SMALL
}
#ifdef LMC_FILM_LAYERS_TU
void LaunchStepSmallPlainLayers(const DScene &S, const DCache *cache, const ChainArrays &A, const ChainFilmLayers &film, const StepParams &P, const int *list, const int *listCount,
                          const NextLists &next, int bvhDepth, bool glossy, bool ldsStack, int blockThreads, bool profile, hipStream_t s) {
    LaunchStepSmallPlainT(S, cache, A, film, P, list, listCount, next, bvhDepth, glossy, ldsStack, blockThreads, profile, s);
}
#else
void LeanLaunchPlan(int bvhStackNeed, int blockThreads, int *stackWords, int *ldsWordsPerThread, long long *ldsBytesPerBlock) {
    const int sw = LeanStackWords(bvhStackNeed);
    *stackWords = sw;
    *ldsWordsPerThread = LeanLdsWordsPerThread(sw);
    *ldsBytesPerBlock = (long long)blockThreads * LeanLdsWordsPerThread(sw) * (long long)sizeof(float);
}
void LaunchStepSmallPlain(const DScene &S, const DCache *cache, const ChainArrays &A, const Film &film, const StepParams &P, const int *list, const int *listCount,
                          const NextLists &next, int bvhDepth, bool glossy, bool ldsStack, int blockThreads, bool profile, hipStream_t s) {
    DispatchFilm(film, [&](const auto &f) { LaunchStepSmallPlainT(S, cache, A, f, P, list, listCount, next, bvhDepth, glossy, ldsStack, blockThreads, profile, s); });
}
#endif  // LMC_FILM_LAYERS_TU
