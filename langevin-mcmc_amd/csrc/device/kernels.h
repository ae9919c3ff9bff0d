// Launch entry points of kernels.hip (compiled by hipcc for gfx950); called from host/context.cpp and the units beside it (ckpt.cpp, mcrender.cpp, probes.cpp, plugin_abi.cpp, list_probes.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "dchain.h"
#include "dstep_params.h"

namespace lmcd {  // the H2MC launches' types (dh2coop.h, dh2mc.h): only named here, so that the LMC kernels do not depend on those headers
struct H2Arrays;
struct MalaPipe;
struct H2Bins;
struct H2MCParam;
}  // namespace lmcd

void LaunchSeedRng(int n, long long firstSeed, uint64_t *state, uint32_t *tab, hipStream_t s);
void LaunchLowerBoundProbe(int n, const float *cdf, int nq, const float *u, int *out, hipStream_t s);
void LaunchRngProbe(int nSeeds, const unsigned long long *seeds, int mode, int n, float mean, float stddev, uint32_t *tabScratch, uint32_t *out, hipStream_t s);
// single-call form of the plugin symbols (plugin.hip, step_small_h2mc.hip): in / out are device-visible pointers of host-mapped pinned buffers
void LaunchPluginGrad(int c, int l, const float *in, float *out, int wantGrad, hipStream_t s);
void LaunchPluginHess(int c, int l, const float *in, float *stage /* 655 floats of device memory */, float *out, hipStream_t s);
void LaunchCacheProbe(const lmcd::DCache *cache, int dim, int n, const float *u, int *row, const float *query, const int *cl, float *pdf, hipStream_t s);  // step_large_cache.hip
void LaunchTransProbe(int n, int mode, const float *x, const float *y, float *o, hipStream_t s);
// test probe of the texture look-up and the BSDFs (shade_probe.hip, shade_probe.h: the layout of a case's ints / in / out rows): S holds materials,
// bitmaps and texPool alone; op 0 EvalTex, 1 BsdfEvaluate<glossy>, 2 BsdfSample<glossy>; one case per lane, rows from n on are not written
void LaunchShadeProbe(const lmcd::DScene &S, int op, bool glossy, int n, const int *ints, const float *in, int *ok, float *out, hipStream_t s);
void LaunchStreamProbe(long long nWords, const float *in, float *out, hipStream_t s);
void LaunchAddInto(float *dst, const float *src, size_t n, hipStream_t s);  // dst += src
void LaunchAddIntoF64(double *dst, const double *src, size_t n, hipStream_t s);
void LaunchAddIntoI64(long long *dst, const long long *src, size_t n, hipStream_t s);
void LaunchFilmFixedToFloat(const long long *fx, float *rgb, size_t n, hipStream_t s);  // rgb[i] = float(double(fx[i]) * 2^-32)
void LaunchFilmSplatProbe(const lmcd::Film &film, int n, const float *screenXY, const float *rgb, hipStream_t s);
// a pipeline stage's work lists (dh2coop.h H2Bins): the counts turned into offsets, the chains of `list` scattered into the stage's N-entry array by bin
void LaunchBinsCompact(const lmcd::H2Bins &bins, const int *list, const int *listCount, int gridBlocks, hipStream_t s);
void LaunchSplitList(const int *list, const int *listCount, int parts, int *sub, int stride, int *subCount, int gridBlocks, hipStream_t s);
void LaunchSumF64(double *dst, const double *src, int n, hipStream_t s);  // dst[0] = sum of src[0 .. n), left to right
void LaunchTrace(const lmcd::DScene &S, int n, const float *rays, int *prim, float *t, int anyHit, bool tight, hipStream_t s);  // tight: dscene.h Stk::kTight
void LaunchKdProbe(const lmcd::DCacheDim &C, int dim, int nq, const float *q, float radiusSq, int knn, int *outN, int *outIdx, float *outDist, hipStream_t s);
// test probe of the lean small step's cache look-up (query_probe.hip): per query i, ints[i * LEAN_PROBE_INTS ..] = [VSource mode, nMatches, idx[5] (-1: none),
// cacheQueries, cacheHits increments, hit of the generic CacheQuery], w[i * 5 ..] the blend weights, gauss[i * (3 dim + 1) ..] = mean, covL, invCov of
// every dimension and logDet, generic[i * 2 dim ..] = v1, v2 of the generic CacheQuery (zeros on a miss).  A: stand-in chain arrays of N = nq.
constexpr int LEAN_PROBE_INTS = 10;
struct LeanQueryProbeOut {
    int *ints;
    float *w, *gauss, *generic;
};
void LaunchLeanQueryProbe(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::StepParams &P, int dim, int nq, const float *q,
                          const int *queried, const float *ssScore, const LeanQueryProbeOut &out, hipStream_t s);
void LaunchGaussProbe(int n, int dim, const float *v1, const float *M, float ss, float shk, const float *sc, const float *offset, float *out, hipStream_t s);
void LaunchGradBatch(int c, int l, int n, const float *primarySoA, const float *scene, const float *vertSoA, float *logLum, float *gradSoA, int wantGrad,
                     hipStream_t s);
// MLTInit, sharded by init stream: a rank runs the streams [tBegin, tBegin + nStreams); its sample arrays start at global sample gBase
void LaunchInitPass1(const lmcd::DScene &S, int tBegin, int nStreams, long long perThread, long long extra, long long gBase, uint32_t *tabScratch,
                     float *contribScratch, uint64_t *ckState, uint32_t *ckTicks, unsigned char *count, hipStream_t s);
void LaunchInitPass2(const lmcd::DScene &S, long long gBegin, long long numLocal, long long perThread, long long extra, int nSlots, uint32_t *tabScratch,
                     float *contribScratch, const uint64_t *ckState, const uint32_t *ckTicks, const unsigned long long *offset, unsigned char *outCL, float *outLs,
                     hipStream_t s);
void LaunchInitRegen(const lmcd::DScene &S, int numChains, long long perThread, long long extra, const long long *seedSample, const unsigned char *seedCL,
                     uint32_t *tabScratch, float *contribScratch, const uint64_t *seedCkState, const uint32_t *seedCkTicks, float *initPath, float *initContrib,
                     float *initScoreSum, hipStream_t s);
// direct.cpp:4-54; tabScratch: 64 words per 16x16 tile
// waveKernel: one wave per tile with speculative stream positions (kernels.hip) when maxDepth <= 2 and the BVH fits the LDS stack
void LaunchDirect(const lmcd::DScene &S, const lmcd::Film &film, int directSpp, int minDepth, int maxDepth, int bvhDepth, bool waveKernel, uint32_t *tabScratch,
                  hipStream_t s);
void LaunchBidirMC(const lmcd::DScene &S, const lmcd::Film &film, int nThreads, int samplesPerThread, uint32_t *tabScratch, float *contribScratch, hipStream_t s);
// the mc integrator (mc.hip): stream ids [streamBegin, streamEnd) of nTiles * spp; tabScratch: 64 words per thread (MCThreads), counters: 2 x u64
// film: float (contributions weighted by 1 / spp) or, with FILM_EXACT in its H (FilmFx), W*H*3 + 1 fixed-point words of unweighted contributions, the last
// the overflow counter; the launch adds to the film and to the counters, it clears neither
// layerMode ("mc_layers"): 0: the film as above; 1 / 2: nLayers films one after the other (exact: one overflow word behind the last), a contribution in the
// layer McLayerOf gives its (camDepth, lightDepth)
void LaunchMC(const lmcd::DScene &S, const lmcd::Film &film, int layerMode, int nLayers, bool bidirectional, int spp, int minDepth, int maxDepth, long long streamBegin,
              long long streamEnd, uint32_t *tabScratch, unsigned long long *counters, hipStream_t s);
// (McLayerOf / McLayerCount, the numbering of the layers: dchain.h, beside the layered MLT film that shares it)
void LaunchMCSumLayers(const long long *layers, long long *total, size_t n, int nLayers, hipStream_t s);  // total[i] = sum over k of layers[k * n + i]
void LaunchMCSumLayers(const float *layers, float *total, size_t n, int nLayers, hipStream_t s);          // ... float adds in increasing k
long long MCThreads(const lmcd::DScene &S, long long streamBegin, long long streamEnd);
void LaunchMCFixedToFloat(const long long *fx, float *rgb, size_t n, int spp, hipStream_t s);  // rgb[i] = float(double(fx[i]) * 2^-32 / double(spp))
void LaunchSetupChains(const lmcd::ChainArrays &A, int chainBegin, long long perChain, long long chainsNeedExtra, hipStream_t s);
void LaunchFirstKind(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::StepParams &P, hipStream_t s);
// one of the three step launches (device/step_*.hip): chains of `list` (count read on the device) run one mutation and
// append themselves to the lists of the next step
void LaunchStepLarge(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::Film &film, const lmcd::StepParams &P,
                     const int *list, const int *listCount, const lmcd::NextLists &next, float *gradBuf, int gradStride, bool glossy, int gridBlocks, int bvhStackNeed, int blockThreads, hipStream_t s);
void LaunchStepLargeMux(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::Film &film, const lmcd::StepParams &P,
                     const int *list, const int *listCount, const lmcd::NextLists &next, float *gradBuf, int gradStride, bool glossy, int gridBlocks, int bvhStackNeed, int blockThreads, hipStream_t s);  // step_large_mux.hip
void LaunchStepLargeCache(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::Film &film, const lmcd::StepParams &P,
                     const int *list, const int *listCount, const lmcd::NextLists &next, float *gradBuf, int gradStride, bool glossy, int gridBlocks, int bvhStackNeed, int blockThreads, hipStream_t s);  // step_large_cache.hip
void LaunchStepSmallGrad(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::Film &film, const lmcd::StepParams &P,
                         const int *list, const int *listCount, const lmcd::NextLists &next, float *gradBuf, int gradStride, bool glossy, int gridBlocks, hipStream_t s);
void LaunchStepSmallLeanGrad(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::Film &film, const lmcd::StepParams &P, const int *list,
                             const int *listCount, const lmcd::NextLists &next, float *gradBuf, int gradStride, bool glossy, int gridBlocks, int blockThreads, int bvhStackNeed,
                             hipStream_t s);
void LaunchStepSmallPlain(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::Film &film, const lmcd::StepParams &P,
                          const int *list, const int *listCount, const lmcd::NextLists &next, int bvhDepth, bool glossy, bool ldsStack, int blockThreads,
                          bool profile, hipStream_t s);  // one chain per thread: the grid is A.N slots; ldsStack = false: the private-stack instantiations whatever the tree
// ... the same launches with the layered MLT film (dchain.h ChainFilmLayers, "film_layers"), each from a unit of its own (device/step_*_layers.hip)
void LaunchStepLargeLayers(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::ChainFilmLayers &film, const lmcd::StepParams &P,
                     const int *list, const int *listCount, const lmcd::NextLists &next, float *gradBuf, int gradStride, bool glossy, int gridBlocks, int bvhStackNeed, int blockThreads, hipStream_t s);
void LaunchStepLargeMuxLayers(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::ChainFilmLayers &film, const lmcd::StepParams &P,
                     const int *list, const int *listCount, const lmcd::NextLists &next, float *gradBuf, int gradStride, bool glossy, int gridBlocks, int bvhStackNeed, int blockThreads, hipStream_t s);
void LaunchStepLargeCacheLayers(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::ChainFilmLayers &film, const lmcd::StepParams &P,
                     const int *list, const int *listCount, const lmcd::NextLists &next, float *gradBuf, int gradStride, bool glossy, int gridBlocks, int bvhStackNeed, int blockThreads, hipStream_t s);
void LaunchStepSmallGradLayers(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::ChainFilmLayers &film, const lmcd::StepParams &P,
                         const int *list, const int *listCount, const lmcd::NextLists &next, float *gradBuf, int gradStride, bool glossy, int gridBlocks, hipStream_t s);
void LaunchStepSmallLeanGradLayers(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::ChainFilmLayers &film, const lmcd::StepParams &P, const int *list,
                             const int *listCount, const lmcd::NextLists &next, float *gradBuf, int gradStride, bool glossy, int gridBlocks, int blockThreads, int bvhStackNeed,
                             hipStream_t s);
void LaunchStepSmallPlainLayers(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::ChainFilmLayers &film, const lmcd::StepParams &P,
                          const int *list, const int *listCount, const lmcd::NextLists &next, int bvhDepth, bool glossy, bool ldsStack, int blockThreads,
                          bool profile, hipStream_t s);
void LaunchMalaFinishLayers(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::ChainFilmLayers &film, const lmcd::StepParams &P, const lmcd::MalaPipe &M,
                            const int *list, const int *listCount, int gridBlocks, hipStream_t s);
// test probe of its splat routine (filmlayers.hip): n splats (screenXY, rgb, technique cl[2 i], cl[2 i + 1]) through SplatT into `film`; *outside += the finite
// ones whose technique is outside the film's table
void LaunchFilmLayerSplatProbe(const lmcd::ChainFilmLayers &film, int n, const float *screenXY, const float *rgb, const int *cl, unsigned long long *outside, hipStream_t s);
// which instantiation of k_step_small that launch takes (step_small_plain.hip LeanFormOf)
struct LeanForm {
    bool lds, glossy, prof, lightless, quant, tight;
};
LeanForm LeanFormOf(const lmcd::DScene &S, int bvhDepth, bool glossy, bool ldsStack, bool profile);
// what that launch asks of LDS for a tree with the given stack need (dsmall.h LeanStackWords / LeanLdsWordsPerThread): host arithmetic only
void LeanLaunchPlan(int bvhStackNeed, int blockThreads, int *stackWords, int *ldsWordsPerThread, long long *ldsBytesPerBlock);
// the resident schedule (step_resident.h / .hip): every chain of the slot arrays advances by up to maxSteps complete mutations in ONE launch (caches frozen);
// lanes = active chains per 64-lane wave (16 / 32 / 64); guard[0] += chain-steps run, guard[1] += steps that would have needed the gradient program or a cache push
void LaunchStepResident(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::Film &film, const lmcd::StepParams &P, int maxSteps,
                        int lanes, unsigned long long *guard, bool glossy, int mux, int bvhStackNeed, hipStream_t s);
// all small steps of an H2MC render: the launches of the wave-cooperative pipeline (device/dh2coop.h; step_h2_phases.hip, h2hess.hip, h2gauss.hip)
void LaunchH2Begin(const lmcd::DScene &S, const lmcd::ChainArrays &A, const lmcd::StepParams &P, const lmcd::H2Arrays &H, const int *list, const int *listCount, int gridBlocks,
                   hipStream_t s);
void LaunchH2Perturb(const lmcd::DScene &S, const lmcd::ChainArrays &A, const lmcd::StepParams &P, const lmcd::H2Arrays &H, const int *list, const int *listCount,
                     int bvhStackNeed, int gridBlocks, hipStream_t s);
void LaunchH2Finish(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::Film &film, const lmcd::StepParams &P, const lmcd::H2Arrays &H,
                    const int *list, const int *listCount, int gridBlocks, hipStream_t s);
void LaunchH2Hess(const float *rec, const lmcd::H2Bins &bins, int N, const float *scene38 /* host memory: passed by value */, float *hout, int gridBlocks, hipStream_t s);
void LaunchH2Gauss(const lmcd::H2Bins &bins, int N, const float *hout, const lmcd::H2MCParam &param, int expFlags, const int *chainFlags, int stage, float *gaussBuf,
                   const float *offsetSoA, float *px, int gridBlocks, hipStream_t s);
void LaunchH2Sample(const int *list, const int *listCount, int N, const int *chainFlags, const unsigned char *stepKind, const float *curContrib, const float *gaussBuf,
                    float sigma, float *offsetSoA, float *py, int gridBlocks, hipStream_t s);
// the gradient steps of the LMC cache-fill phase as a pipeline (device/dh2coop.h MalaPipe; step_mala_phases.hip, gradcoop.hip)
void LaunchMalaBegin(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::StepParams &P, const lmcd::MalaPipe &M, const int *list,
                     const int *listCount, int gridBlocks, hipStream_t s);
void LaunchMalaMid(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::StepParams &P, const lmcd::MalaPipe &M, const int *list,
                   const int *listCount, int bvhStackNeed, bool glossy, int gridBlocks, hipStream_t s);
void LaunchMalaFinish(const lmcd::DScene &S, const lmcd::DCache *cache, const lmcd::ChainArrays &A, const lmcd::Film &film, const lmcd::StepParams &P, const lmcd::MalaPipe &M,
                      const int *list, const int *listCount, int gridBlocks, hipStream_t s);
void LaunchMalaGrad(const float *rec, const lmcd::H2Bins &bins, int N, const float *scene38 /* host memory: passed by value */, float *gout, int gridBlocks, hipStream_t s);
// n gradient + Hessian evaluations of the (c,l) path program (the throughput form of the H2MC plugin symbols)
void LaunchHessBatch(int c, int l, int n, const float *primarySoA, const float *scene, const float *vertSoA, float *logLum, float *gradSoA, float *hessSoA,
                     hipStream_t s);
// id-ordered work lists of the next step from A.nextKind (coalescing: a wave's 64 list entries are (nearly) consecutive chains)
// sortPlain: group the plain small steps of every 1024-chain tile by technique (QueueNext's key)
void LaunchBuildLists(const lmcd::ChainArrays &A, const lmcd::NextLists &next, int sortPlain, unsigned leanDims, hipStream_t s);
void LaunchInitLists(int n, int *large, int *counts, hipStream_t s);
// pending global-cache pushes of the step just run, all dims in one pass, chain-id order; tileCounts: one word per 1024 chains
void LaunchCachePush(const lmcd::ChainArrays &A, const lmcd::CachePushTargets &T, unsigned long long *tileCounts, int *stageCounts /* zeroed first */, hipStream_t s);
// multi-rank push: append the gathered stages of all ranks (rank order) to the cache rows; see kernels.hip k_push_apply
void LaunchCachePushApply(const float *gathered, size_t stageFloats, int world, const lmcd::PushStageLayout &lay, const lmcd::CachePushTargets &T,
                          int *hostCounts /* pinned; nullptr: the fill counts stay on the device */, hipStream_t s);
// measurement aid: state-layout probe (kernels.hip k_layout_probe)
void LaunchLayoutProbe(int N, int words, int mode, int batch, const float *in, float *out, hipStream_t s);
// groups the entries of a work list by the technique key of A.nextKind (blockHist: 64 ints per 2048 entries of the longest list)
void LaunchSortByTechnique(const unsigned char *nextKind, const int *in, int *out, const int *count, int *blockHist, int maxEntries, hipStream_t s);
// inclusive scan of v[0, n) in place; tileSums: n / 2048 + 1 ints
void LaunchInclusiveScan(int *v, int n, int *tileSums, hipStream_t s);
// chain relocation (relocate.hip): the chains of the step's large-step launch whose technique changed since they were placed are sorted by technique into the slots they occupy
struct RelocBuffers {
    unsigned *placedKey;        // N: the key a slot's chain was placed under (all ones: never placed): the technique key, or with `fine` the 24-bit [technique | screen Morton] key
    int *tileCount, *tileHist;  // RelocTiles(N), 64 x RelocTiles(N): members per 1024-slot tile / per (tile, key); then their exclusive prefixes
    int *members;               // N: the slots that take part, ascending
    int *sorted;                // N: member indices by key
    int *count;                 // 2: number of members (0: the relocation was skipped, its movers exceeded `capacity`), relocations skipped so far
    float *staging;             // RelocRecordWords(maxDepth) floats per member
    int capacity;               // records the staging buffer holds: a step with more movers leaves them where they are (host/context.cpp)
    bool fine;                  // the per-step relocation and the full re-sort place by the fine key (LMC_RELOC_FINE=0: the technique alone, round 4's rule)
};
size_t RelocTiles(int N);
size_t RelocRecordWords(int maxDepth);
void LaunchRelocIota(int n, int *v, hipStream_t s);
// withoutGaussianOnly (H2MC renders): chains that hold a stored Gaussian stay where they are (the pipeline's Gaussian buffers are per slot)
void LaunchRelocate(const lmcd::ChainArrays &A, int maxDepth, const RelocBuffers &B, bool withoutGaussianOnly, hipStream_t s);
// its first half on its own (the three launches that fill B.members / B.sorted / B.count; LaunchRelocate = this + the move): what lmc_reloc_plan_probe runs
void LaunchRelocPlan(const lmcd::ChainArrays &A, int maxDepth, const RelocBuffers &B, bool withoutGaussianOnly, hipStream_t s);
void LaunchRelocFineKey(const lmcd::ChainArrays &A, const int *leafPosOfTri, int numTris, int mode, unsigned long long *keys, const lmcd::TriData *tris, const lmcd::DMaterial *materials, hipStream_t s);
void LaunchRelocMove(const lmcd::ChainArrays &A, int maxDepth, const RelocBuffers &B, hipStream_t s, int keyMode = 0);
// the periodic full re-sort by (technique, screen Morton code): work buffers of the device radix sort
struct RelocSortBuffers {
    unsigned *keys[2];  // N each
    int *vals[2];       // N each
    int *hist;          // 256 x RelocSortBlocks(N)
    int *scanSums;      // 256 x RelocSortBlocks(N) / 2048 + 2
};
size_t RelocSortBlocks(int N);
// the stable 24-bit sort itself: keys in W.keys[0][0 .. *nPtr) (the count lives on the device, at most nMax; W sized for nMax) -> out[p] = index of the p-th key,
// the sorted keys in W.keys[1]; entries from *nPtr on are not written
void LaunchRadixSort24(const RelocSortBuffers &W, const int *nPtr, int nMax, int *out, hipStream_t s);
void LaunchRelocFullSort(const lmcd::ChainArrays &A, int maxDepth, const RelocBuffers &B, const RelocSortBuffers &W, hipStream_t s);
void LaunchRelocateFine(const lmcd::ChainArrays &A, int maxDepth, const RelocBuffers &B, const RelocSortBuffers &W, bool withoutGaussianOnly, hipStream_t s);
// dilated grid of one cache dim on the device (DCacheDim::gridStart / gridRows); buffer sizes in kernels.hip
void LaunchBuildCacheGrid(const float *pts, int n, int dim, int G, int m, const int *coord, int *scratchStart, int *scratchCursor, int *scratchWordCount, int *tileSums,
                          uint2 *words, int *cellStart, unsigned short *idx, hipStream_t s);
// checkpoint records (checkpoint.hip): the chains [first, first + n) of this context as n fixed-size records in chain order (read through A.slotOf), and
// back into the slots [first, first + n) of a freshly set-up identity layout.  h2Gauss: H2Arrays::gauss of an H2MC render, nullptr otherwise
size_t CkptRecordWords(int maxDepth, bool sampleCache, bool h2mc);
void LaunchCkptPack(const lmcd::ChainArrays &A, int maxDepth, bool sampleCache, const float *h2Gauss, int first, int n, float *staging, hipStream_t s);
void LaunchCkptUnpack(const lmcd::ChainArrays &A, int maxDepth, bool sampleCache, float *h2Gauss, int first, int n, const float *staging, hipStream_t s);
// chain diagnostics (chaindiag.hip; host/chaindiag.cpp).  kindOf: one byte per rank-local CHAIN id, the launch (NEXT_*) that runs the chain's current
// step, 0 for a chain in none of the step's work lists
void LaunchLatchKind(const lmcd::ChainArrays &A, const int *large, const int *generic, const int *lean, const int *counts, unsigned char *kindOf, hipStream_t s);
// n rows of 48 words (include/lmc_abi.h LMC_ROW_WORDS), one wave per row; ids: rank-local chain ids in [0, A.N); which: 0 current, 1 init; kindOf may be nullptr
void LaunchChainRows(const lmcd::ChainArrays &A, int which, const int *ids, int n, const unsigned char *kindOf, float *out, hipStream_t s);
// the pending splat lists of n chains (lmc_chain_splats): counts[j] = list length, out[(j * cap + k) * 6 ..] = x, y, r, g, b, label (labels == nullptr: -1)
void LaunchChainSplats(const lmcd::ChainArrays &A, const unsigned char *labels, const int *ids, int n, int cap, float *out, int *counts, hipStream_t s);
// table[3][13][13][2] += the chain-steps of the step just run and those of them that were accepted, by (latched kind - 1, c, l of the state after it)
void LaunchStepTable(const lmcd::ChainArrays &A, const unsigned char *kindOf, unsigned long long *table, hipStream_t s);
