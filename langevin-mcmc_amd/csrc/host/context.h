// The context behind the C ABI (include/lmc_abi.h: lmc_ctx) and what context.cpp -- init, the cache transition, the step path, the group exchange,
// the RCCL binding -- offers the host units beside it: ckpt.cpp, mcrender.cpp, probes.cpp.  Private to csrc/host/.
#pragma once
#include <chrono>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/lmc_abi.h"
#include "../device/kernels.h"
#include "../device/dh2coop.h"
#include "accel.h"
#include "hostutil.h"
#include "mcfilm.h"
#include "scene.h"

// (every unit that sees a context is host code around the lmcd:: launch functions)
using namespace lmcd;
using namespace lmc_host;

namespace lmc_host {

struct CacheDimHost {
    DevBuf<float> pss, v1, v2, weight;
    DevBuf<float> extra, distCdf;  // `samplecache`: the rows' paths + contributions (CACHE_ROW_EXTRA words each), PiecewiseConstant1D over the weights
    DevBuf<KdNode> nodes;
    DevBuf<uint2> gridWords;           // the compact existence grid (dchain.h DCacheDim): occupancy words + ranks,
    DevBuf<int> gridCellStart;         // the candidate range of every non-empty cell,
    DevBuf<unsigned short> gridIdx;    // the candidates' row indices
    int gridG = 0, gridM = 0;
    int gridCoord[4] = {0, 1, 2, 3};  // the coordinates the grid is laid over, chosen from the rows when the dim becomes ready (accel.h ChooseGridCoords)
    DevBuf<int> vind;
    bool ready = false;
    bool relevant = false;
};

int GetRcclDestroy(void *comm);  // RCCL is bound lazily (context.cpp)
struct ChainDiag;                // chaindiag.cpp: the state of the chain diagnostics (trace buffer, kind latch, step table)

}  // namespace lmc_host

struct lmc_ctx {
    std::unique_ptr<lmc::Scene> scene;
    int device = 0;
    int useGradient = 1;
    int maxDervDepth = 8;  // --max-derivatives-depth default, main.cpp:46
    bool useOccFilter = true;  // LMC_OCC_FILTER=0: A/B switch for the existence test in front of the cache query
    int gridDims = 4;          // LMC_GRID_DIMS: rank of its grid (3 or 4)
    bool largeLdsStack = true;  // LMC_LARGE_LDS=0: A/B switch for the LDS traversal stack of the large-step launch
    bool leanLdsStack = true;   // LMC_LEAN_LDS=0: the lean launch on its private-stack instantiations (the fallback of trees deeper than BVH_LDS_STACK) whatever the tree
    int largeBlock = 64;        // LMC_LARGE_BLOCK: its block size (64, 128 or 256); 128 disturbs the lean launch less (its bracket 2.4 instead of 2.7 ms) but the step and the start-up end 1-2 % later (profiles/r02_j_ab_block_sizes.jsonl)
    bool leanGrad = true;      // LMC_LEAN_GRAD=0: the cache-filling launch falls back to k_step<false,true,true,true>
    bool anyDeepCache = false;  // (always false since the LDS search is gone: see DCacheDim::deep)
    bool sortH2mc = true;
    bool sortGeneric = true;   // LMC_SORT_GENERIC=0: A/B switch for the technique sort of the cache-filling launch
    DevBuf<int> listScratch, listScratch2, sortBins, sortBins2;
    int expFlags = 0;      // LMC_EXP_NOSPLAT / LMC_EXP_NOQUERY: measurement aids (dstep_params.h)
    hipStream_t stream = nullptr;
    // The three step launches of one iteration touch disjoint chains, so they run concurrently: large steps and the generic
    // (gradient) small steps on two side streams, the lean small steps on the main stream, joined before k_build_lists.
    // LMC_OVERLAP=0 serialises them on the main stream (A/B).
    hipStream_t sideStream[2] = {nullptr, nullptr};
    static constexpr int H2_MAX_PARTS = 4;
    hipStream_t partStream[H2_MAX_PARTS - 1] = {};  // H2MC: the pipelines of the other parts of the chain population (LaunchGeneric)
    hipEvent_t partFork = nullptr, partJoin[H2_MAX_PARTS - 1] = {};
    hipEvent_t h2HeadDone[H2_MAX_PARTS] = {};  // H2MC: behind each part's k_h2_begin (the large-step launch can be made to wait for them: LMC_H2_LARGE_AFTER)
    int h2HeadParts = 0;
    hipEvent_t forkEvent = nullptr, joinEvent[2] = {nullptr, nullptr};
    hipEvent_t packedEvent = nullptr, copiedEvent = nullptr;  // in-process group: this member's stage is complete / this member has copied every stage (ExchangeStagesAsync)
    // in-process group, film merge (lmc_group_film_reduce): staging for the slices pulled from the peers + the peers' weight sums, allocated when the
    // group is set up (nothing is allocated inside the merge); events: this member's film is final / this member's slice holds the sum
    DevBuf<float> filmStage;
    DevBuf<long long> filmStageFx;  // ... in exact mode (sized for the mode when the group is set up)
    DevBuf<double> weightStage;
    hipEvent_t filmReadyEvent = nullptr, sliceReducedEvent = nullptr, weightsCopiedEvent = nullptr;
    int groupPeerPairs = 0, groupPeerEnabled = 0, groupDevices = 0;  // ordered pairs of distinct member devices / ... with direct peer access enabled (lmc_group_info)
    // host time spent queueing the launches of this member's steps (StepPhase1 + exchange + StepPhase2) and the steps it covers (lmc_host_issue_timing)
    double hostIssueMs = 0;
    long long hostIssueSteps = 0;
    DevBuf<double> commScratch;  // RCCL job: device words of lmc_comm_allreduce_f64 / lmc_comm_barrier, allocated by lmc_comm_init
    bool overlap = true;
    // scene buffers
    DevBuf<BvhNode4> nodes;
    DevBuf<BvhNode4Q> qnodes;
    double thickFlatShare = 0;  // accel.h ThickenedFlatLeafShare of the scene's tree: decides the node format of the hot launches (UploadScene)
    DevBuf<LeafTri> leafTris;
    DevBuf<int> leafPosOfTri;
    DevBuf<TriData> tris;
    DevBuf<DMesh> meshes;
    DevBuf<DMaterial> materials;
    DevBuf<DBitmap> bitmaps;
    DevBuf<float> texPool;  // the texels of every bitmap, back to back
    DevBuf<DLight> lights;
    DevBuf<float> areaFunc, areaCdf, lightFunc, lightCdf, envImage, envCdfRows, envCdfCols, envRowWeights;
    DScene S;
    int bvhDepth = 0;
    int leafHist[8] = {};  // leaves of the uploaded tree that hold 1 .. 8 triangles (lmc_lean_info)
    // film
    DevBuf<float> film, directFilm;
    // exact mode ("film_exact", INTEGRATION.md "Exact film"): the MLT splats go to filmFx, W*H*3 signed 64-bit fixed-point words (unit 2^-32) followed by
    // the film_overflow counter; `film` then only receives the converted floats of lmc_film_read.  directFilm and mcFilm stay float in either mode.
    DevBuf<long long> filmFx;
    bool filmExact = false;
    // the layered MLT film ("film_layers", INTEGRATION.md "Layered MLT film"; exact mode only): the MLT splats go to filmLayersFx, filmNLayers exact films of
    // W*H*3 words one after the other and ONE overflow word behind them, split by path length (1) or technique (2).  filmFx then only receives their sum
    // (SyncLayerSum, in front of every read of it), as `film` receives the converted floats.  splatLabels: the techniques of the pending splat lists, one
    // byte per entry by CHAIN id (dchain.h ChainFilmLayers).  Both allocated by SetUpChains in this mode only.
    int filmLayers = 0;  // the option; fixed once chains are set up, like filmExact
    int filmNLayers = 0;
    DevBuf<long long> filmLayersFx;
    DevBuf<unsigned char> splatLabels;
    DevBuf<float> mcFilm;                  // lmc_mc_render's film (the mc integrator), weighted by 1 / spp
    DevBuf<unsigned long long> mcCounters;  // [paths traced, contributions splatted] of the last lmc_mc_render (exact mode: since the film was last cleared)
    // exact mode of the mc film ("mc_film_exact", INTEGRATION.md "Exact mc film"): the contributions go unweighted to mcFilmFx, W*H*3 fixed-point words followed
    // by the overflow counter; mcFilm then only receives lmc_mc_read's converted floats, divided by mcDivisor (the spp of the last render / accumulate call)
    DevBuf<long long> mcFilmFx;
    bool mcExactOpt = false;   // the option: read by the next lmc_mc_render / lmc_mc_accumulate / lmc_mc_load
    bool mcFilmIsExact = false;  // the mode of the film the context holds
    int mcDivisor = 0;
    lmc::McCoverage mcCoverage;  // the stream ids mcFilmFx holds
    long long mcLaunchStreams = 262144;  // "mc_launch_streams": stream ids per launch of a render / accumulate call, either mode
    int mcLaunches = 0;                  // "mc_launches": launches of the last such call
    // the layered mc film ("mc_layers", INTEGRATION.md "Layered mc film"): mcNLayers films of W*H*3 words one after the other (exact: one overflow word behind
    // them), split by path length (mode 1) or technique (mode 2).  mcFilm / mcFilmFx then hold their sum, made after every render / accumulate call, so
    // every call that reads the film sees the total.
    DevBuf<float> mcLayersF;
    DevBuf<long long> mcLayersFx;
    int mcLayersOpt = 0;   // the option: read by the next lmc_mc_render
    int mcLayerMode = 0;   // the mode of the film the context holds (0: unlayered)
    int mcNLayers = 0;
    int world = 1, rank = 0;          // position in the job (lmc_comm_init: RCCL ranks; lmc_group_chains_init: in-process group)
    std::vector<lmc_ctx *> group;    // in-process group this context is a member of (empty / 1: none)
    bool filmReduced = false;  // the device film + weightSum already hold the all-reduced sums (lmc_film_allreduce is in place)
    void *comm = nullptr;  // ncclComm_t of lmc_comm_init (multi-GPU: one process per GPU, chains sharded by id range)
    // chains
    int N = 0, numChainsTotal = 0, chainBegin = 0;
    // the job's shape as lmc_chains_init was given it, the steps asked for since and the render's wall time before this process took it over: what a
    // checkpoint's header carries besides the fingerprint (lmc_checkpoint_save / _load)
    int forceDiffuse = 0, initThreads = 0;
    long long numInitSamples = 0, perChain = 0, chainsNeedExtra = 0, stepsDone = 0;
    double secondsBefore = 0;
    std::chrono::steady_clock::time_point chainsSince;  // when lmc_chains_init / lmc_checkpoint_load left the chains ready
    unsigned long long sceneHash = 0;                    // content hash of the scene's files, computed by the first save / load
    ChainArrays A;
    DevBuf<uint64_t> rngState;
    DevBuf<uint32_t> rngTab;
    DevBuf<unsigned char> rngTicked;
    DevBuf<float> curPath, pathBuf1, curContrib, scoreSum, gaussian, gaussian1, curSplat, chV1, chV2, chCurrNewV2, chPropNewV1, chPropNewV2, chPss, chLastPss, chPath, chContrib, pathWeight,
        lastScoreSum, lastScore, contribList, pushData, initPath, initContrib, initScoreSum, initLsAll;
    DevBuf<unsigned char> initCLAll;
    DevBuf<unsigned char> nextKind;
    DevBuf<int> flags, curSplatCount, adjacentReject, sampleIdx, numSamples, pushDim;
    DevBuf<unsigned long long> counters, prof;
    bool profileLean = false;  // LMC_PROF=1: the lean launch runs its region-timer instantiation (lmc_prof_read)
    DevBuf<double> weightSum;
    DevBuf<float> gradBuf;
    // H2MC renders: hand-off state of the wave-cooperative pipeline (device/dh2coop.h)
    DevBuf<float> h2Rec, h2Out, h2Gauss, h2Offset, h2Py, h2Px, h2PropContrib;
    DevBuf<int> h2Step, h2Items, h2BinOf, h2Counts, h2SubList, h2SubCount;
    H2Bins h2Bins[H2_MAX_PARTS][2] = {};  // [part][stage]
    int h2Parts = 1, h2PartStride = 0;
    const int *h2SplitOf = nullptr;  // the generic list h2SubList currently holds the two halves of (cut at the end of the step that built it, StepPhase2)
    DevBuf<unsigned char> h2Kind;
    H2Arrays H2{};
    int h2HessGrid = 0, h2GaussGrid = 0;
    // LMC renders with gradients: the cache-filling small steps as a pipeline (dh2coop.h MalaPipe; the buffers above, sized for it); LMC_MALA_PIPE=0: one launch
    bool malaPipe = true;
    MalaPipe MP{};
    int gradStride = 0, stepGrid = 0;
    // launch shape of the lean small-step kernel and the technique sort of its work list; LMC_LEAN_BLOCK / LMC_SORT_PLAIN
    // override them for A/B runs (profiles/)
    int leanBlock = 64, sortPlain = 0;  // (the lean launch runs one chain per thread: its launch function sizes the grid, step_small_plain.hip)
    // chain relocation (device/relocate.hip): the chains kept physically grouped by technique from the first step on (fill phase included: the safety argument is at the launch site, StepPhase1); LMC_RELOCATE overrides
    bool relocate = false;
    DevBuf<int> chainId, slotOf, relocTileCount, relocTileHist, relocMembers, relocSorted, relocCount;
    DevBuf<unsigned> relocPlacedKey;
    DevBuf<unsigned char> stepKind;
    bool relocFine = false;  // LMC_RELOC_FINE=1 (A/B, rejected: profiles/r06_r_*): the per-step relocation sorts its movers by the fine key (relocate.hip k_relf_*)
    DevBuf<float> relocStaging;
    RelocBuffers RB{};
    long long relocations = 0;
    int pendingResort = 0;
    // the periodic full re-sort by (technique, screen Morton code) (relocate.hip): every resortEvery-th step ends with it; 0 = off
    int resortEvery = 0, resortFirst = 0;
    int resortEveryOpt = -1, resortFirstOpt = -1;  // lmc_set_option "resort_every" / "resort_first" (-1: not set)
    long long stepsSinceInit = 0, resorts = 0;
    DevBuf<unsigned> sortKeys[2];
    DevBuf<int> sortVals[2], sortHist, sortScanSums;
    RelocSortBuffers RS{};
    // work lists (double buffered): [parity][large | smallGrad | smallPlain]
    DevBuf<int> lists[2][3], listCounts[2];
    int parity = 0;
    // cache
    CacheDimHost cacheDims[PSS_MAX_LENGTH + 1];
    DCache cacheHost;
    DevBuf<DCache> cacheDev;
    DevBuf<int> cacheCounts;                 // rows filled per slot (dims 6, 8, 10, 12)
    DevBuf<unsigned long long> pushTiles;    // scratch of the push launches: one word per 1024 chains
    DevBuf<int> gridScratchStart, gridScratchCursor, gridScratchWordCount, gridTileSums;  // build-time scratch of the existence grids, sized for the largest dim's cell count (the builds are stream-ordered)
    CachePushTargets pushT;                  // the cache rows themselves
    CachePushTargets stageT;                 // ... and this rank's stage of a step's pushes (same row layout; kernels.hip k_push_apply)
    PushStageLayout stageLayout;
    DevBuf<float> pushStage, pushGather;     // the stage; the stages of all ranks after the exchange
    DevBuf<int> warmCounts;                  // four zeros: the list lengths of the warm-up launches at the end of MLTInit
    int *hostCounts = nullptr;               // pinned mirror of cacheCounts
    hipEvent_t countsEvent = nullptr;        // ... is up to date (CacheApplyLaunch / CacheApplyFinish)
    bool countsInFlight = false, appliedEarly = false;
    // a gradient cache becoming ready (CacheApplyFinish): its rows come down, its existence grid is built and its kd-tree goes up on THIS stream, beside
    // the step's launches; the device's copy of the cache struct is then refreshed from a pinned copy in stream order behind them
    hipStream_t cacheStream = nullptr;
    DCache *cachePinned = nullptr;
    bool earlyApply = true;                  // LMC_EARLY_APPLY=0: a single rank also applies its pushes at the end of the step
    int lastCounts[CACHE_SLOTS] = {0, 0, 0, 0}; // ... as last read back, and the steps run since (CacheApplyLaunch)
    long long stepsSinceCounts = 0;
    // the rows of a dim that is about to fill up, sent to the host behind the apply of the step that is expected to fill it (CacheApplyLaunch): when
    // the counts say "ready" the rows are there already and the kd-tree build starts at once (the fetch was 0.2 ms of a 1.2 ms transition)
    float *rowsPinned[CACHE_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    bool rowsPrefetched[CACHE_SLOTS] = {false, false, false, false};
    int lastDelta[CACHE_SLOTS] = {0, 0, 0, 0};  // rows added per step, as of the last two read-backs
    // ... and the way up: a dim's kd-tree (nodes, then the point order) in a pinned buffer of its own, so that the copies are queued and the host goes on
    // (pageable copies made the host wait for the stream, existence-grid builds included, once per dim: 0.3 ms)
    char *treePinned[CACHE_SLOTS] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t treesUpEvent = nullptr;
    bool allCachesReady = false;
    // the resident schedule (device/step_resident.h, RunResident): 0 = lock step only; K >= 1 = once the caches are frozen, up to K mutations
    // of every chain per launch.  residentLanes: active chains per 64-lane wave ("resident_lanes"; 0 = ResidentLanes' choice); the rest is bookkeeping for
    // lmc_resident_stats
    int residentSteps = 0, residentLanes = 0;
    long long residentLaunches = 0, lockSteps = 0;
    double residentMs = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> residentEvents;  // one pair per resident launch not yet read by lmc_resident_stats
    DevBuf<unsigned long long> residentGuard;                       // [chain-steps of resident launches, steps that would have needed a gradient / push]
    bool residentResortPending = false;                             // a full re-sort is due before the next lock step (relocation on)
    int mutationAtInit = -1;  // (mala, h2mc) the resident chain state was laid out for by lmc_chains_init; lmc_chains_step refuses any other
    // chain diagnostics (chaindiag.cpp; include/lmc_abi.h "Chain diagnostics"): nullptr until a trace is opened or "step_table" is set; owned by the
    // context, freed by lmc_destroy (DiagFree)
    lmc_host::ChainDiag *diag = nullptr;
    bool needGeneric = true;  // some chain may still need the generic small-step launch (gradient / deep cache tree)
    bool genericTokenOnly = false;  // ... but only as the fallback of the lean launch without light sub-paths: a few blocks, no list sort
    // init results
    float normalization = 0.f;
    std::vector<float> lengthFunc, lengthCdf;  // lengthDist of MLTInit (mlt.h:99), read by the multiplexed large step
    float lengthFuncInt = 0.f;
    long long numInitContribs = 0;
    std::vector<unsigned char> initCL;            // MLTInit contributions in stream order (parity probe lmc_init_contribs)
    std::vector<float> initLs;
    std::vector<unsigned long long> initOffsets;  // first contribution of every init sample
    // timing
    struct StepEvents {
        hipEvent_t e[8];  // main stream: step begin | lean launch begin | lean launch end | step end;  side streams: large begin / end, generic begin / end
    };
    // Events are recorded only between lmc_set_option("timing", 1) and the lmc_step_timing call that reads them, and come
    // from a pool that is reused: a render that never asks for timings (dpt_amd) creates none.
    bool timing = false;
    std::vector<StepEvents> events, eventPool;
    double smallMs = 0, largeMs = 0, largeOnlyMs = 0, genericMs = 0;  // accumulated by lmc_step_timing for lmc_kernel_timing / lmc_kernel_timing_split
    ~lmc_ctx() {
        for (lmc_ctx *peer : group)  // the other members of an in-process group hold raw pointers to this context
            if (peer != this) {
                peer->group.clear();
                peer->world = 1, peer->rank = 0;
            }
        for (auto *v : {&events, &eventPool})
            for (auto &ev : *v)
                for (auto e : ev.e) (void)hipEventDestroy(e);
        if (comm) {
            try {
                (void)GetRcclDestroy(comm);
            } catch (...) {
            }
        }
        if (hostCounts) (void)hipHostFree(hostCounts);
        for (float *r : rowsPinned)
            if (r) (void)hipHostFree(r);
        for (char *r : treePinned)
            if (r) (void)hipHostFree(r);
        if (treesUpEvent) (void)hipEventDestroy(treesUpEvent);
        if (cachePinned) (void)hipHostFree(cachePinned);
        for (auto e : h2HeadDone)
            if (e) (void)hipEventDestroy(e);
        if (cacheStream) (void)hipStreamDestroy(cacheStream);
        if (countsEvent) (void)hipEventDestroy(countsEvent);
        for (auto st : partStream)
            if (st) (void)hipStreamDestroy(st);
        for (auto e : {partFork, partJoin[0], partJoin[1], partJoin[2], forkEvent, joinEvent[0], joinEvent[1], packedEvent, copiedEvent, filmReadyEvent, sliceReducedEvent, weightsCopiedEvent})
            if (e) (void)hipEventDestroy(e);
        for (auto st : sideStream)
            if (st) (void)hipStreamDestroy(st);
        for (auto &e : residentEvents) (void)hipEventDestroy(e.first), (void)hipEventDestroy(e.second);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace lmc_host {

// what the chains of a context are set up from, after MLTInit or from a checkpoint: the job's shape and the job-wide (technique, lsScore) tables
struct ChainSetUp {
    int numChainsTotal = 0, chainBegin = 0, chainEnd = 0;
    long long perChain = 0, chainsNeedExtra = 0;
    const std::vector<float> *seedLs = nullptr;
    const std::vector<unsigned char> *seedCL = nullptr;
    bool fromCheckpoint = false;  // the init states and the chains' words come from records (checkpoint.hip) instead of the init-state regeneration
};

// The material records and the bitmaps as the device reads them: what UploadScene (context.cpp) puts into DScene::materials / texPool / bitmaps, and
// what the shading probe (shade_probes.cpp) looks its textures up through.  `mats` are final -- with LMC_TEX_INLINE a textured reference already names
// its texels' word offset in `pool` and carries width / height / gamma --, `pool` holds at least one word.
struct PackedMaterials {
    std::vector<DMaterial> mats;
    std::vector<float> pool;
    std::vector<size_t> poolOff;  // first word of every bitmap in `pool`
    int glossy = 0;               // any non-Lambertian record
};
PackedMaterials PackMaterials(const std::vector<lmc::Material> &materials, const std::vector<lmc::Bitmap> &bitmaps);
// DScene::bitmaps for a pool that lives at devPool (at least one entry)
std::vector<DBitmap> BitmapHeaders(const PackedMaterials &pm, const std::vector<lmc::Bitmap> &bitmaps, const float *devPool);

// context.cpp, for ckpt.cpp (a load sets the chains up, publishes the cache dims its file holds ready and builds the next step's lists) and mcrender.cpp
void SetUpChains(lmc_ctx *c, const ChainSetUp &U);
void GroupSetUpMerge(const std::vector<lmc_ctx *> &g);
void UploadCacheStruct(lmc_ctx *c, hipStream_t after = nullptr);
bool CachePending(lmc_ctx *c);
void PublishCacheDim(lmc_ctx *c, int d, const lmc::KdTreeResult &t, hipStream_t s);
StepParams MakeStepParams(const lmc_ctx *c);
void BuildNextLists(lmc_ctx *c, int nxt);
int ResidentK(const lmc_ctx *c);
// chaindiag.cpp, for context.cpp: the hooks of the step path, each behind `if (c->diag)` at its call site
void DiagStepBegin(lmc_ctx *c, int cur);    // head of StepPhase1, step stream: the kind latch from the work lists lists[cur]
void DiagStepEnd(lmc_ctx *c);               // StepPhase2, behind the step's launches, ahead of the full re-sort and the list build: trace rows, step table
bool DiagNeedsLockStep(const lmc_ctx *c);   // a trace is open or the step table is on: no resident launches
void DiagChainsReset(lmc_ctx *c);           // SetUpChains (lmc_chains_init, lmc_checkpoint_load): closes an open trace, sizes the latch for the new chains
void DiagSetStepTable(lmc_ctx *c, bool on);  // lmc_set_option "step_table"
bool DiagStepTableOn(const lmc_ctx *c);
void DiagFree(lmc_ctx *c);
// filmlayers.cpp (the layered MLT film, "film_layers"), for context.cpp and ckpt.cpp
ChainFilmLayers LayeredFilm(const lmc_ctx *c);                // the film the layered step launches splat into
void LayersCheckInit(const lmc_ctx *c, const char *what);     // lmc_chains_init / lmc_group_chains_init: the mode needs film_exact and refuses H2MC; throws before anything changes
void LayersAlloc(lmc_ctx *c);                                  // SetUpChains: the layers (zeroed) and the label array, or nothing with the mode off
void SyncLayerSum(lmc_ctx *c);                                 // filmFx = the sum of the layers, overflow word included (stream-ordered; nothing with the mode off)
void RefuseLayered(const lmc_ctx *c, const char *what, const char *why);  // throws "<what>: ... film_layers ..." while the mode is on
// ckpt.cpp, for mcrender.cpp (a state file of the mc film carries the same fingerprint)
uint64_t HashSceneFiles(const lmc::Scene &sc);

}  // namespace lmc_host
