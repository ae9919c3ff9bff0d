// The batch calls and the test probes of the ABI (include/lmc_abi.h) that are no part of a render: the batched path program, single kernels and device
// functions on caller-given arrays, checkers of a context's caches, the host-only hooks of the sharded init plan and of the scene front end.  Host
// logic only; the probes of the bookkeeping launches are in list_probes.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/lmc_abi.h"
#include "../device/drng.h"
#include "../device/kernels.h"
#include "../device/dh2coop.h"
#include "../device/dh2mc.h"
#include "accel.h"
#include "context.h"
#include "hostutil.h"
#include "scene.h"
#include "shardplan.h"

extern "C" {

// ---- CPU test hooks (no GPU): the host-side plan of the sharded MLTInit (shardplan.h), from the very blocks the ranks exchange
int lmc_shard_layout(int world, int rank, int initThreads, long long numInitSamples, long long *out5) {
    LMC_TRY
    if (world < 1 || rank < 0 || rank >= world || initThreads < 1) throw std::runtime_error("lmc_shard_layout: bad arguments");
    const lmc::ShardLayout L = lmc::MakeShardLayout(world, rank, initThreads, numInitSamples);
    out5[0] = L.t0, out5[1] = L.t1, out5[2] = L.g0, out5[3] = L.g1, out5[4] = L.maxLocalSamples;
    return 0;
    LMC_CATCH(-1)
}
int lmc_shard_counts_probe(int world, int initThreads, long long numInitSamples, const unsigned char *paddedCounts, long long maxLocalSamples,
                           unsigned long long *rankFirst) {
    LMC_TRY
    std::vector<unsigned long long> hOff, rf;
    lmc::AssembleCounts(world, initThreads, numInitSamples, paddedCounts, maxLocalSamples, hOff, rf);
    for (int r = 0; r <= world; r++) rankFirst[r] = rf[r];
    return 0;
    LMC_CATCH(-1)
}
int lmc_shard_plan_probe(int world, int initThreads, long long numInitSamples, int numChainsTotal, const unsigned char *paddedCounts, long long maxLocalSamples,
                         const unsigned char *paddedCL, const float *paddedLs, long long maxLocalContribs, long long *seedSample, unsigned char *seedCL,
                         float *seedLs, int *ownedBegin, float *normalization) {
    LMC_TRY
    std::vector<unsigned long long> hOff, rf;
    lmc::AssembleCounts(world, initThreads, numInitSamples, paddedCounts, maxLocalSamples, hOff, rf);
    const unsigned long long total = rf[world];
    if ((long long)total < numChainsTotal) throw std::runtime_error("MLT initialization failed, consider using a larger number of initial samples or smaller number of chains");
    std::vector<unsigned char> cl(total);
    std::vector<float> ls(total);
    lmc::AssembleBlocks(world, rf, paddedCL, (unsigned long long)maxLocalContribs, 1, cl.data());
    lmc::AssembleBlocks(world, rf, paddedLs, (unsigned long long)maxLocalContribs, sizeof(float), ls.data());
    std::vector<uint32_t> hostTab(64);
    Rng hr;
    hr.tab = hostTab.data();
    hr.state = PcgSeed((uint64_t)total, hr.tab);
    hr.ticks = 0;
    std::vector<long long> ss;
    std::vector<unsigned char> sc;
    std::vector<float> sl;
    float norm = 0.f;
    lmc::SeedWalk(numInitSamples, numChainsTotal, hOff, cl.data(), ls.data(), [](void *r) { return ((Rng *)r)->Uniform(); }, &hr, ss, sc, sl, norm);
    const std::vector<int> ob = lmc::OwnedRanges(world, initThreads, numInitSamples, ss);
    for (int i = 0; i < numChainsTotal; i++) seedSample[i] = ss[i], seedCL[i] = sc[i], seedLs[i] = sl[i];
    for (int r = 0; r <= world; r++) ownedBegin[r] = ob[r];
    *normalization = norm;
    return 0;
    LMC_CATCH(-1)
}

// ---- batched path program (context-free)
int lmc_grad_batch(int c, int l, int n, const float *primarySoA, const float *scene38, const float *vertSoA, float *loglum, float *gradSoA) {
    LMC_TRY
    if (!(c >= 1 && l >= 0 && c + l >= 3 && c + l - 1 <= 8)) throw std::runtime_error("lmc_grad_batch: technique (c,l) out of range");
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) EnsureDevice(0);
    else EnsureDevice(dev);
    const int L = std::max(c + l - 1, 2), V = 238 + 59 * (c + l - 3);
    DevBuf<float> dPrim, dScene, dVert, dLL, dGrad;
    dPrim.Upload(primarySoA, (size_t)(2 * L + 1) * n), dScene.Upload(scene38, 38), dVert.Upload(vertSoA, (size_t)V * n);
    dLL.Alloc(n), dGrad.Alloc((size_t)2 * L * n);
    LaunchGradBatch(c, l, n, dPrim.p, dScene.p, dVert.p, dLL.p, dGrad.p, gradSoA ? 1 : 0, 0);
    HIP_CHECK(hipDeviceSynchronize());
    if (loglum) HIP_CHECK(hipMemcpy(loglum, dLL.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (gradSoA) HIP_CHECK(hipMemcpy(gradSoA, dGrad.p, (size_t)2 * L * n * 4, hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}

// gradient + Hessian batch (H2MC): hess_soa[(2L)^2 * n], entry (i,k) of item j at [(i * 2L + k) * n + j]
int lmc_hess_batch(int c, int l, int n, const float *primarySoA, const float *scene38, const float *vertSoA, float *loglum, float *gradSoA, float *hessSoA) {
    LMC_TRY
    if (!(c >= 1 && l >= 0 && c + l >= 3 && c + l - 1 <= 8)) throw std::runtime_error("lmc_hess_batch: technique (c,l) out of range");
    if (!hessSoA) throw std::runtime_error("lmc_hess_batch: null output");
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) EnsureDevice(0);
    else EnsureDevice(dev);
    const int L = std::max(c + l - 1, 2), V = 238 + 59 * (c + l - 3), dim = 2 * L;
    DevBuf<float> dPrim, dScene, dVert, dLL, dGrad, dHess;
    dPrim.Upload(primarySoA, (size_t)(2 * L + 1) * n), dScene.Upload(scene38, 38), dVert.Upload(vertSoA, (size_t)V * n);
    dLL.Alloc(n), dGrad.Alloc((size_t)dim * n), dHess.Alloc((size_t)dim * dim * n);
    LaunchHessBatch(c, l, n, dPrim.p, dScene.p, dVert.p, dLL.p, dGrad.p, dHess.p, 0);
    HIP_CHECK(hipDeviceSynchronize());
    if (loglum) HIP_CHECK(hipMemcpy(loglum, dLL.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (gradSoA) HIP_CHECK(hipMemcpy(gradSoA, dGrad.p, (size_t)dim * n * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hessSoA, dHess.p, (size_t)dim * dim * n * 4, hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}

// ---- probes
// exp / log / pow of device/dtrans.h on the device (mode 0 / 1 / 2): the GPU side of the bit-equality test against the host build
int lmc_trans_probe(int n, int mode, const float *x, const float *y, float *out) {
    LMC_TRY
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) EnsureDevice(0);
    else EnsureDevice(dev);
    DevBuf<float> dx, dy, dout;
    dx.Upload(x, n), dy.Upload(y, n), dout.Alloc(n);
    LaunchTransProbe(n, mode, dx.p, dy.p, dout.p, 0);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}
// LMC_TRACE_TIGHT=1 (read at every call): the two ray probes walk the tree as the three-wave lean launches do (two leaf triangles per round)
static bool TraceTight() {
    const char *e = getenv("LMC_TRACE_TIGHT");
    return e && atoi(e) != 0;
}
int lmc_trace(lmc_ctx *c, int n, const float *rays, int *prim, float *t) {
    LMC_TRY
    DevBuf<float> dR, dT;
    DevBuf<int> dP;
    dR.Upload(rays, (size_t)n * 8), dT.Alloc(n), dP.Alloc(n);
    LaunchTrace(c->S, n, dR.p, dP.p, dT.p, 0, TraceTight(), c->stream);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(prim, dP.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(t, dT.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}
int lmc_occluded(lmc_ctx *c, int n, const float *rays, int *occ) {
    LMC_TRY
    DevBuf<float> dR, dT;
    DevBuf<int> dP;
    dR.Upload(rays, (size_t)n * 8), dT.Alloc(n), dP.Alloc(n);
    LaunchTrace(c->S, n, dR.p, dP.p, dT.p, 1, TraceTight(), c->stream);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(occ, dP.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}
int lmc_rng_probe(int nSeeds, const unsigned long long *seeds, int mode, int n, float mean, float stddev, unsigned *out) {
    LMC_TRY
    EnsureDevice(0);
    DevBuf<unsigned long long> dS;
    DevBuf<uint32_t> dTab, dOut;
    dS.Upload(seeds, nSeeds), dTab.Alloc((size_t)nSeeds * 64), dOut.Alloc((size_t)nSeeds * (n + 66));
    LaunchRngProbe(nSeeds, dS.p, mode, n, mean, stddev, dTab.p, dOut.p, 0);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, dOut.p, dOut.n * 4, hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}
// test hook: the device's nine-way monotone search over cdf[0..n) for nq keys (tests compare with numpy.searchsorted)
int lmc_lower_bound_probe(int n, const float *cdf, int nq, const float *u, int *out) {
    LMC_TRY
    EnsureDevice(0);
    DevBuf<float> dC, dU;
    DevBuf<int> dO;
    dC.Upload(cdf, n), dU.Upload(u, nq), dO.Alloc(nq);
    LaunchLowerBoundProbe(n, dC.p, nq, dU.p, dO.p, 0);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, dO.p, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}
int lmc_stream_probe(long long nWords, int reps) {
    LMC_TRY
    EnsureDevice(0);
    DevBuf<float> a, b;
    a.Alloc((size_t)nWords), b.Alloc((size_t)nWords, false);
    for (int r = 0; r < reps; r++) LaunchStreamProbe(nWords, a.p, b.p, 0);
    HIP_CHECK(hipDeviceSynchronize());
    return 0;
    LMC_CATCH(-1)
}
// test hook, no device needed: the LDS plan of the lean small-step launch for a tree with the given stack need (device/dsmall.h)
int lmc_lean_plan_probe(int bvhStackNeed, int blockThreads, int *stackWords, int *ldsWordsPerThread, long long *ldsBytesPerBlock) {
    LMC_TRY
    if (bvhStackNeed < 0 || blockThreads < 64 || !stackWords || !ldsWordsPerThread || !ldsBytesPerBlock) throw std::runtime_error("lmc_lean_plan_probe: bad arguments");
    LeanLaunchPlan(bvhStackNeed, blockThreads, stackWords, ldsWordsPerThread, ldsBytesPerBlock);
    return 0;
    LMC_CATCH(-1)
}
// what the context's lean small-step launch is: the tree's leaves by size, its stack need and LDS stack words, the instantiation of k_step_small
// (step_small_plain.hip LeanFormOf: the function the launch itself asks) and the block size
int lmc_lean_info(lmc_ctx *c, int *out16) {
    LMC_TRY
    if (!c || !out16) throw std::runtime_error("lmc_lean_info: bad arguments");
    for (int k = 0; k < 8; k++) out16[k] = c->leafHist[k];
    const LeanForm f = LeanFormOf(c->S, c->bvhDepth, c->S.glossy != 0, c->leanLdsStack, c->profileLean);
    int sw, wpt;
    long long bytes;
    LeanLaunchPlan(c->bvhDepth, c->leanBlock, &sw, &wpt, &bytes);
    out16[8] = c->bvhDepth, out16[9] = sw, out16[10] = f.lds, out16[11] = f.glossy, out16[12] = f.lightless, out16[13] = f.quant, out16[14] = f.tight, out16[15] = c->leanBlock;
    return 0;
    LMC_CATCH(-1)
}
// measurement aid: milliseconds per launch of the state-layout probe (kernels.hip k_layout_probe)
int lmc_layout_probe(int nChains, int words, int mode, int batch, int reps, double *msPerLaunch) {
    LMC_TRY
    EnsureDevice(0);
    DevBuf<float> a, b;
    a.Alloc((size_t)nChains * words), b.Alloc((size_t)nChains * words, false);
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    LaunchLayoutProbe(nChains, words, mode, batch, a.p, b.p, 0);
    HIP_CHECK(hipEventRecord(e0, 0));
    for (int r = 0; r < reps; r++) LaunchLayoutProbe(nChains, words, mode, batch, a.p, b.p, 0);
    HIP_CHECK(hipEventRecord(e1, 0));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    *msPerLaunch = ms / reps;
    HIP_CHECK(hipEventDestroy(e0));
    HIP_CHECK(hipEventDestroy(e1));
    return 0;
    LMC_CATCH(-1)
}
int lmc_kd_probe(int dim, int npts, const float *pts, int nq, const float *q, float radiusSq, int knn, int *outN, int *outIdx, float *outDist) {
    LMC_TRY
    EnsureDevice(0);
    if (dim < 1 || dim > MAXPSS || knn > 8) throw std::runtime_error("lmc_kd_probe: bad arguments");
    lmc::KdTreeResult t = lmc::BuildKdTree(pts, npts, dim);
    DevBuf<KdNode> dN;
    DevBuf<int> dV, dOutN, dOutI;
    DevBuf<float> dP, dQ, dOutD;
    dN.Upload(t.nodes), dV.Upload(t.vind), dP.Upload(pts, (size_t)npts * dim), dQ.Upload(q, (size_t)nq * dim);
    dOutN.Alloc(nq), dOutI.Alloc((size_t)nq * knn), dOutD.Alloc((size_t)nq * knn);
    DCacheDim C;
    memset(&C, 0, sizeof(C));
    C.ready = 1, C.nodes = dN.p, C.vind = dV.p, C.pts = dP.p, C.v1 = dP.p, C.v2 = dP.p;
    for (int k = 0; k < dim; k++) C.rootLow[k] = t.rootLow[k], C.rootHigh[k] = t.rootHigh[k];
    LaunchKdProbe(C, dim, nq, dQ.p, radiusSq, knn, dOutN.p, dOutI.p, dOutD.p, 0);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(outN, dOutN.p, (size_t)nq * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(outIdx, dOutI.p, (size_t)nq * knn * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(outDist, dOutD.p, (size_t)nq * knn * 4, hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}
// parity probe: the rows of one cache dim as they stand (pss: PSS_MAX_SIZE x dim, weight: PSS_MAX_SIZE, extra: PSS_MAX_SIZE x
// CACHE_ROW_EXTRA = every row's DPath words followed by its Contrib words, only with `samplecache`; any pointer may be NULL).
// Returns the number of rows filled, -1 on error.
// test probe: n caller-given splats through the device's Splat (dchain.h) into a fresh W x H film, one launch of n lanes in 64-thread blocks.
// exact != 0: out_fixed receives the W*H*3 fixed-point words, *overflow the dropped splats; out_float the film as lmc_film_read returns it
// (exact: converted from the words on the device).  Any of the three outputs may be NULL.
int lmc_film_splat_probe(int W, int H, int n, const float *screen_xy, const float *rgb, int exact, long long *out_fixed, float *out_float, long long *overflow) {
    LMC_TRY
    EnsureDevice(0);
    if (W <= 0 || H <= 0 || n < 0 || (long long)W * H > (1ll << 26)) throw std::runtime_error("lmc_film_splat_probe: bad film size or splat count");
    const size_t words = (size_t)W * H * 3;
    DevBuf<float> dXY, dRGB, dFilm;
    DevBuf<long long> dFx;
    dXY.Upload(screen_xy, (size_t)n * 2), dRGB.Upload(rgb, (size_t)n * 3), dFilm.Alloc(words);
    if (exact) dFx.Alloc(words + 1);
    if (n > 0) LaunchFilmSplatProbe(exact ? FilmFx(dFx.p, W, H) : Film{dFilm.p, W, H}, n, dXY.p, dRGB.p, 0);
    if (exact) LaunchFilmFixedToFloat(dFx.p, dFilm.p, words, 0);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    if (out_float) HIP_CHECK(hipMemcpy(out_float, dFilm.p, words * sizeof(float), hipMemcpyDeviceToHost));
    if (out_fixed) {
        if (!exact) throw std::runtime_error("lmc_film_splat_probe: the fixed-point words exist in exact mode only");
        HIP_CHECK(hipMemcpy(out_fixed, dFx.p, words * sizeof(long long), hipMemcpyDeviceToHost));
    }
    if (overflow) {
        *overflow = 0;
        if (exact) HIP_CHECK(hipMemcpy(overflow, dFx.p + words, sizeof(long long), hipMemcpyDeviceToHost));
    }
    return 0;
    LMC_CATCH(-1)
}

int lmc_cache_rows(lmc_ctx *c, int dim, float *pss, float *weight, float *extra) {
    LMC_TRY
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (dim < 6 || dim > PSS_MAX_LENGTH || (dim & 1) || !c->cacheDims[dim].relevant) return -1;
    CacheDimHost &cd = c->cacheDims[dim];
    if (pss) HIP_CHECK(hipMemcpy(pss, cd.pss.p, (size_t)PSS_MAX_SIZE * dim * sizeof(float), hipMemcpyDeviceToHost));
    if (weight) HIP_CHECK(hipMemcpy(weight, cd.weight.p, (size_t)PSS_MAX_SIZE * sizeof(float), hipMemcpyDeviceToHost));
    if (extra) {
        if (!cd.extra.p) return -1;
        HIP_CHECK(hipMemcpy(extra, cd.extra.p, (size_t)PSS_MAX_SIZE * CACHE_ROW_EXTRA * sizeof(float), hipMemcpyDeviceToHost));
    }
    int counts[CACHE_SLOTS];
    HIP_CHECK(hipMemcpy(counts, c->cacheCounts.p, sizeof(counts), hipMemcpyDeviceToHost));
    return counts[(dim - 6) / 2];
    LMC_CATCH(-1)
}
// parity probe of LargeStepCache's cache-side pieces on the device (`samplecache`, the dim must be ready): row[i] = sampleCache with
// the uniform u[i] (global_cache.h:126-137), pdf[i] = evalPdfCache(query[i * dim ..], technique cl[2 i], cl[2 i + 1]) (:139-164).
// Returns 0, -2 when the dim is not ready or the option is off, -1 on error.
int lmc_cache_probe(lmc_ctx *c, int dim, int n, const float *u, int *row, const float *query, const int *cl, float *pdf) {
    LMC_TRY
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (dim < 6 || dim > PSS_MAX_LENGTH || (dim & 1) || !c->cacheDims[dim].ready || !c->S.opt.sampleCache || !c->cacheDims[dim].extra.p) return -2;
    DevBuf<float> du, dq, dp;
    DevBuf<int> dr, dcl;
    du.Upload(u, n), dq.Upload(query, (size_t)n * dim), dcl.Upload(cl, (size_t)2 * n), dr.Alloc(n), dp.Alloc(n);
    LaunchCacheProbe(c->cacheDev.p, dim, n, du.p, dr.p, dq.p, dcl.p, dp.p, c->stream);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(row, dr.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(pdf, dp.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}
// checker of the device-built grid of one cache dim against the host build (accel.cpp): returns the number of cells whose row
// sets differ (0 = identical), -1 on error, -2 when that dim's cache is not ready
int lmc_cache_grid_check(lmc_ctx *c, int dim) {
    LMC_TRY
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (dim < 0 || dim > PSS_MAX_LENGTH || !c->cacheDims[dim].ready) return -2;
    CacheDimHost &cd = c->cacheDims[dim];
    std::vector<float> pts = cd.pss.Download();
    lmc::CacheGrid g = lmc::BuildCacheGrid(pts.data(), PSS_MAX_SIZE, dim, cd.gridM, cd.gridCoord);
    if (g.G != cd.gridG) return 1 << 30;
    std::vector<uint2> words = cd.gridWords.Download();
    std::vector<int> cellStart = cd.gridCellStart.Download();
    std::vector<unsigned short> idx = cd.gridIdx.Download();
    int bad = 0, rank = 0;
    const size_t cells = g.start.size() - 1;
    for (size_t cell = 0; cell < cells; cell++) {
        const uint2 w = words[cell >> 5];
        const bool occupied = (w.x >> (cell & 31)) & 1u;
        if ((cell & 31) == 0 && (int)w.y != rank) {  // the word's rank = non-empty cells before it
            bad++;
            rank = (int)w.y;
        }
        if (occupied != (g.start[cell + 1] > g.start[cell])) {
            bad++;
            if (occupied) rank++;
            continue;
        }
        if (!occupied) continue;
        const int s0 = cellStart[rank], s1 = cellStart[rank + 1];
        rank++;
        if (s1 - s0 != g.start[cell + 1] - g.start[cell]) {
            bad++;
            continue;
        }
        std::vector<std::vector<float>> dv, hv;  // the same set of rows (the device lists indices into the point table, in the order of its atomics)
        for (int j = s0; j < s1; j++) dv.emplace_back(pts.begin() + (size_t)idx[j] * dim, pts.begin() + (size_t)(idx[j] + 1) * dim);
        for (int j = g.start[cell]; j < g.start[cell + 1]; j++) hv.emplace_back(g.rows.begin() + (size_t)j * dim, g.rows.begin() + (size_t)(j + 1) * dim);
        std::sort(dv.begin(), dv.end()), std::sort(hv.begin(), hv.end());
        if (dv != hv) bad++;
    }
    return bad;
    LMC_CATCH(-1)
}

// Host-only (no GPU): what the front end made of a scene file, as one JSON document -- the cross-check surface of the parsers (XML, .serialized,
// OBJ, textures) against independent ones (tests/test_scene_io.py).  Returns the document's length (it is truncated to cap - 1 characters), -1 on error.
long long lmc_scene_dump(const char *scene_xml, int force_diffuse, char *out, long long cap) {
    LMC_TRY
    lmc::LoadOverrides ov;
    ov.forceDiffuse = force_diffuse != 0;
    std::unique_ptr<lmc::Scene> sc = lmc::ParseScene(scene_xml, ov);
    std::string j;
    char buf[512];
    auto num = [&](double v) {
        snprintf(buf, sizeof(buf), "%.9g", v);
        j += buf;
    };
    auto vec = [&](const float *v, int n) {
        j += "[";
        for (int k = 0; k < n; k++) {
            if (k) j += ",";
            num(v[k]);
        }
        j += "]";
    };
    auto tex = [&](const lmc::TextureRef &t) {
        j += "{\"bitmap\":";
        if (t.bitmap >= 0) {
            const lmc::Bitmap &b = sc->bitmaps[t.bitmap];
            std::string fn = b.filename;
            const size_t slash = fn.find_last_of('/');
            if (slash != std::string::npos) fn = fn.substr(slash + 1);
            j += "\"" + fn + "\",\"width\":" + std::to_string(b.img.width) + ",\"height\":" + std::to_string(b.img.height) + ",\"gamma\":";
            num(b.gamma);
            j += ",\"average\":";
            vec(b.avg, 3);
        } else {
            j += "null";
        }
        j += ",\"value\":";
        vec(t.value, 3);
        j += ",\"s_scale\":";
        num(t.sScale);
        j += ",\"t_scale\":";
        num(t.tScale);
        j += "}";
    };
    j += "{\"num_tris\":" + std::to_string(sc->numTris()) + ",\"meshes\":[";
    for (size_t m = 0; m < sc->meshes.size(); m++) {
        const lmc::Mesh &M = sc->meshes[m];
        if (m) j += ",";
        const float bmin[3] = {M.bmin.x, M.bmin.y, M.bmin.z}, bmax[3] = {M.bmax.x, M.bmax.y, M.bmax.z};
        j += "{\"tris\":" + std::to_string(M.numTris()) + ",\"verts\":" + std::to_string(M.P.size()) + ",\"has_normals\":" + (M.N.empty() ? "false" : "true") + ",\"has_st\":" + (M.ST.empty() ? "false" : "true");
        double area = 0;  // sum of the triangle areas, in double (Mesh::totalArea exists for emitters only)
        for (size_t t = 0; t < M.numTris(); t++) {
            const lmc::V3 &a = M.P[M.idx[3 * t]], &b = M.P[M.idx[3 * t + 1]], &c = M.P[M.idx[3 * t + 2]];
            const double e1[3] = {(double)b.x - a.x, (double)b.y - a.y, (double)b.z - a.z}, e2[3] = {(double)c.x - a.x, (double)c.y - a.y, (double)c.z - a.z};
            const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
            area += 0.5 * std::sqrt(cx * cx + cy * cy + cz * cz);
        }
        j += ",\"material\":" + std::to_string(M.material) + ",\"area_light\":" + std::to_string(M.areaLight) + ",\"area\":";
        num(area);
        j += ",\"emitter_total_area\":";
        num(M.totalArea);
        j += ",\"bmin\":";
        vec(bmin, 3);
        j += ",\"bmax\":";
        vec(bmax, 3);
        j += "}";
    }
    j += "],\"materials\":[";
    for (size_t m = 0; m < sc->materials.size(); m++) {
        const lmc::Material &M = sc->materials[m];
        if (m) j += ",";
        j += "{\"type\":" + std::to_string(M.type) + ",\"two_sided\":" + (M.twoSided ? "true" : "false") + ",\"kd\":";
        tex(M.Kd);
        j += ",\"ks\":";
        tex(M.Ks);
        j += ",\"kt\":";
        tex(M.Kt);
        j += ",\"exp_or_alpha\":";
        tex(M.expOrAlpha);
        j += ",\"eta\":";
        num(M.eta);
        j += ",\"ks_weight\":";
        num(M.KsWeight);
        j += "}";
    }
    j += "],\"lights\":[";
    for (size_t l = 0; l < sc->lights.size(); l++) {
        const lmc::Light &L = sc->lights[l];
        if (l) j += ",";
        const float rad[3] = {L.radiance.x, L.radiance.y, L.radiance.z}, inten[3] = {L.intensity.x, L.intensity.y, L.intensity.z}, pos[3] = {L.position.x, L.position.y, L.position.z};
        j += "{\"type\":" + std::to_string(L.type) + ",\"sampling_weight\":";
        num(L.samplingWeight);
        j += ",\"mesh\":" + std::to_string(L.mesh) + ",\"radiance\":";
        vec(rad, 3);
        j += ",\"intensity\":";
        vec(inten, 3);
        j += ",\"position\":";
        vec(pos, 3);
        j += ",\"env_width\":" + std::to_string(L.image.width) + ",\"env_height\":" + std::to_string(L.image.height) + ",\"env_normalization\":";
        num(L.sampleInfo.normalization);
        j += "}";
    }
    j += "],\"env_light\":" + std::to_string(sc->envLight) + ",\"light_cdf\":";
    vec(sc->lightCdf.data(), (int)sc->lightCdf.size());
    j += ",\"light_func_int\":";
    num(sc->lightFuncInt);
    const float c3[3] = {sc->bsphereCenter.x, sc->bsphereCenter.y, sc->bsphereCenter.z};
    j += ",\"bsphere_center\":";
    vec(c3, 3);
    j += ",\"bsphere_radius\":";
    num(sc->bsphereRadius);
    const lmc::Camera &C = sc->camera;
    j += ",\"camera\":{\"width\":" + std::to_string(C.width) + ",\"height\":" + std::to_string(C.height) + ",\"fov\":";
    num(C.fov);
    j += ",\"near\":";
    num(C.nearClip);
    j += ",\"far\":";
    num(C.farClip);
    const lmc::DptOptions &o = sc->options;
    j += "},\"options\":{\"spp\":" + std::to_string(o.spp) + ",\"numinitsamples\":" + std::to_string(o.numInitSamples) + ",\"maxdepth\":" + std::to_string(o.maxDepth) + ",\"mindepth\":" + std::to_string(o.minDepth) +
         ",\"directspp\":" + std::to_string(o.directSpp) + ",\"numchains\":" + std::to_string(o.numChains) + ",\"mala\":" + (o.mala ? "true" : "false") + ",\"h2mc\":" + (o.h2mc ? "true" : "false") + ",\"largestepprob\":";
    num(o.largeStepProbability);
    j += ",\"largestepscale\":";
    num(o.largeStepProbScale);
    j += ",\"perturbstddev\":";
    num(o.perturbStdDev);
    j += "},\"output\":\"" + sc->outputName + "\"}";
    if (out && cap > 0) {
        const size_t n = std::min<size_t>(j.size(), (size_t)cap - 1);
        memcpy(out, j.data(), n);
        out[n] = 0;
    }
    return (long long)j.size();
    LMC_CATCH(-1)
}

// host-only probe of the existence test in front of the cache query (accel.cpp BuildCacheGrid + the kernel's candidate loop):
// out[i] = 1 iff some cache point lies within the radius of query i.  No device needed.
int lmc_cache_filter_probe(int dim, int npts, const float *pts, int nq, const float *q, int *out) {
    LMC_TRY
    if (dim < 3 || dim > MAXPSS) throw std::runtime_error("lmc_cache_filter_probe: bad dim");
    bool first = true;
    const int lead[4] = {0, 1, 2, 3};
    for (int m = 3; m <= 4; m++)  // both grid ranks the kernel can be configured with ...
        for (int chosen = 0; chosen < 2; chosen++) {  // ... over the leading coordinates and over the ones ChooseGridCoords picks: all must agree
            lmc::CacheGrid g = lmc::BuildCacheGrid(pts, npts, dim, m, chosen ? nullptr : lead);
            for (int i = 0; i < nq; i++) {
                const int e = g.Exists(q + (size_t)i * dim, dim) ? 1 : 0;
                if (!first && e != out[i]) throw std::runtime_error("lmc_cache_filter_probe: the grids disagree");
                out[i] = e;
            }
            first = false;
        }
    return 0;
    LMC_CATCH(-1)
}
// test probe (device/query_probe.hip): the lean small step's cache look-up on caller-given cache rows and chain states, next to the generic CacheQuery.
// The kd-tree is the host build (as lmc_kd_probe's); the existence grid of rank grid_m lies over the leading coordinates or the ones ChooseGridCoords
// picks, and is built by lmc::BuildCacheGrid on the host (converted to the compact layout) or by LaunchBuildCacheGrid on the device.
int lmc_lean_query_probe(int dim, int npts, const float *pts, const float *v1, const float *v2, float malaStepsize, float malaStdDev, int gridM, int chosenCoords,
                         int deviceGrid, int nq, const float *q, const int *queried, const float *lastPss, const float *chV1, const float *chV2, const float *ssScore,
                         int *outInt, float *outW, float *outChain, float *outGauss, float *outGeneric) {
    LMC_TRY
    EnsureDevice(0);
    if (dim < 6 || dim > PSS_MAX_LENGTH || (dim & 1) || npts < 1 || npts > PSS_MAX_SIZE || nq < 1 || gridM < 3 || gridM > 4)
        throw std::runtime_error("lmc_lean_query_probe: bad arguments");
    lmc::KdTreeResult t = lmc::BuildKdTree(pts, npts, dim);
    if (t.depth >= KD_STACK || t.nodes.size() > KD_MAX_NODES) throw std::runtime_error("lmc_lean_query_probe: kd-tree deeper or larger than the search accepts");
    DevBuf<KdNode> dN;
    DevBuf<int> dV;
    DevBuf<float> dP, dV1, dV2;
    const size_t rowWords = (size_t)npts * dim;
    dN.Upload(t.nodes), dV.Upload(t.vind), dP.Upload(pts, rowWords), dV1.Upload(v1, rowWords), dV2.Upload(v2, rowWords);
    std::vector<DCache> cacheHost(1);
    memset(cacheHost.data(), 0, sizeof(DCache));
    DCacheDim &C = cacheHost[0].d[dim];
    C.ready = 1, C.nodes = dN.p, C.vind = dV.p, C.pts = dP.p, C.v1 = dV1.p, C.v2 = dV2.p;
    for (int k = 0; k < dim; k++) C.rootLow[k] = t.rootLow[k], C.rootHigh[k] = t.rootHigh[k];
    // the existence grid
    const int G = CacheGridG(dim), m = std::min(gridM, dim);
    C.gridG = G, C.gridM = m;
    for (int k = 0; k < 4; k++) C.gridCoord[k] = k;
    if (chosenCoords) lmc::ChooseGridCoords(pts, npts, dim, m, C.gridCoord);
    size_t cells = 1, nbrs = 1;
    for (int k = 0; k < m; k++) cells *= G, nbrs *= 3;
    const size_t nWords = (cells + 31) / 32;
    DevBuf<uint2> dWords;
    DevBuf<int> dCellStart, sStart, sCursor, sWordCount, sTiles;
    DevBuf<unsigned short> dIdx;
    if (deviceGrid) {
        dWords.Alloc(nWords), dCellStart.Alloc(std::min(cells, (size_t)npts * nbrs) + 1), dIdx.Alloc((size_t)npts * nbrs);
        sStart.Alloc(cells + 1), sCursor.Alloc(cells), sWordCount.Alloc(nWords), sTiles.Alloc((cells + 1) / 2048 + 2);
        LaunchBuildCacheGrid(dP.p, npts, dim, G, m, C.gridCoord, sStart.p, sCursor.p, sWordCount.p, sTiles.p, dWords.p, dCellStart.p, dIdx.p, 0);
        HIP_CHECK(hipGetLastError());
    } else {
        lmc::CacheGrid g = lmc::BuildCacheGrid(pts, npts, dim, m, C.gridCoord);
        std::vector<uint2> words(nWords, uint2{0u, 0u});
        std::vector<int> cellStart;
        std::vector<unsigned short> idx(g.rowIdx.begin(), g.rowIdx.end());
        for (size_t cell = 0; cell < cells; cell++) {
            if ((cell & 31) == 0) words[cell >> 5].y = (unsigned)cellStart.size();
            if (g.start[cell + 1] > g.start[cell]) words[cell >> 5].x |= 1u << (cell & 31), cellStart.push_back(g.start[cell]);
        }
        cellStart.push_back(g.start[cells]);
        dWords.Upload(words), dCellStart.Upload(cellStart), dIdx.Upload(idx);
    }
    C.gridWords = dWords.p, C.gridCellStart = dCellStart.p, C.gridIdx = dIdx.p;
    DevBuf<DCache> dCache;
    dCache.Upload(cacheHost);
    // the stand-in chain arrays ([word][chain], N = nq) and the queries
    auto soa = [&](const float *rows) {
        std::vector<float> v((size_t)dim * nq);
        for (int i = 0; i < nq; i++)
            for (int k = 0; k < dim; k++) v[(size_t)k * nq + i] = rows[(size_t)i * dim + k];
        return v;
    };
    DevBuf<float> aV1, aV2, aLast, aWeight, dQ, dSs, oW, oGauss, oGeneric;
    DevBuf<int> dQueried, oInt;
    aV1.Upload(soa(chV1)), aV2.Upload(soa(chV2)), aLast.Upload(soa(lastPss)), aWeight.Alloc(nq);
    dQ.Upload(q, (size_t)nq * dim), dSs.Upload(ssScore, nq), dQueried.Upload(queried, nq);
    oInt.Alloc((size_t)nq * LEAN_PROBE_INTS), oW.Alloc((size_t)nq * 5), oGauss.Alloc((size_t)nq * (3 * dim + 1)), oGeneric.Alloc((size_t)nq * 2 * dim);
    ChainArrays A;
    memset(&A, 0, sizeof(A));
    A.N = nq, A.chV1 = aV1.p, A.chV2 = aV2.p, A.chLastPss = aLast.p, A.pathWeight = aWeight.p;
    std::vector<DScene> S(1);
    memset(S.data(), 0, sizeof(DScene));
    S[0].opt.malaStepsize = malaStepsize, S[0].opt.malaStdDev = malaStdDev;
    StepParams P;
    memset(&P, 0, sizeof(P));
    LaunchLeanQueryProbe(S[0], dCache.p, A, P, dim, nq, dQ.p, dQueried.p, dSs.p, LeanQueryProbeOut{oInt.p, oW.p, oGauss.p, oGeneric.p}, 0);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(outInt, oInt.p, oInt.n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(outW, oW.p, oW.n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(outGauss, oGauss.p, oGauss.n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(outGeneric, oGeneric.p, oGeneric.n * sizeof(float), hipMemcpyDeviceToHost));
    const std::vector<float> after[3] = {aV1.Download(), aV2.Download(), aLast.Download()};
    for (int i = 0; i < nq; i++)
        for (int a = 0; a < 3; a++)
            for (int k = 0; k < dim; k++) outChain[((size_t)i * 3 + a) * dim + k] = after[a][(size_t)k * nq + i];
    return 0;
    LMC_CATCH(-1)
}
int lmc_gauss_probe(int n, int dim, const float *v1, const float *M, float ss, float shk, const float *sc, const float *offset, float *out) {
    LMC_TRY
    EnsureDevice(0);
    DevBuf<float> dV, dM, dS, dO, dOut;
    dV.Upload(v1, (size_t)n * dim), dM.Upload(M, (size_t)n * dim), dS.Upload(sc, n), dO.Upload(offset, (size_t)n * dim), dOut.Alloc((size_t)n * (3 * dim + 2));
    LaunchGaussProbe(n, dim, dV.p, dM.p, ss, shk, dS.p, dO.p, dOut.p, 0);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, dOut.p, dOut.n * 4, hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}

// the H2MC step's cooperative launches on caller-supplied states (tests/test_gpu_h2mc.py)
int lmc_h2_hess_probe(int c, int l, int n, const float *primary, const float *scene38, const float *vert, float *loglum, float *grad, float *hess) {
    LMC_TRY
    const int t = H2TechIndex(c, l);
    if (t < 0) throw std::runtime_error("lmc_h2_hess_probe: technique (c,l) out of range");
    if (n < 1 || !primary || !vert) throw std::runtime_error("lmc_h2_hess_probe: n >= 1 states are required");
    const int L = std::max(c + l - 1, 2), V = 238 + 59 * (c + l - 3), dim = 2 * L;
    // lmc_h2_hess_list_probe (list_probes.cpp) with the simplest work list: one bin (the technique's signature 0) holds every state, in identity order
    std::vector<float> prim17((size_t)n * 17, 0.f), vertFull((size_t)n * LMC_PROBE_VERT_WORDS, 0.f);
    for (int i = 0; i < n; i++) {
        memcpy(prim17.data() + (size_t)i * 17, primary + (size_t)i * (2 * L + 1), (2 * L + 1) * sizeof(float));
        memcpy(vertFull.data() + (size_t)i * LMC_PROBE_VERT_WORDS, vert + (size_t)i * V, V * sizeof(float));
    }
    std::vector<int> cs((size_t)n, c), ls((size_t)n, l), items((size_t)n, 0), count(H2_NBINS, 0), start(H2_NBINS, 0);
    for (int i = 0; i < n; i++) items[i] = i;
    count[t * H2_NSIG] = n;
    std::vector<float> o((size_t)n * H2_OUT_WORDS);
    if (lmc_h2_hess_list_probe(n, prim17.data(), cs.data(), ls.data(), vertFull.data(), scene38, n, items.data(), count.data(), start.data(), 1024, o.data()) != 0) return -1;
    for (int i = 0; i < n; i++) {
        const float *r = o.data() + (size_t)i * H2_OUT_WORDS;
        if (loglum) loglum[i] = r[H2_OUT_LOGLUM];
        if (grad) {  // the launch writes dim words
            memset(grad + (size_t)i * 16, 0, 16 * sizeof(float));
            memcpy(grad + (size_t)i * 16, r, dim * sizeof(float));
        }
        if (hess) {
            float *h = hess + (size_t)i * 256;
            memset(h, 0, 256 * sizeof(float));
            for (int a = 0; a < dim; a++)
                for (int b = a; b < dim; b++) h[a * dim + b] = r[H2_OUT_HESS + a * dim + b];
        }
    }
    return 0;
    LMC_CATCH(-1)
}
int lmc_h2_gauss_probe(int n, int dim, const float *grad, const float *hess, float sigma, const float *offset, float *gauss, float *px) {
    LMC_TRY
    if (dim < 4 || dim > 16 || (dim & 1)) throw std::runtime_error("lmc_h2_gauss_probe: dim must be even, 4..16");
    if (n < 1 || !grad || !hess) throw std::runtime_error("lmc_h2_gauss_probe: n >= 1 gradients and Hessians are required");
    const int t = H2TechIndex(dim / 2 + 1, 0);
    // lmc_h2_gauss_list_probe (list_probes.cpp) with the simplest work list: one bin holds every state, in identity order; stage 1, every flag clear
    std::vector<float> hess256((size_t)n * 256, 0.f), off16((size_t)n * 16, 0.f);
    for (int i = 0; i < n; i++) {
        memcpy(hess256.data() + (size_t)i * 256, hess + (size_t)i * dim * dim, (size_t)dim * dim * sizeof(float));
        if (offset) memcpy(off16.data() + (size_t)i * 16, offset + (size_t)i * dim, (size_t)dim * sizeof(float));
    }
    std::vector<int> dims((size_t)n, dim), flags((size_t)n, 0), items((size_t)n, 0), count(H2_NBINS, 0), start(H2_NBINS, 0);
    for (int i = 0; i < n; i++) items[i] = i;
    count[t * H2_NSIG] = n;
    std::vector<float> both(2 * (size_t)n * H2_GAUSS_AOS), pxAll((size_t)n);
    if (lmc_h2_gauss_list_probe(n, dims.data(), grad, hess256.data(), flags.data(), off16.data(), 1, sigma, n, items.data(), count.data(), start.data(), 256, both.data(), pxAll.data()) != 0)
        return -1;
    if (gauss) {  // stage 1 with F_GSEL clear: the second buffer; the words the launch left alone (an isotropic record stores no matrices) read as zero
        const float *g = both.data() + (size_t)n * H2_GAUSS_AOS;
        for (size_t k = 0; k < (size_t)n * H2_GAUSS_AOS; k++) {
            uint32_t bits;
            memcpy(&bits, g + k, 4);
            gauss[k] = bits == 0x7fc0beefu ? 0.0f : g[k];
        }
    }
    if (px) memcpy(px, pxAll.data(), (size_t)n * sizeof(float));
    return 0;
    LMC_CATCH(-1)
}

}  // extern "C"
