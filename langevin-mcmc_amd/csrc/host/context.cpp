// C-ABI implementation (include/lmc_abi.h): scene upload, MLT initialisation, the chain-step loop and the
// global-cache maintenance around the gfx950 kernels.  Host logic only -- every numeric result returned by this
// library is produced by the HIP kernels in device/kernels.hip; there is no CPU fallback.
// The cold parts of the ABI live in units of their own beside this one: checkpoints (ckpt.cpp), the mc and direct-lighting passes (mcrender.cpp),
// the probes and batch calls (probes.cpp, list_probes.cpp), the reference's plugin symbols (plugin_abi.cpp).  context.h is what they see of this unit.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include <rccl/rccl.h>  // declarations only (types, enum values, signatures): librccl is dlopen'ed, never linked

#include "../../../include/lmc_abi.h"
#include "../device/drng.h"
#include "../device/kernels.h"
#include "../device/upload.h"
#include "../device/dh2coop.h"
#include "../device/dh2mc.h"
#include "accel.h"
#include "context.h"
#include "hostutil.h"
#include "scene.h"
#include "shardplan.h"

using namespace lmcd;

static thread_local std::string g_err;

void lmc_host::EnsureDevice(int device) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) throw std::runtime_error("no HIP device available: the MI355X back end has no CPU fallback");
    if (device < 0 || device >= count) throw std::runtime_error("HIP device ordinal out of range");
    HIP_CHECK(hipSetDevice(device));
}

// ------------------------------------------------------------------------------------------------ materials and bitmaps
PackedMaterials lmc_host::PackMaterials(const std::vector<lmc::Material> &materials, const std::vector<lmc::Bitmap> &bitmapList) {
    PackedMaterials pm;
    std::vector<DMaterial> &mats = pm.mats;
    for (const lmc::Material &m : materials) {
        DMaterial d;
        memset(&d, 0, sizeof(d));
        d.type = m.type, d.twoSided = m.twoSided ? 1 : 0;
        auto tex = [](const lmc::TextureRef &t) {
            DTexRef r;
            r.bitmap = t.bitmap, r.sScale = t.sScale, r.tScale = t.tScale;
            memcpy(r.value, t.value, 12);
            return r;
        };
        d.Kd = tex(m.Kd), d.Ks = tex(m.Ks), d.Kt = tex(m.Kt), d.expOrAlpha = tex(m.expOrAlpha);
        d.eta = m.eta, d.invEta = m.invEta, d.KsWeight = m.KsWeight;
        if (m.type != lmc::BSDF_LAMBERTIAN && m.type != lmc::BSDF_PHONG && m.type != lmc::BSDF_ROUGHDIELECTRIC) throw std::runtime_error("unknown BSDF type");
        if (m.type != lmc::BSDF_LAMBERTIAN) pm.glossy = 1;
        for (const DTexRef *r : {&d.Kd, &d.Ks, &d.Kt, &d.expOrAlpha})
            if (r->bitmap >= (int)bitmapList.size()) throw std::runtime_error("a texture names a bitmap the scene does not have");
        mats.push_back(d);
    }
    // every bitmap's texels in ONE buffer (DScene::texPool): a textured DTexRef names its bitmap by the word offset of its texels there and carries
    // width / height / gamma itself (dscene.h LMC_TEX_INLINE), so that a look-up needs no header fetch between the material record and the texels
    std::vector<float> &pool = pm.pool;
    std::vector<size_t> &poolOff = pm.poolOff;
    for (const lmc::Bitmap &bm : bitmapList) {
        poolOff.push_back(pool.size());
        pool.insert(pool.end(), bm.img.data.begin(), bm.img.data.end());
    }
    if (pool.size() >= (size_t)1 << 31) throw std::runtime_error("the scene's bitmaps hold more than 2^31 words");
    if (pool.empty()) pool.push_back(0.f);
#if LMC_TEX_INLINE
    for (DMaterial &d : mats)
        for (DTexRef *r : {&d.Kd, &d.Ks, &d.Kt, &d.expOrAlpha})
            if (r->bitmap >= 0) {
                const lmc::Bitmap &bm = bitmapList[r->bitmap];
                const int W = bm.img.width, H = bm.img.height;
                r->bitmap = (int)poolOff[r->bitmap];
                memcpy(&r->value[0], &W, 4), memcpy(&r->value[1], &H, 4), r->value[2] = bm.gamma;
            }
#endif
    return pm;
}

std::vector<DBitmap> lmc_host::BitmapHeaders(const PackedMaterials &pm, const std::vector<lmc::Bitmap> &bitmapList, const float *devPool) {
    std::vector<DBitmap> bitmaps;
    for (size_t i = 0; i < bitmapList.size(); i++) bitmaps.push_back(DBitmap{devPool + pm.poolOff[i], bitmapList[i].img.width, bitmapList[i].img.height, bitmapList[i].gamma});
    if (bitmaps.empty()) bitmaps.push_back(DBitmap{nullptr, 0, 0, 1.f});
    return bitmaps;
}

// ------------------------------------------------------------------------------------------------ scene upload
static void UploadScene(lmc_ctx *c) {
    const lmc::Scene &sc = *c->scene;
    std::vector<TriData> tris;
    std::vector<DMesh> meshes;
    std::vector<float> areaFunc, areaCdf;
    int triBase = 0;
    for (size_t mi = 0; mi < sc.meshes.size(); mi++) {
        const lmc::Mesh &m = sc.meshes[mi];
        DMesh dm;
        memset(&dm, 0, sizeof(dm));
        dm.material = m.material;
        dm.areaLight = m.areaLight;
        dm.hasST = m.ST.empty() ? 0 : 1;
        dm.triBase = triBase;
        dm.numTris = (int)m.numTris();
        dm.totalArea = m.totalArea;
        dm.invTotalArea = 1.0f / m.totalArea;  // inf when the mesh is no emitter, like inverse(totalArea) in trianglemesh.cpp:186
        dm.areaOff = (int)areaFunc.size();
        dm.areaCdfOff = (int)areaCdf.size();
        dm.areaFuncInt = m.areaFuncInt;
        areaFunc.insert(areaFunc.end(), m.areaFunc.begin(), m.areaFunc.end());
        areaCdf.insert(areaCdf.end(), m.areaCdf.begin(), m.areaCdf.end());
        for (size_t t = 0; t < m.numTris(); t++) {
            TriData T;
            memset(&T, 0, sizeof(T));
            uint32_t i0 = m.idx[3 * t], i1 = m.idx[3 * t + 1], i2 = m.idx[3 * t + 2];
            for (int k = 0; k < 3; k++) {
                T.p0[k] = m.P[i0][k];
                T.e1[k] = m.P[i1][k] - m.P[i0][k];
                T.e2[k] = m.P[i2][k] - m.P[i0][k];
                T.n0[k] = m.N[i0][k], T.n1[k] = m.N[i1][k], T.n2[k] = m.N[i2][k];
            }
            if (dm.hasST) {
                T.st[0] = m.ST[i0].x, T.st[1] = m.ST[i0].y, T.st[2] = m.ST[i1].x, T.st[3] = m.ST[i1].y, T.st[4] = m.ST[i2].x, T.st[5] = m.ST[i2].y;
            }
            T.mesh = (int)mi, T.hasST = dm.hasST, T.material = dm.material, T.areaLight = dm.areaLight;
            tris.push_back(T);
        }
        triBase += dm.numTris;
        meshes.push_back(dm);
    }
    const lmc::Bvh4Result bvh = lmc::CollapseToBvh4(lmc::BuildSceneBvh(tris));
    c->bvhDepth = bvh.stackNeed;  // what the traversal stack must hold (the LDS stack has BVH_LDS_STACK entries)
    for (int &h : c->leafHist) h = 0;
    for (const lmcd::BvhNode4 &nd : bvh.nodes)
        for (int k = 0; k < 4; k++)
            if (nd.child[k] < 0) c->leafHist[(unsigned)~nd.child[k] & 7u]++;  // leaf code: (first << 3) | (count - 1); BVH4_EMPTY is positive
    // the material records and every bitmap's texels in ONE buffer (DScene::texPool): PackMaterials above
    const PackedMaterials pm = PackMaterials(sc.materials, sc.bitmaps);
    const std::vector<DMaterial> &mats = pm.mats;
    const int glossy = pm.glossy;
    c->texPool.Upload(pm.pool);
    c->bitmaps.Upload(BitmapHeaders(pm, sc.bitmaps, c->texPool.p));
    std::vector<DLight> lights;
    for (const lmc::Light &L : sc.lights) {
        DLight d;
        memset(&d, 0, sizeof(d));
        d.type = L.type, d.samplingWeight = L.samplingWeight, d.mesh = L.mesh;
        for (int k = 0; k < 3; k++) d.pos[k] = L.position[k], d.intensity[k] = L.intensity[k], d.radiance[k] = L.radiance[k];
        lights.push_back(d);
    }
    c->nodes.Upload(bvh.nodes), c->leafTris.Upload(bvh.leafTris), c->tris.Upload(tris), c->meshes.Upload(meshes), c->materials.Upload(mats),
        c->lights.Upload(lights);
    c->areaFunc.Upload(areaFunc), c->areaCdf.Upload(areaCdf), c->lightFunc.Upload(sc.lightFunc), c->lightCdf.Upload(sc.lightCdf);
    {   // triangle id -> its position in the tree's leaf order (a space-filling order of the scene): the spatial part of the relocation's fine key (relocate.hip)
        std::vector<int> pos(tris.size(), 0);
        for (size_t q = bvh.leafTris.size(); q-- > 0;) {
            const int id = bvh.leafTris[q].id;
            if (id >= 0 && (size_t)id < pos.size()) pos[id] = (int)q;
        }
        c->leafPosOfTri.Upload(pos);
    }
    DScene &S = c->S;
    memset(&S, 0, sizeof(S));
    // Node format of the scene's hot launches (lean small steps, large steps; dscene.h LdsStackT::kQuant): the 64-byte quantised nodes unless the tree
    // is full of flat leaves away from their node's faces, which the format thickens and every ray leaving such a surface then re-enters
    // (profiles/r05_n_ab_configs_quant.jsonl: torus headline +5 %, full-material torus +10 %, veach-door -7 %; the share separates them: 0.0006 vs 0.55).
    // LMC_BVH_NODES=exact|quant overrides (A/B); a build with -DLMC_BVH_QUANT=1 walks the quantised nodes in every kernel.
    c->thickFlatShare = lmc::ThickenedFlatLeafShare(bvh);
    bool quant = !bvh.qnodes.empty() && c->thickFlatShare < 0.05;
    if (const char *e = getenv("LMC_BVH_NODES")) quant = !bvh.qnodes.empty() && std::string(e) == "quant" ? true : std::string(e) == "exact" ? false : quant;
    if (LMC_BVH_QUANT) {  // a build whose every kernel walks the quantised nodes must not run on a tree the format cannot hold (QuantizeBvh4 left qnodes empty)
        if (bvh.qnodes.empty()) throw std::runtime_error("LMC_BVH_QUANT build: this scene's tree cannot be represented by the quantised nodes");
        quant = true;
    }
    if (quant) c->qnodes.Upload(bvh.qnodes);
    else
        c->qnodes.Free();
    S.nodes = c->nodes.p, S.qnodes = quant ? c->qnodes.p : nullptr, S.leafTris = c->leafTris.p, S.tris = c->tris.p, S.meshes = c->meshes.p, S.materials = c->materials.p, S.bitmaps = c->bitmaps.p, S.texPool = c->texPool.p, S.lights = c->lights.p;
    S.areaFunc = c->areaFunc.p, S.areaCdf = c->areaCdf.p, S.lightFunc = c->lightFunc.p, S.lightCdf = c->lightCdf.p;
    S.lightFuncInt = sc.lightFuncInt, S.lightWeightSum = sc.lightWeightSum;
    S.numTris = (int)tris.size(), S.numNodes = (int)bvh.nodes.size(), S.numMeshes = (int)meshes.size(), S.numLights = (int)lights.size(), S.numMaterials = (int)mats.size();
    S.envLight = sc.envLight;
    S.glossy = glossy;
    if (sc.envLight >= 0) {
        const lmc::Light &L = sc.lights[sc.envLight];
        c->envImage.Upload(L.image.data), c->envCdfRows.Upload(L.sampleInfo.cdfRows), c->envCdfCols.Upload(L.sampleInfo.cdfCols),
            c->envRowWeights.Upload(L.sampleInfo.rowWeights);
        DEnv &E = S.env;
        E.W = L.image.width, E.H = L.image.height;
        E.image = c->envImage.p, E.cdfRows = c->envCdfRows.p, E.cdfCols = c->envCdfCols.p, E.rowWeights = c->envRowWeights.p;
        E.normalization = L.sampleInfo.normalization, E.pixelSize[0] = L.sampleInfo.pixelSize[0], E.pixelSize[1] = L.sampleInfo.pixelSize[1];
        lmc::M4 tw = lmc::ToM4(L.toWorld), tl = lmc::ToM4(L.toLight);
        memcpy(E.toWorld, tw.m, 64), memcpy(E.toLight, tl.m, 64);
        int o = 0;
        for (const lmc::AnimXform *x : {&L.toWorld, &L.toLight}) {
            E.xformBlocks[o++] = x->isMoving;
            for (int k = 0; k < 2; k++)
                for (int i = 0; i < 3; i++) E.xformBlocks[o++] = x->t[k][i];
            for (int k = 0; k < 2; k++)
                for (int i = 0; i < 4; i++) E.xformBlocks[o++] = x->q[k][i];
        }
    }
    const lmc::Camera &cam = sc.camera;
    memcpy(S.cam.sampleToCam, cam.sampleToCam.m, 64), memcpy(S.cam.camToSample, cam.camToSample.m, 64);
    lmc::M4 tw = lmc::ToM4(cam.camToWorld), wc = lmc::ToM4(cam.worldToCamera);
    memcpy(S.cam.toWorld, tw.m, 64), memcpy(S.cam.worldToCamera, wc.m, 64);
    S.cam.width = cam.width, S.cam.height = cam.height, S.cam.nearClip = cam.nearClip, S.cam.farClip = cam.farClip, S.cam.dist = cam.dist;
    for (int k = 0; k < 3; k++) S.bsCenter[k] = sc.bsphereCenter[k];
    S.bsRadius = sc.bsphereRadius;
    lmc::SerializeSceneBlock(sc, S.sceneParams);
    c->film.Alloc((size_t)cam.width * cam.height * 3);
}

static void SyncOptions(lmc_ctx *c) {
    const lmc::DptOptions &o = c->scene->options;
    DOptions &d = c->S.opt;
    d.minDepth = o.minDepth, d.maxDepth = o.maxDepth, d.mala = o.mala ? 1 : 0, d.h2mc = o.h2mc ? 1 : 0;
    d.roughnessThreshold = o.roughnessThreshold, d.largeStepProbability = o.largeStepProbability, d.largeStepProbScale = o.largeStepProbScale;
    d.malaGN = o.malaGN, d.malaStepsize = o.malaStepsize, d.malaStdDev = o.malaStdDev, d.perturbStdDev = o.perturbStdDev;
    d.discreteStdDev = o.discreteStdDev, d.uniformMixingProbability = o.uniformMixingProbability, d.seedOffset = o.seedOffset;
    if (o.maxDepth > MAXD || o.maxDepth < 1)
        throw std::runtime_error(std::string("maxdepth must be in [1, 12] on the MI355X back end") +
                                 (o.integrator == "mc" ? " (integrator=mc too: unbounded paths, maxdepth -1, are not served)" : ""));
    d.useLightCoord = o.useLightCoordinateSampling ? 1 : 0;
    c->S.sceneParams[0] = d.useLightCoord ? 1.0f : 0.0f;  // scene.cpp:165: the flag opens the serialized scene block the path programs read
    d.sampleCache = (o.sampleFromGlobalCache && o.mala) ? 1 : 0;  // mlt.cpp:71-73: LargeStepCache only together with mala
    // a scene lit by its environment map alone has, in practice, no state with a light sub-path: EnvLight::Emit (envlight.cpp:228-248)
    // starts its rays on a disc as wide as the scene's bounding sphere, and with a ground plane in the scene the first ray misses
    // everything the camera sees (torus: the l >= 2 techniques are empty in 4e5 init samples on the oracle and on the device alike,
    // tests/test_host.py).  The lean launch then runs without that half of the walk; a state with l > 1, should one appear, takes the
    // generic launch (LMC_LEAN_LIGHTLESS=0: A/B switch)
    // LMC_LEAN_LIGHTLESS=2 forces it on any scene: every state with l > 1 then takes the fallback, which is how the tests exercise it
    const int lightlessMode = getenv("LMC_LEAN_LIGHTLESS") ? atoi(getenv("LMC_LEAN_LIGHTLESS")) : 1;
    d.leanLightless = (lightlessMode == 2 || (lightlessMode == 1 && c->S.numLights == 1 && c->S.envLight >= 0)) ? 1 : 0;
}

void lmc_host::UploadCacheStruct(lmc_ctx *c, hipStream_t after) {
    if (c->cacheDev.n != 1) c->cacheDev.Alloc(1);
    if (after) {
        // in stream order behind what `after` holds (the step's launches, which read the struct as it was), from a pinned copy: the host goes on
        // queueing.  The copy has run long before the pinned words are written again: that happens behind a later step's countsEvent, which the
        // device reaches after that step's launches, which wait for this stream (StepPhase1's fork).
        *c->cachePinned = c->cacheHost;
        static_assert(sizeof(DCache) % 4 == 0, "the struct goes up word by word");
        lmcd::UploadSegments U;  // as a kernel, not a DMA copy: upload.h
        U.Add(c->cacheDev.p, c->cachePinned, sizeof(DCache));
        LaunchUploadSegments(U, after);
        return;
    }
    HIP_CHECK(hipMemcpy(c->cacheDev.p, &c->cacheHost, sizeof(DCache), hipMemcpyHostToDevice));  // in place: the kernels keep the pointer
}

// ------------------------------------------------------------------------------------------------ ABI
// (`extern "C"` is opened around the ABI functions only; everything internal has C++ linkage: file-local, or in lmc_host where context.h declares it)
void LmcSetLastError(const std::string &what) { g_err = what; }  // last_error.h

extern "C" {

const char *lmc_last_error(void) { return g_err.c_str(); }

lmc_ctx *lmc_create(const lmc_scene_desc *desc) {
    LMC_TRY
    if (!desc || !desc->scene_xml) throw std::runtime_error("lmc_create: null scene description");
    EnsureDevice(desc->device);
    std::unique_ptr<lmc_ctx> c(new lmc_ctx);
    c->device = desc->device;
    c->useGradient = desc->use_gradient;
    c->forceDiffuse = desc->force_diffuse != 0;
    lmc::LoadOverrides ov;
    ov.forceDiffuse = desc->force_diffuse != 0;
    ov.maxDepth = desc->max_depth, ov.width = desc->width, ov.height = desc->height, ov.seedOffset = desc->seed_offset;
    c->scene = lmc::ParseScene(desc->scene_xml, ov);
    HIP_CHECK(hipStreamCreate(&c->stream));
    {
        // the side launches (large steps, cache-filling small steps) are short lists of long-running waves: with a higher
        // queue priority their workgroups are placed before the hot launch's, which would otherwise hold every CU's LDS
        // until it retires (LMC_STREAM_PRIO=0: A/B switch)
        int lo = 0, hi = 0;  // hi = the numerically lowest value = greatest priority
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        const char *e = getenv("LMC_STREAM_PRIO");
        const int mode = e ? atoi(e) : 1;  // 1: side launches first (highest priority), 0: equal, -1: side launches last
        const char *eL = getenv("LMC_STREAM_PRIO_LARGE");  // the large-step stream on its own (H2MC A/B: the small-step pipeline ahead of the large steps)
        const int modeL = eL ? atoi(eL) : mode;
        for (int k = 0; k < 2; k++) {
            const int m = k == 0 ? modeL : mode;
            HIP_CHECK(hipStreamCreateWithPriority(&c->sideStream[k], hipStreamNonBlocking, m > 0 ? hi : m < 0 ? lo : 0));
        }
        for (auto &ps : c->partStream) HIP_CHECK(hipStreamCreateWithPriority(&ps, hipStreamNonBlocking, mode > 0 ? hi : mode < 0 ? lo : 0));
        HIP_CHECK(hipStreamCreateWithPriority(&c->cacheStream, hipStreamNonBlocking, mode > 0 ? hi : mode < 0 ? lo : 0));
        HIP_CHECK(hipHostMalloc((void **)&c->cachePinned, sizeof(DCache), hipHostMallocDefault));
    }
    HIP_CHECK(hipEventCreateWithFlags(&c->partFork, hipEventDisableTiming));
    for (auto &e : c->partJoin) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&c->forkEvent, hipEventDisableTiming));
    for (auto &e : c->joinEvent) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&c->packedEvent, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&c->copiedEvent, hipEventDisableTiming));
    if (const char *e = getenv("LMC_OVERLAP")) c->overlap = atoi(e) != 0;
    if (const char *e = getenv("LMC_OCC_FILTER")) c->useOccFilter = atoi(e) != 0;
    if (const char *e = getenv("LMC_LARGE_LDS")) c->largeLdsStack = atoi(e) != 0;
    if (const char *e = getenv("LMC_LEAN_LDS")) c->leanLdsStack = atoi(e) != 0;
    if (const char *e = getenv("LMC_LARGE_BLOCK")) c->largeBlock = atoi(e) == 64 ? 64 : atoi(e) == 128 ? 128 : 256;
    if (const char *e = getenv("LMC_PROF")) c->profileLean = atoi(e) != 0;
    if (const char *e = getenv("LMC_LEAN_GRAD")) c->leanGrad = atoi(e) != 0;
    if (const char *e = getenv("LMC_MALA_PIPE")) c->malaPipe = atoi(e) != 0;
    if (const char *e = getenv("LMC_EARLY_APPLY")) c->earlyApply = atoi(e) != 0;
    if (const char *e = getenv("LMC_SORT_H2MC")) c->sortH2mc = atoi(e) != 0;
    if (const char *e = getenv("LMC_SORT_GENERIC")) c->sortGeneric = atoi(e) != 0;
    if (const char *e = getenv("LMC_GRID_DIMS")) c->gridDims = std::min(4, std::max(3, atoi(e)));
    if (const char *e = getenv("LMC_FILM_EXACT")) c->filmExact = atoi(e) != 0;  // the default of the "film_exact" option
    if (const char *e = getenv("LMC_EXP_OUTLIER_TEST")) c->expFlags |= atoi(e) ? 128 : 0;  // tests: outlier reset after 6 / 2 adjacent rejections (dchain.h OutlierReset)
    {   // work-skipping measurement switches (dstep_params.h): compiled into -DLMC_EXP_SWITCHES builds only (scripts/build_exp.sh); the shipped library
        // refuses to run while one is set -- a number produced with work skipped must not look like any other
        static const struct {
            const char *name;
            int one, two;
        } sw[] = {{"LMC_EXP_NOSPLAT", 1, 1}, {"LMC_EXP_NOQUERY", 2, 2}, {"LMC_EXP_QUERY_STOP", 256, 512}, {"LMC_EXP_NOGRAD", 4, 4}, {"LMC_EXP_NOSTATS", 8, 8},
                  {"LMC_EXP_NOHESS", 16, 16}, {"LMC_EXP_NOEIGEN", 32, 32}, {"LMC_EXP_NOHESSLAUNCH", 64, 64}, {"LMC_EXP_NOTRAV", 1024, 1024}, {"LMC_EXP_NOSTORE", 2048, 2048}, {"LMC_EXP_NOREUSE", 4096, 4096}};
        for (const auto &w : sw) {
            const char *e = getenv(w.name);
            if (!e || atoi(e) == 0) continue;
#ifdef LMC_EXP_SWITCHES
            c->expFlags |= atoi(e) == 2 ? w.two : w.one;
#else
            throw std::runtime_error(std::string(w.name) + " is set, but this build of liblmc_hip.so has no work-skipping measurement switches (they exist in -DLMC_EXP_SWITCHES builds only: scripts/build_exp.sh, selected with LMC_LIB)");
#endif
        }
    }
    UploadScene(c.get());
    SyncOptions(c.get());
    memset(&c->cacheHost, 0, sizeof(c->cacheHost));
    UploadCacheStruct(c.get());
    return c.release();
    LMC_CATCH(nullptr)
}

void lmc_destroy(lmc_ctx *ctx) {
    if (ctx && ctx->diag) DiagFree(ctx);
    delete ctx;
}

// HIP devices this process can use; 0 without a GPU / driver (never an error: callers use it to refuse a job they cannot place)
int lmc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int lmc_info(lmc_ctx *c, int *out) {
    out[0] = c->S.cam.width, out[1] = c->S.cam.height, out[2] = c->S.numTris, out[3] = c->S.opt.maxDepth, out[4] = c->S.numNodes, out[5] = c->bvhDepth;
    out[6] = c->S.numLights, out[7] = c->S.opt.mala;
    return 0;
}

int lmc_scene_params(lmc_ctx *c, float *out38) {
    memcpy(out38, c->S.sceneParams, 38 * sizeof(float));
    return 0;
}

int lmc_set_option(lmc_ctx *c, const char *name, double v) {
    LMC_TRY
    lmc::DptOptions &o = c->scene->options;
    std::string n(name);
    if (n == "overlap") {  // run-time switch of the concurrent side launches (same results either way; bench.py measures both)
        c->overlap = v != 0;
        return 0;
    }
    if (n == "largestepprob") o.largeStepProbability = (float)v;
    else if (n == "largestepscale") o.largeStepProbScale = (float)v;
    else if (n == "mala") o.mala = v != 0;
    else if (n == "h2mc") o.h2mc = v != 0;
    else if (n == "uniformmixprob") o.uniformMixingProbability = (float)v;
    else if (n == "mala-stepsize") o.malaStepsize = (float)v;
    else if (n == "mala-gn") o.malaGN = (float)v;
    else if (n == "perturbstddev") o.perturbStdDev = (float)v;
    else if (n == "mindepth") o.minDepth = (int)v;
    else if (n == "uselightcoordinatesampling") o.useLightCoordinateSampling = v != 0;
    else if (n == "largestepmultiplexed") o.largeStepMultiplexed = v != 0;
    else if (n == "samplecache") o.sampleFromGlobalCache = v != 0;
    else if (n == "bidirectional") o.bidirectional = v != 0;  // the generator of lmc_mc_render (tests: both on one scene)
    else if (n == "max-derivatives-depth") c->maxDervDepth = (int)v;  // main.cpp:59-60
    else if (n == "timing") c->timing = v != 0;  // record per-step HIP events for lmc_step_timing / lmc_kernel_timing
    else if (n == "exp_resort") c->pendingResort = (int)v;
    else if (n == "resort_every") c->resortEveryOpt = std::max(0, (int)v);  // period of the full re-sort (relocate.hip); takes effect at the next lmc_chains_init; overrides LMC_RESORT_EVERY
    else if (n == "resort_first") c->resortFirstOpt = std::max(0, (int)v);
    else if (n == "mc_film_exact") {  // the mc film's accumulator (device/mc.hip): takes effect at the next lmc_mc_render
        c->mcExactOpt = v != 0;
        return 0;
    } else if (n == "mc_layers") {  // the mc film split by path length (1) or technique (2), host/mcrender.cpp: takes effect at the next lmc_mc_render
        if (v != 0 && v != 1 && v != 2) throw std::runtime_error("mc_layers: 0 (off), 1 (by path length) or 2 (by technique) expected");
        c->mcLayersOpt = (int)v;
        return 0;
    } else if (n == "mc_launch_streams") {  // stream ids per launch of lmc_mc_render / lmc_mc_accumulate
        if (!(v >= 1 && v <= 1e12)) throw std::runtime_error("mc_launch_streams: at least 1 stream id per launch expected");
        c->mcLaunchStreams = (long long)v;
        return 0;
    } else if (n == "film_exact") {  // the film's accumulator (dchain.h Film): takes effect at the next lmc_chains_init / lmc_checkpoint_load
        if ((v != 0) != c->filmExact && c->N > 0)
            throw std::runtime_error(std::string("film_exact: this context's chains are set up with the ") + (c->filmExact ? "fixed-point" : "float") + " film; the mode is chosen before lmc_chains_init / lmc_checkpoint_load");
        c->filmExact = v != 0;
        return 0;
    } else if (n == "film_layers") {  // the MLT film split by path length (1) or technique (2), host/filmlayers.cpp: chosen before lmc_chains_init, like film_exact
        if (v != 0 && v != 1 && v != 2) throw std::runtime_error("film_layers: 0 (off), 1 (by path length) or 2 (by technique) expected");
        if ((int)v != c->filmLayers && c->N > 0)
            throw std::runtime_error("film_layers: this context's chains are set up with film_layers = " + std::to_string(c->filmLayers) + "; the mode is chosen before lmc_chains_init");
        c->filmLayers = (int)v;
        return 0;
    } else if (n == "step_table") {  // the per-technique step table (chaindiag.cpp): counts from the next step on
        DiagSetStepTable(c, v != 0);
        return 0;
    } else if (n == "resident_steps") {  // the resident schedule (RunResident); takes effect at the next lmc_chains_step
        if (o.h2mc && v > 0) throw std::runtime_error("resident_steps: H2MC contexts run in lock step only (their small step is the wave-cooperative pipeline)");
        if (v < 0 || v > 1e6) throw std::runtime_error("resident_steps: K >= 0 expected (0 = lock step)");
        c->residentSteps = (int)v;
    } else if (n == "resident_lanes") {
        if (v != 0 && v != 16 && v != 32 && v != 64) throw std::runtime_error("resident_lanes: 16, 32 or 64 chains per 64-lane wave (0: by the number of chains)");
        c->residentLanes = (int)v;
    } else throw std::runtime_error("Unknown dpt option:" + n);
    SyncOptions(c);
    return 0;
    LMC_CATCH(-1)
}

// <dpt> options as parsed (parsescene.cpp:535-590), by XML name
int lmc_get_option(lmc_ctx *c, const char *name, double *v) {
    LMC_TRY
    const lmc::DptOptions &o = c->scene->options;
    std::string n(name);
    if (n == "spp") *v = o.spp;
    else if (n == "numinitsamples") *v = o.numInitSamples;
    else if (n == "numchains") *v = o.numChains;
    else if (n == "directspp") *v = o.directSpp;
    else if (n == "mindepth") *v = o.minDepth;
    else if (n == "maxdepth") *v = o.maxDepth;
    else if (n == "largestepprob") *v = o.largeStepProbability;
    else if (n == "largestepscale") *v = o.largeStepProbScale;
    else if (n == "mala") *v = o.mala ? 1 : 0;
    else if (n == "h2mc") *v = o.h2mc ? 1 : 0;
    else if (n == "seedoffset") *v = o.seedOffset;
    else if (n == "uselightcoordinatesampling") *v = o.useLightCoordinateSampling ? 1 : 0;
    else if (n == "largestepmultiplexed") *v = o.largeStepMultiplexed ? 1 : 0;
    else if (n == "samplecache") *v = o.sampleFromGlobalCache ? 1 : 0;
    else if (n == "bidirectional") *v = o.bidirectional ? 1 : 0;
    else if (n == "integrator_mc") *v = o.integrator == "mc" ? 1 : 0;  // <string integrator>: "mcmc" (default) or "mc" (lmc_mc_render)
    else if (n == "bvh_quantised") *v = c->S.qnodes ? 1 : 0;            // back-end state, not a <dpt> option: the node format of the scene's hot launches ...
    else if (n == "bvh_thick_flat_share") *v = c->thickFlatShare;       // ... and the figure it was chosen by (UploadScene)
    else if (n == "film_exact") *v = c->filmExact ? 1 : 0;
    else if (n == "film_layers") *v = c->filmLayers;
    else if (n == "mc_film_exact") *v = c->mcExactOpt ? 1 : 0;
    else if (n == "mc_layers") *v = c->mcLayersOpt;
    else if (n == "mc_launch_streams") *v = (double)c->mcLaunchStreams;
    else if (n == "mc_launches") *v = c->mcLaunches;  // launches of the last lmc_mc_render / lmc_mc_accumulate
    else if (n == "step_table") *v = c->diag && DiagStepTableOn(c) ? 1 : 0;
    else if (n == "resident_steps") *v = c->residentSteps;
    else if (n == "resident_lanes") *v = c->residentLanes;
    else if (n == "resident_guard") {  // steps of resident launches that would have needed the gradient program or pushed to the cache (must stay 0)
        HIP_CHECK(hipSetDevice(c->device));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        *v = c->residentGuard.p ? (double)c->residentGuard.Download()[1] : 0.0;
    } else throw std::runtime_error("Unknown dpt option:" + n);
    return 0;
    LMC_CATCH(-1)
}
// film "filename" of the scene (parsescene.cpp: outputName), without extension handling: the caller appends
// "_timeuse_<seconds>s.exr" like mlt.cpp:208
const char *lmc_output_name(lmc_ctx *c) { return c->scene->outputName.c_str(); }

// image files through the library's own readers / writer (host/imageio.cpp): EXR (NONE/ZIPS/ZIP, half or float) and PNG in,
// RGB half ZIP EXR out like the reference's WriteImage.  rgb == NULL: only the size is returned.
int lmc_image_read(const char *path, int *w, int *h, float *rgb) {
    LMC_TRY
    lmc::Image3f img = lmc::ReadImage(path);
    if (w) *w = img.width;
    if (h) *h = img.height;
    if (rgb) memcpy(rgb, img.data.data(), img.data.size() * sizeof(float));
    return 0;
    LMC_CATCH(-1)
}
int lmc_image_write_exr(const char *path, const float *rgb, int w, int h) {
    LMC_TRY
    lmc::WriteEXRHalf(path, rgb, w, h);
    return 0;
    LMC_CATCH(-1)
}

}  // extern "C"

// ---- multi-GPU: the one data-path collective of the LMC path is a sum of the per-GPU films.  RCCL is
// bound at run time (dlopen) so that single-GPU users and the CPU-side tests do not need it.
namespace {
// Signatures, ncclUniqueId and the enum values come from rccl.h at BUILD time (decltype of the declarations: a mismatch with the
// installed header is a compile error, not a silent ABI bug); the library itself is still bound at run time.
struct Rccl {
    void *h = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
static_assert(sizeof(ncclUniqueId) == 128, "lmc_comm_unique_id hands out 128 bytes (include/lmc_abi.h)");
Rccl &GetRccl() {
    static Rccl r;
    static bool ready = false;  // set only after EVERY required symbol has resolved: a failed first call must not leave a half-filled table behind
    if (ready) return r;
    void *h = nullptr;
    // LMC_RCCL_LIB: another library with the six entry points (tests/helpers/rccl_stub.cpp: the collectives over host shared memory, so that a job of several
    // rank PROCESSES can be run on the one GPU of the test tier -- real RCCL refuses two ranks on one device)
    if (const char *e = getenv("LMC_RCCL_LIB")) {
        h = dlopen(e, RTLD_NOW | RTLD_GLOBAL);
        if (!h) throw std::runtime_error(std::string("LMC_RCCL_LIB: ") + dlerror());
    }
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        if (h) break;
        h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    }
    if (!h) throw std::runtime_error(std::string("RCCL not found: ") + dlerror());
    Rccl t;
    t.h = h;
    t.GetUniqueId = (decltype(t.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    t.CommInitRank = (decltype(t.CommInitRank))dlsym(h, "ncclCommInitRank");
    t.AllReduce = (decltype(t.AllReduce))dlsym(h, "ncclAllReduce");
    t.AllGather = (decltype(t.AllGather))dlsym(h, "ncclAllGather");
    t.CommDestroy = (decltype(t.CommDestroy))dlsym(h, "ncclCommDestroy");
    t.GetErrorString = (decltype(t.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!t.GetUniqueId || !t.CommInitRank || !t.AllReduce || !t.AllGather || !t.CommDestroy) throw std::runtime_error("RCCL symbols missing");
    r = t;
    ready = true;
    return r;
}
void RcclCheck(ncclResult_t rc, const char *what) {
    if (rc != ncclSuccess) {
        Rccl &r = GetRccl();
        throw std::runtime_error(std::string("RCCL error in ") + what + ": " + (r.GetErrorString ? r.GetErrorString(rc) : "?"));
    }
}
}  // namespace

int lmc_host::GetRcclDestroy(void *comm) { return GetRccl().CommDestroy ? (int)GetRccl().CommDestroy((ncclComm_t)comm) : 0; }

// ================================================================================================ MLTInit + chain set-up
// MLTInit (mlt.h:41-154), sharded over the ranks of a job BY INIT STREAM (rank r runs the streams [V r / R, V (r + 1) / R): pass 1,
// pass 2 and the checkpoints of those streams stay on r), identical to the one-rank result bit for bit:
//   phase 1  pass 1 on the local streams                        -> exchange: contributions per sample (1 byte each)
//   phase 2  every rank knows every sample's offset; pass 2 on the local samples
//                                                               -> exchange: (c,l) and lsScore of every contribution, in stream order
//   phase 3  every rank runs the SAME sequential float sums and the same equal-spaced CDF walk (mlt.h:107-148) on the host, so
//            normalization and the seeds agree without further communication; a rank's samples seed a contiguous range of chains
//                                                               -> exchange: RNG checkpoints of the seeding samples
//   phase 4  the rank regenerates the init states of ITS chains only and sets its chains up
// What is exchanged is an all-gather of fixed-size blocks (padded to the largest rank's share): RCCL when the context has a
// communicator (lmc_comm_init), device copies between the member contexts of an in-process group (lmc_group_*), nothing at all for a
// single rank.  Init work and the 1.3 KB per chain of init state no longer grow with the number of ranks; what does is 5 bytes per
// init contribution + 25 bytes per chain of the whole job on the host of every rank.
namespace {
struct InitJob {
    // job
    long long numInitSamples = 0, perThread = 0, extra = 0, perChain = 0, chainsNeedExtra = 0;
    int V = 1, numChainsTotal = 0, chainBegin = 0, chainEnd = 0, world = 1, rank = 0;
    // this rank's share: streams [t0, t1), samples [g0, g1)
    int t0 = 0, t1 = 0;
    long long g0 = 0, g1 = 0, maxLocalSamples = 0;
    DevBuf<uint64_t> ckState;
    DevBuf<uint32_t> ckTicks;
    DevBuf<unsigned char> count, gatherCount;
    // phase 2
    std::vector<unsigned long long> hOff;  // first contribution of every sample of the JOB (+ total at the end)
    std::vector<unsigned long long> rankFirst;  // first contribution of every rank's block (+ total)
    unsigned long long total = 0, o0 = 0, o1 = 0, maxLocalContribs = 0;
    DevBuf<unsigned char> outCL, gatherCL;
    DevBuf<float> outLs, gatherLs;
    // phase 3
    std::vector<long long> seedSample;  // per chain of the job
    std::vector<unsigned char> seedCL;
    std::vector<float> seedLs;
    std::vector<int> ownedBegin;  // [world + 1]: rank r's samples seed the chains [ownedBegin[r], ownedBegin[r + 1])
    int maxOwned = 0;
    DevBuf<uint64_t> sendCk, gatherCk;  // per seeded chain: (state, ticks)
};
using lmc::SampleBase;

// recv (on every member) = the members' `bytes` bytes at send, concatenated in rank order
typedef void *(*BufOf)(lmc_ctx *);
void AllGatherBlocks(const std::vector<lmc_ctx *> &g, const std::function<void *(lmc_ctx *)> &send, const std::function<void *(lmc_ctx *)> &recv, size_t bytes) {
    if (bytes == 0) return;
    if (g.size() == 1 && g[0]->world > 1) {  // one rank of an RCCL job
        lmc_ctx *c = g[0];
        HIP_CHECK(hipSetDevice(c->device));
        RcclCheck(GetRccl().AllGather(send(c), recv(c), bytes, ncclUint8, (ncclComm_t)c->comm, c->stream), "ncclAllGather");
        HIP_CHECK(hipStreamSynchronize(c->stream));
        return;
    }
    for (lmc_ctx *c : g) {  // in-process group (or a single rank): everything the members queued must be there before it is copied
        HIP_CHECK(hipSetDevice(c->device));
        HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    for (lmc_ctx *c : g) {
        HIP_CHECK(hipSetDevice(c->device));
        for (size_t q = 0; q < g.size(); q++) HIP_CHECK(hipMemcpyAsync((char *)recv(c) + q * bytes, send(g[q]), bytes, hipMemcpyDefault, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
    }
}

// The per-step exchange of the cache pushes, STREAM-ORDERED: nothing here makes the host wait (the init-time AllGatherBlocks above
// synchronises after every collective because the host reads the result next; in the step loop the consumer is the next kernel on the
// same stream).  RCCL rank: ncclAllGather on the step stream.  In-process group: every member's stream waits for every member's stage
// (packedEvent), copies the stages device to device, and before any member may overwrite its stage again waits for every member's
// copies (copiedEvent) -- a barrier among the streams, not among the host threads: the host runs ahead and queues the next step.
// The three parts of one member's share (every member's part A must be queued before any member's part B, every part B before any part C:
// the sequential driver runs them member by member, the threaded driver of RunSteps puts a barrier of its host threads in between)
void ExchangeStagePartA(lmc_ctx *c) {
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipEventRecord(c->packedEvent, c->stream));
}
void ExchangeStagePartB(lmc_ctx *c, size_t bytes) {
    HIP_CHECK(hipSetDevice(c->device));
    const std::vector<lmc_ctx *> &g = c->group;
    for (size_t q = 0; q < g.size(); q++) {
        if (g[q] != c) HIP_CHECK(hipStreamWaitEvent(c->stream, g[q]->packedEvent, 0));
        HIP_CHECK(hipMemcpyAsync((char *)c->pushGather.p + q * bytes, g[q]->pushStage.p, bytes, hipMemcpyDefault, c->stream));
    }
    HIP_CHECK(hipEventRecord(c->copiedEvent, c->stream));
}
void ExchangeStagePartC(lmc_ctx *c) {
    HIP_CHECK(hipSetDevice(c->device));
    for (lmc_ctx *peer : c->group)
        if (peer != c) HIP_CHECK(hipStreamWaitEvent(c->stream, peer->copiedEvent, 0));
}
bool RcclEarlyExchange() {
    static const bool on = !(getenv("LMC_RCCL_EARLY_EXCHANGE") && atoi(getenv("LMC_RCCL_EARLY_EXCHANGE")) == 0);
    return on;
}
void ExchangeStagesAsync(const std::vector<lmc_ctx *> &g, size_t bytes) {
    if (bytes == 0) return;
    if (g.size() == 1) {
        lmc_ctx *c = g[0];
        if (c->world <= 1) return;
        if (c->appliedEarly) return;  // exchanged and applied behind the pack on the large-step stream (StepPhase1)
        HIP_CHECK(hipSetDevice(c->device));
        RcclCheck(GetRccl().AllGather(c->pushStage.p, c->pushGather.p, bytes, ncclUint8, (ncclComm_t)c->comm, c->stream), "ncclAllGather(cache pushes)");
        return;
    }
    for (lmc_ctx *c : g) ExchangeStagePartA(c);
    for (lmc_ctx *c : g) ExchangeStagePartB(c, bytes);
    for (lmc_ctx *c : g) ExchangeStagePartC(c);
}

// Host threads of an in-process group: one per member, so that the launches of the members' steps are queued side by side instead of one member
// after the other from a single thread (about 15 launches + 8 event operations per member and step).  fn(k) runs for every member; the first
// exception is re-thrown on the caller's thread.  LMC_GROUP_THREADS=0: the members one after the other on the caller's thread (A/B).
bool GroupThreads() {
    static const bool on = !(getenv("LMC_GROUP_THREADS") && atoi(getenv("LMC_GROUP_THREADS")) == 0);
    return on;
}
struct GroupBarrier {
    std::mutex m;
    std::condition_variable cv;
    int n, count = 0, gen = 0;
    bool aborted = false;
    explicit GroupBarrier(int n_) : n(n_) {}
    bool Wait() {  // false: another member failed, give up
        std::unique_lock<std::mutex> lk(m);
        if (aborted) return false;
        const int g = gen;
        if (++count == n) {
            count = 0, gen++;
            cv.notify_all();
            return true;
        }
        cv.wait(lk, [&] { return gen != g || aborted; });
        return !aborted;
    }
    void Abort() {
        std::lock_guard<std::mutex> lk(m);
        aborted = true;
        cv.notify_all();
    }
};
void ForEachMember(size_t n, const std::function<void(size_t)> &fn, GroupBarrier *bar = nullptr) {
    if (n <= 1 || !GroupThreads()) {
        for (size_t k = 0; k < n; k++) fn(k);
        return;
    }
    std::vector<std::exception_ptr> err(n);
    std::vector<std::thread> th;
    for (size_t k = 0; k < n; k++)
        th.emplace_back([&, k] {
            try {
                fn(k);
            } catch (...) {
                err[k] = std::current_exception();
                if (bar) bar->Abort();
            }
        });
    for (auto &t : th) t.join();
    for (auto &e : err)
        if (e) std::rethrow_exception(e);
}

void InitPhase1(lmc_ctx *c, InitJob &J) {
    HIP_CHECK(hipSetDevice(c->device));
    const lmc::ShardLayout lay = lmc::MakeShardLayout(J.world, J.rank, J.V, J.numInitSamples);
    J.t0 = lay.t0, J.t1 = lay.t1, J.g0 = lay.g0, J.g1 = lay.g1, J.maxLocalSamples = lay.maxLocalSamples;
    const size_t nLocal = (size_t)(J.g1 - J.g0), nStreams = (size_t)(J.t1 - J.t0);
    J.ckState.Alloc(std::max<size_t>(nLocal, 1)), J.ckTicks.Alloc(std::max<size_t>(nLocal, 1));
    J.count.Alloc((size_t)J.maxLocalSamples), J.gatherCount.Alloc((size_t)J.maxLocalSamples * J.world, false);
    DevBuf<uint32_t> tab1;
    DevBuf<float> contrib1;
    tab1.Alloc(std::max<size_t>(nStreams, 1) * 64, false), contrib1.Alloc(std::max<size_t>(nStreams, 1) * MAXCONTRIB * CONTRIB_WORDS, false);
    LaunchInitPass1(c->S, J.t0, (int)nStreams, J.perThread, J.extra, J.g0, tab1.p, contrib1.p, J.ckState.p, J.ckTicks.p, J.count.p, c->stream);
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

void InitPhase2(lmc_ctx *c, InitJob &J) {
    HIP_CHECK(hipSetDevice(c->device));
    std::vector<unsigned char> padded = J.gatherCount.Download();
    std::vector<unsigned long long> rankFirst;
    lmc::AssembleCounts(J.world, J.V, J.numInitSamples, padded.data(), J.maxLocalSamples, J.hOff, rankFirst);
    const unsigned long long total = J.hOff[J.numInitSamples];
    J.total = total;
    J.rankFirst = rankFirst;
    if ((long long)total < J.numChainsTotal)
        throw std::runtime_error("MLT initialization failed, consider using a larger number of initial samples or smaller number of chains");
    J.o0 = rankFirst[J.rank], J.o1 = rankFirst[J.rank + 1];
    J.maxLocalContribs = 0;
    for (int r = 0; r < J.world; r++) J.maxLocalContribs = std::max(J.maxLocalContribs, rankFirst[r + 1] - rankFirst[r]);
    // pass 2 on the local samples: (c,l,lsScore) of every contribution, in (stream, sample, contribution) order
    const size_t nLocal = (size_t)(J.g1 - J.g0);
    std::vector<unsigned long long> rel(std::max<size_t>(nLocal, 1), 0);
    for (size_t k = 0; k < nLocal; k++) rel[k] = J.hOff[J.g0 + k] - J.o0;
    DevBuf<unsigned long long> dOff;
    dOff.Upload(rel);
    J.outCL.Alloc((size_t)J.maxLocalContribs), J.outLs.Alloc((size_t)J.maxLocalContribs);
    J.gatherCL.Alloc((size_t)J.maxLocalContribs * J.world, false), J.gatherLs.Alloc((size_t)J.maxLocalContribs * J.world, false);
    const int nSlots = (int)std::min<long long>(std::max<long long>((long long)nLocal, 1), 1 << 18);
    DevBuf<uint32_t> tab2;
    DevBuf<float> contrib2;
    tab2.Alloc((size_t)nSlots * 64, false), contrib2.Alloc((size_t)nSlots * MAXCONTRIB * CONTRIB_WORDS, false);
    LaunchInitPass2(c->S, J.g0, (long long)nLocal, J.perThread, J.extra, nSlots, tab2.p, contrib2.p, J.ckState.p, J.ckTicks.p, dOff.p, J.outCL.p, J.outLs.p, c->stream);
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

void InitPhase3(lmc_ctx *c, InitJob &J) {
    HIP_CHECK(hipSetDevice(c->device));
    const unsigned long long total = J.total;
    // the contributions of the whole job, in stream order
    std::vector<unsigned char> hCL(total);
    std::vector<float> hLs(total);
    {
        std::vector<unsigned char> pCL = J.gatherCL.Download();
        std::vector<float> pLs = J.gatherLs.Download();
        lmc::AssembleBlocks(J.world, J.rankFirst, pCL.data(), J.maxLocalContribs, 1, hCL.data());
        lmc::AssembleBlocks(J.world, J.rankFirst, pLs.data(), J.maxLocalContribs, sizeof(float), hLs.data());
    }
    J.outCL.Free(), J.outLs.Free(), J.gatherCL.Free(), J.gatherLs.Free(), J.gatherCount.Free(), J.count.Free();
    c->numInitContribs = (long long)total;
    // ---- equal-spaced seeding (mlt.h:107-148) on RNG rng(mStates.size()) (mlt.h:115): the same walk on every rank
    std::vector<uint32_t> hostTab(64);
    Rng hr;
    hr.tab = hostTab.data();
    hr.state = PcgSeed((uint64_t)total, hr.tab);
    hr.ticks = 0;
    const int NT = J.numChainsTotal;
    lmc::SeedWalk(J.numInitSamples, NT, J.hOff, hCL.data(), hLs.data(), [](void *r) { return ((Rng *)r)->Uniform(); }, &hr, J.seedSample, J.seedCL, J.seedLs, c->normalization);
    {  // lengthDist, mlt.h:88-99: per-length score sums in stream order (float, like the reference's accumulation), the same on every rank
        std::vector<float> lengthContrib;
        for (unsigned long long k = 0; k < total; k++) {
            const int pathLength = (hCL[k] >> 4) + (hCL[k] & 15) - 1;
            if (pathLength >= (int)lengthContrib.size()) lengthContrib.resize(pathLength + 1, 0.f);
            lengthContrib[pathLength] += hLs[k];
        }
        if ((int)lengthContrib.size() > LENGTH_DIST_MAX) throw std::runtime_error("path length beyond LENGTH_DIST_MAX");
        lmc::BuildPiecewise1D(lengthContrib.data(), (int)lengthContrib.size(), c->lengthFunc, c->lengthCdf, c->lengthFuncInt);
    }
    c->initCL.swap(hCL), c->initLs.swap(hLs);
    c->initOffsets.assign(J.hOff.begin(), J.hOff.end() - 1);
    J.ownedBegin = lmc::OwnedRanges(J.world, J.V, J.numInitSamples, J.seedSample);
    J.maxOwned = 0;
    for (int r = 0; r < J.world; r++) J.maxOwned = std::max(J.maxOwned, J.ownedBegin[r + 1] - J.ownedBegin[r]);
    // the checkpoints of the samples of MINE that seed chains, in chain order
    const int a = J.ownedBegin[J.rank], b = J.ownedBegin[J.rank + 1];
    std::vector<uint64_t> hState = J.ckState.Download();
    std::vector<uint32_t> hTicks = J.ckTicks.Download();
    std::vector<uint64_t> send((size_t)std::max(J.maxOwned, 1) * 2, 0);
    for (int i = a; i < b; i++) {
        const long long k = J.seedSample[i] - J.g0;
        send[(size_t)(i - a) * 2] = hState[k], send[(size_t)(i - a) * 2 + 1] = hTicks[k];
    }
    J.sendCk.Upload(send);
    J.gatherCk.Alloc((size_t)std::max(J.maxOwned, 1) * 2 * J.world, false);
    J.ckState.Free(), J.ckTicks.Free();
}

void InitPhase4(lmc_ctx *c, InitJob &J);
}  // namespace

// what the resident chain state is laid out for: mala, h2mc, samplecache (chain.path copies, cache rows with paths)
static int MutationKey(const lmc_ctx *c) {
    const lmc::DptOptions &o = c->scene->options;
    // uselightcoordinatesampling: which launch runs a chain's small steps is decided when its step is queued and the launch plan is fixed when
    // the caches become ready -- switching it under resident chains would leave them on a list no launch serves
    return (o.mala ? 1 : 0) | (o.h2mc ? 2 : 0) | ((o.sampleFromGlobalCache && o.mala) ? 4 : 0) | (o.useLightCoordinateSampling ? 8 : 0);
}
static void WarmStepLaunches(lmc_ctx *c);
namespace {
void InitPhase4(lmc_ctx *c, InitJob &J) {
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int chainBegin = J.chainBegin;
    const size_t N = (size_t)(J.chainEnd - J.chainBegin);
    // ---- the init states of this rank's chains, regenerated from the checkpoints of their seeding samples (wherever those ran)
    {
        std::vector<uint64_t> all = J.gatherCk.Download();
        std::vector<long long> seedSample(N);
        std::vector<unsigned char> seedCL(N);
        std::vector<uint64_t> ckS(N);
        std::vector<uint32_t> ckT(N);
        int owner = 0;
        for (size_t k = 0; k < N; k++) {
            const int i = chainBegin + (int)k;
            while (i >= J.ownedBegin[owner + 1]) owner++;
            const size_t at = ((size_t)owner * std::max(J.maxOwned, 1) + (size_t)(i - J.ownedBegin[owner])) * 2;
            seedSample[k] = J.seedSample[i], seedCL[k] = J.seedCL[i], ckS[k] = all[at], ckT[k] = (uint32_t)all[at + 1];
        }
        DevBuf<long long> dSeedSample;
        DevBuf<unsigned char> dSeedCL;
        DevBuf<uint64_t> dCkS;
        DevBuf<uint32_t> dCkT, tab3;
        DevBuf<float> contrib3;
        dSeedSample.Upload(seedSample), dSeedCL.Upload(seedCL), dCkS.Upload(ckS), dCkT.Upload(ckT);
        tab3.Alloc(N * 64, false), contrib3.Alloc(N * MAXCONTRIB * CONTRIB_WORDS, false);
        c->initPath.Alloc(N * DPATH_WORDS), c->initContrib.Alloc(N * CONTRIB_WORDS), c->initScoreSum.Alloc(N);
        LaunchInitRegen(c->S, (int)N, J.perThread, J.extra, dSeedSample.p, dSeedCL.p, tab3.p, contrib3.p, dCkS.p, dCkT.p, c->initPath.p, c->initContrib.p,
                        c->initScoreSum.p, s);
        HIP_CHECK(hipStreamSynchronize(s));
    }
    J.sendCk.Free(), J.gatherCk.Free();
    ChainSetUp U;
    U.numChainsTotal = J.numChainsTotal, U.chainBegin = J.chainBegin, U.chainEnd = J.chainEnd, U.perChain = J.perChain, U.chainsNeedExtra = J.chainsNeedExtra;
    U.seedLs = &J.seedLs, U.seedCL = &J.seedCL;
    SetUpChains(c, U);
}
}  // namespace
// the chain arrays and everything the step loop needs beside them, allocated and in the state of a fresh population: identity layout (slot = chain),
// empty caches, zeroed film and counters, every chain queued for a large step.  After a checkpoint's records are in, lmc_checkpoint_load rebuilds the lists.
void lmc_host::SetUpChains(lmc_ctx *c, const ChainSetUp &U) {
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int numChainsTotal = U.numChainsTotal, chainBegin = U.chainBegin, chainEnd = U.chainEnd;
    const long long perChain = U.perChain, chainsNeedExtra = U.chainsNeedExtra;
    c->numChainsTotal = numChainsTotal;
    c->chainBegin = chainBegin;
    c->N = chainEnd - chainBegin;
    c->mutationAtInit = MutationKey(c);
    if (c->diag) DiagChainsReset(c);
    c->perChain = perChain, c->chainsNeedExtra = chainsNeedExtra, c->stepsDone = 0, c->secondsBefore = 0;
    const size_t N = c->N;
    if (U.fromCheckpoint) c->initPath.Alloc(N * DPATH_WORDS), c->initContrib.Alloc(N * CONTRIB_WORDS), c->initScoreSum.Alloc(N);
    c->initLsAll.Upload(*U.seedLs), c->initCLAll.Upload(*U.seedCL);
    // ---- chain arrays
    c->rngState.Alloc(N), c->rngTab.Alloc(N * 64, false), c->rngTicked.Alloc(N);
    c->curPath.Alloc(N * DPATH_WORDS), c->pathBuf1.Alloc(N * DPATH_WORDS), c->curContrib.Alloc(N * CONTRIB_WORDS), c->scoreSum.Alloc(N), c->gaussian.Alloc(N * GAUSS_WORDS), c->gaussian1.Alloc(N * GAUSS_WORDS);
    c->curSplat.Alloc(N * MAXCONTRIB * SPLAT_WORDS), c->curSplatCount.Alloc(N);
    c->chV1.Alloc(N * MAXPSS), c->chV2.Alloc(N * MAXPSS), c->chCurrNewV2.Alloc(N * MAXPSS), c->chPropNewV1.Alloc(N * MAXPSS),
        c->chPropNewV2.Alloc(N * MAXPSS), c->chPss.Alloc(N * MAXPSS), c->chLastPss.Alloc(N * MAXPSS);
    const bool sampleCache = c->S.opt.sampleCache != 0;
    if (sampleCache) c->chPath.Alloc(N * DPATH_WORDS), c->chContrib.Alloc(N * CONTRIB_WORDS);
    else
        c->chPath.Free(), c->chContrib.Free();
    c->pathWeight.Alloc(N), c->lastScoreSum.Alloc(N), c->lastScore.Alloc(N), c->contribList.Alloc(N * MAXCONTRIB * CONTRIB_WORDS, false);
    c->pushData.Alloc(N * GAUSS_WORDS), c->flags.Alloc(N), c->nextKind.Alloc(N + 4), c->adjacentReject.Alloc(N), c->sampleIdx.Alloc(N), c->numSamples.Alloc(N), c->pushDim.Alloc(N);
    c->counters.Alloc(8), c->weightSum.Alloc(1), c->prof.Alloc(16);
    ChainArrays &A = c->A;
    A.N = (int)N;
    A.rngState = c->rngState.p, A.rngTab = c->rngTab.p, A.rngTicked = c->rngTicked.p, A.curPath = c->curPath.p, A.pathBuf1 = c->pathBuf1.p, A.curContrib = c->curContrib.p, A.scoreSum = c->scoreSum.p;
    A.flags = c->flags.p, A.gaussian = c->gaussian.p, A.gaussian1 = c->gaussian1.p, A.curSplat = c->curSplat.p, A.curSplatCount = c->curSplatCount.p;
    A.chV1 = c->chV1.p, A.chV2 = c->chV2.p, A.chCurrNewV2 = c->chCurrNewV2.p, A.chPropNewV1 = c->chPropNewV1.p, A.chPropNewV2 = c->chPropNewV2.p,
    A.chPss = c->chPss.p, A.chLastPss = c->chLastPss.p;
    A.chPath = sampleCache ? c->chPath.p : nullptr, A.chContrib = sampleCache ? c->chContrib.p : nullptr;
    A.pathWeight = c->pathWeight.p, A.lastScoreSum = c->lastScoreSum.p, A.lastScore = c->lastScore.p;
    A.adjacentReject = c->adjacentReject.p, A.sampleIdx = c->sampleIdx.p, A.numSamples = c->numSamples.p;
    A.contribList = c->contribList.p, A.nextKind = c->nextKind.p, A.pushDim = c->pushDim.p, A.pushData = c->pushData.p;
    A.initPath = c->initPath.p, A.initContrib = c->initContrib.p, A.initScoreSum = c->initScoreSum.p, A.initLsAll = c->initLsAll.p, A.initCLAll = c->initCLAll.p;
    A.counters = c->counters.p, A.weightSum = c->weightSum.p, A.prof = c->prof.p;
    // Relocation: off for `samplecache` (chain.path is not moved); H2MC renders move only chains without a stored Gaussian (relocate.hip)
    c->relocate = true;
    if (const char *e = getenv("LMC_RELOCATE")) c->relocate = atoi(e) != 0;
    if (sampleCache) c->relocate = false;
    c->relocations = 0;
    if (c->relocate) {
        c->chainId.Alloc(N, false), c->slotOf.Alloc(N, false), c->relocTileCount.Alloc(RelocTiles((int)N) + 1, false), c->relocTileHist.Alloc(RelocTiles((int)N) * 64, false), c->relocMembers.Alloc(N, false);
        c->relocSorted.Alloc(N, false), c->relocCount.Alloc(2), c->relocPlacedKey.Alloc(N, false), c->stepKind.Alloc(N + 4, false);
        c->relocStaging.Alloc(N * RelocRecordWords(c->S.opt.maxDepth), false);  // the first step is a large step of every chain: N records, cut to N / 2 after it (StepPhase1)
        HIP_CHECK(hipMemsetAsync(c->relocPlacedKey.p, 0xff, N * sizeof(unsigned), s));
        HIP_CHECK(hipMemsetAsync(c->stepKind.p, NEXT_LARGE, N, s));  // k_init_lists: every chain starts with a large step
        LaunchRelocIota((int)N, c->chainId.p, s), LaunchRelocIota((int)N, c->slotOf.p, s);
        // default: every 32nd step (profiles/r06_l_*, r06_m_*: headline steady state +3 % at 32 and at 16, -2 % at 8 -- the lean kernel alone gains 6 / 10 / 11 %,
        // a re-sort costs 1.3 ms at 2^20 chains, 1.7 ms while the fill phase's MALA vectors are alive); LMC_RESORT_EVERY=0 switches it off (A/B)
        c->resortEvery = 32;
        if (const char *e = getenv("LMC_RESORT_EVERY")) c->resortEvery = std::max(0, atoi(e));
        if (c->resortEveryOpt >= 0) c->resortEvery = c->resortEveryOpt;
        // the first one after step resortFirst, then every resortEvery steps.  Every chain's first step is a large step, and so are most of the next few
        // (2^20 chains: 1.05 M, 845 k, 682 k, 553 k, 451 k, 369 k ... large steps in steps 0, 1, 2 ...): an order made before that storm has died down is
        // gone within a step or two.  After it, while a chain's large-step probability is still the unscaled 0.05 (mlt.cpp:96-97: the first 10 % of
        // its samples), an order lasts long: the lean launch of the steps behind a sort ran 1.46 ms instead of 1.71 for the next six steps of the fill
        // phase (profiles/r06_l_step_durations_fill_phase_resort16.txt).  LMC_RESORT_FIRST overrides (A/B).
        c->resortFirst = 4;
        if (const char *e = getenv("LMC_RESORT_FIRST")) c->resortFirst = std::max(0, atoi(e));
        if (c->resortFirstOpt >= 0) c->resortFirst = c->resortFirstOpt;
        if (c->S.opt.h2mc) c->resortEvery = 0;  // the dense Gaussians of an H2MC render live in per-slot buffers that do not move (relocate.hip MemberKey)
        c->stepsSinceInit = 0, c->resorts = 0;
        // per-step relocation by the fine key: measured and not taken -- the lean launch gains 2.5 % (1.12 against 1.15 ms alone), but the radix sort of the step's
        // movers is fifteen more launches on the large-step stream, which then outlasts the hot launch: 2.19 against 1.69 ms per step (profiles/r06_r_*)
        c->relocFine = false;
        if (const char *e = getenv("LMC_RELOC_FINE")) c->relocFine = atoi(e) != 0;
        if (c->resortEvery > 0 || c->relocFine) {
            const size_t nb = RelocSortBlocks((int)N);
            for (int k = 0; k < 2; k++) c->sortKeys[k].Alloc(N, false), c->sortVals[k].Alloc(N, false);
            c->sortHist.Alloc(256 * nb, false), c->sortScanSums.Alloc(256 * nb / 2048 + 2, false);
            c->RS = RelocSortBuffers{{c->sortKeys[0].p, c->sortKeys[1].p}, {c->sortVals[0].p, c->sortVals[1].p}, c->sortHist.p, c->sortScanSums.p};
        }
        c->RB = RelocBuffers{c->relocPlacedKey.p, c->relocTileCount.p, c->relocTileHist.p, c->relocMembers.p, c->relocSorted.p, c->relocCount.p, c->relocStaging.p, (int)N, c->relocFine};
        A.chainId = c->chainId.p, A.slotOf = c->slotOf.p, A.stepKind = c->stepKind.p;
    } else {
        A.chainId = nullptr, A.slotOf = nullptr, A.stepKind = nullptr;
        for (auto *b : {&c->chainId, &c->slotOf, &c->relocTileCount, &c->relocTileHist, &c->relocMembers, &c->relocSorted, &c->relocCount}) b->Free();
        c->relocPlacedKey.Free(), c->stepKind.Free(), c->relocStaging.Free();
    }
    if (!U.fromCheckpoint) {
        LaunchSeedRng((int)N, (long long)chainBegin + c->S.opt.seedOffset, c->rngState.p, c->rngTab.p, s);  // RNG rng(chainId + seedOffset), mlt.cpp:61-62
        LaunchSetupChains(A, chainBegin, perChain, chainsNeedExtra, s);
    }
    // step launch geometry of the large-step and generic launches: one thread per chain up to a persistent cap; gradient work buffer per launched thread
    // (the lean launch has no cap: one chain per thread, grid sized by its launch function)
    c->stepGrid = (int)std::min<size_t>((N + 255) / 256, 4096);
    c->gradStride = c->stepGrid * 256;
    if (const char *e = getenv("LMC_LEAN_BLOCK")) c->leanBlock = std::max(64, std::min(256, atoi(e) / 64 * 64));
    // Technique sort of the lean launch's work list.  On a Lambertian-only scene the lean kernel waits for its streamed chain state and scattered
    // lanes cost more than divergence saves (sorted: -10 %, r02 / r03 A/Bs); the glossy instantiations run with 15-17 % of their lanes active and the
    // vector ALU issuing a third of the time (profiles/r04_p_*): there grouping the WHOLE list by technique pays (full-material torus at maxdepth 12:
    // 144 -> 153 M inside 1024-chain tiles -> 163 M over the whole list; veach-door 139 -> 144 M either way; profiles/r04_u_ab_sort_glossy.jsonl).
    // LMC_SORT_PLAIN overrides: 0 | 1 (1024-chain tiles) | 2 (256-chain tiles) | 3 (two classes) | 4 (whole list)
    c->sortPlain = c->S.glossy ? 4 : 0;
    if (const char *e = getenv("LMC_SORT_PLAIN")) c->sortPlain = atoi(e);
    c->gradBuf.Alloc(c->useGradient ? (size_t)c->gradStride * 640 : 1, false);  // V <= 238 + 59*6 = 592 words for c+l <= 9
    // global cache: dims 2L for L in [3, maxDepth], capped by PSS_MAX_LENGTH
    size_t maxGridCells = 0;
    for (int d = 0; d <= PSS_MAX_LENGTH; d++) {
        CacheDimHost &cd = c->cacheDims[d];
        cd.ready = false;
        cd.relevant = (d % 2 == 0) && d >= 2 * std::max(c->S.opt.minDepth, 3) && d <= 2 * c->S.opt.maxDepth;
        if (cd.relevant) {
            cd.pss.Alloc((size_t)PSS_MAX_SIZE * d), cd.v1.Alloc((size_t)PSS_MAX_SIZE * d), cd.v2.Alloc((size_t)PSS_MAX_SIZE * d);
            cd.weight.Alloc(PSS_MAX_SIZE);
            if (sampleCache) cd.extra.Alloc((size_t)PSS_MAX_SIZE * CACHE_ROW_EXTRA), cd.distCdf.Alloc(PSS_MAX_SIZE + 1);
            // everything the "cache became ready" event needs is allocated here: hipMalloc inside the step loop costs more than
            // the kd-tree build it would sit next to
            cd.gridG = CacheGridG(d), cd.gridM = std::min(c->gridDims, d);
            size_t cells = 1, nbrs = 1;
            for (int k = 0; k < cd.gridM; k++) cells *= cd.gridG, nbrs *= 3;
            cd.gridWords.Alloc((cells + 31) / 32, false), cd.gridCellStart.Alloc(std::min(cells, (size_t)PSS_MAX_SIZE * nbrs) + 1, false), cd.gridIdx.Alloc((size_t)PSS_MAX_SIZE * nbrs, false);
            maxGridCells = std::max(maxGridCells, cells);
            cd.nodes.Alloc(KD_MAX_NODES, false), cd.vind.Alloc(PSS_MAX_SIZE, false);
            // ... the pinned buffers of the rows' way down and the tree's way up included (hipHostMalloc: 0.1 ms each)
            const int sl = (d - 6) / 2;
            if (sl >= 0 && sl < CACHE_SLOTS && d == 6 + 2 * sl) {
                if (!c->rowsPinned[sl]) HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&c->rowsPinned[sl]), (size_t)PSS_MAX_SIZE * PSS_MAX_LENGTH * sizeof(float)));
                if (!c->treePinned[sl]) HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&c->treePinned[sl]), (size_t)KD_MAX_NODES * sizeof(KdNode) + (size_t)PSS_MAX_SIZE * sizeof(int)));
            }
        }
    }
    if (maxGridCells) {
        c->gridScratchStart.Alloc(maxGridCells + 1, false), c->gridScratchCursor.Alloc(maxGridCells, false), c->gridScratchWordCount.Alloc((maxGridCells + 31) / 32, false);
        c->gridTileSums.Alloc((maxGridCells + 1) / 2048 + 2, false);
    }
    c->cacheCounts.Alloc(CACHE_SLOTS), c->pushTiles.Alloc((N + 1023) / 1024);
    if (!c->hostCounts) HIP_CHECK(hipHostMalloc((void **)&c->hostCounts, CACHE_SLOTS * sizeof(int)));
    if (!c->countsEvent) HIP_CHECK(hipEventCreateWithFlags(&c->countsEvent, hipEventDisableTiming));
    if (!c->treesUpEvent) HIP_CHECK(hipEventCreateWithFlags(&c->treesUpEvent, hipEventDisableTiming));
    c->stageLayout = MakePushStageLayout(sampleCache);
    c->pushStage.Alloc((size_t)c->stageLayout.totalFloats), c->pushGather.Alloc(c->world > 1 ? (size_t)c->stageLayout.totalFloats * c->world : 1);
    memset(&c->stageT, 0, sizeof(c->stageT));
    c->stageT.count = reinterpret_cast<int *>(c->pushStage.p);
    for (int sl = 0; sl < CACHE_SLOTS; sl++)
        if (c->cacheDims[6 + 2 * sl].relevant)
            c->stageT.pss[sl] = c->pushStage.p + c->stageLayout.pss[sl], c->stageT.v1[sl] = c->pushStage.p + c->stageLayout.v1[sl],
            c->stageT.v2[sl] = c->pushStage.p + c->stageLayout.v2[sl], c->stageT.weight[sl] = c->pushStage.p + c->stageLayout.weight[sl],
            c->stageT.extra[sl] = sampleCache ? c->pushStage.p + c->stageLayout.extra[sl] : nullptr;
    memset(&c->pushT, 0, sizeof(c->pushT));
    c->pushT.count = c->cacheCounts.p;
    for (int sl = 0; sl < CACHE_SLOTS; sl++) {
        CacheDimHost &cd = c->cacheDims[6 + 2 * sl];
        if (cd.relevant)
            c->pushT.pss[sl] = cd.pss.p, c->pushT.v1[sl] = cd.v1.p, c->pushT.v2[sl] = cd.v2.p, c->pushT.weight[sl] = cd.weight.p, c->pushT.extra[sl] = sampleCache ? cd.extra.p : nullptr;
    }
    memset(&c->cacheHost, 0, sizeof(c->cacheHost));
    UploadCacheStruct(c);
    c->allCachesReady = false;
    c->residentGuard.Alloc(4);  // zero-filled
    c->residentLaunches = 0, c->lockSteps = 0, c->residentMs = 0, c->residentResortPending = false;
    for (auto &e : c->residentEvents) (void)hipEventDestroy(e.first), (void)hipEventDestroy(e.second);
    c->residentEvents.clear();
    c->stepsSinceCounts = 0;
    for (int sl = 0; sl < CACHE_SLOTS; sl++) c->lastCounts[sl] = 0, c->lastDelta[sl] = 0, c->rowsPrefetched[sl] = false;
    c->needGeneric = true;
    c->genericTokenOnly = false;
    c->anyDeepCache = false;
    if (!c->S.opt.mala && !c->S.opt.h2mc) {  // plain MLT never pushes to the cache (mlt.cpp:120-127 sits behind the MALA step): nothing to pack, exchange or read back
        c->allCachesReady = true;
        c->needGeneric = c->S.opt.useLightCoord || c->S.opt.leanLightless;
        c->genericTokenOnly = c->S.opt.leanLightless && !c->S.opt.useLightCoord;
    }
    if (c->S.opt.h2mc) {  // no gradient cache on the H2MC path: nothing to maintain, every small step takes the "generic" launch
        c->allCachesReady = true;
        c->h2Rec.Alloc(N * (size_t)H2_REC_WORDS, false), c->h2Out.Alloc(N * (size_t)H2_OUT_WORDS), c->h2Gauss.Alloc(2 * N * (size_t)H2_GAUSS_AOS, false);
        c->h2Offset.Alloc(N * (size_t)MAXPSS), c->h2Py.Alloc(N), c->h2Px.Alloc(N), c->h2PropContrib.Alloc(N * (size_t)CONTRIB_WORDS), c->h2Step.Alloc(N), c->h2Kind.Alloc(N);
        // Two halves of the chain population run the pipeline side by side, each on its own stream (LaunchGeneric; LMC_H2_PARTS=1: one pipeline).
        // Per (part, stage): a bin table (count | start | cursor) and the part's share of the stage's N-entry item array; binOf is per stage
        // (the parts' chains are disjoint).  The generic list is cut into the parts' sub-lists every step (kernels.hip k_split_list).
        constexpr int MP = lmc_ctx::H2_MAX_PARTS;
        c->h2Parts = 2;
        if (const char *e = getenv("LMC_H2_PARTS")) c->h2Parts = std::max(1, std::min(MP, atoi(e)));
        c->h2PartStride = (int)(((N + 127) / 128) * 64 + 64);  // the most entries the interleaved split gives one of two (or more) parts
        c->h2Items.Alloc((size_t)MP * 2 * N, false), c->h2BinOf.Alloc(2 * N, false), c->h2Counts.Alloc((size_t)MP * 2 * 3 * H2_COUNT_WORDS);
        c->h2SubList.Alloc(MP * (size_t)c->h2PartStride, false), c->h2SubCount.Alloc(MP);
        c->h2SplitOf = nullptr;  // the lists were re-allocated; an address that happens to repeat must not pass for "already cut"
        H2Arrays &H = c->H2;
        H.rec = c->h2Rec.p, H.hout = c->h2Out.p, H.gauss = c->h2Gauss.p, H.offset = c->h2Offset.p, H.py = c->h2Py.p, H.px = c->h2Px.p, H.propContrib = c->h2PropContrib.p;
        H.step = c->h2Step.p, H.kind = c->h2Kind.p;
        for (int part = 0; part < MP; part++)
            for (int st = 0; st < 2; st++) {
                int *tab = c->h2Counts.p + (size_t)(part * 2 + st) * 3 * H2_COUNT_WORDS;
                int *items = c->h2Items.p + (size_t)(part * 2 + st) * N;  // N entries each: a part may be the whole population (LMC_H2_PARTS=1, or the side streams switched off)
                c->h2Bins[part][st] = H2Bins{items, tab, tab + H2_COUNT_WORDS, tab + 2 * H2_COUNT_WORDS, c->h2BinOf.p + (size_t)st * N};
            }
        for (int st = 0; st < 2; st++) H.bins[st] = c->h2Bins[0][st];
        // the Hessian launch is persistent: one wave per SIMD (its waves take the whole register file), grid-stride over the tasks
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, c->device));
        c->h2HessGrid = prop.multiProcessorCount * 4;
        if (const char *e = getenv("LMC_H2_HESS_GRID")) c->h2HessGrid = std::max(1, atoi(e));
        c->h2GaussGrid = prop.multiProcessorCount * 16;
    }
    if (c->S.opt.mala && !c->S.opt.h2mc && c->useGradient && c->malaPipe && !c->S.opt.sampleCache) {
        c->h2Rec.Alloc(N * (size_t)H2_REC_WORDS, false), c->h2Out.Alloc(N * (size_t)MG_OUT_WORDS);
        c->h2Offset.Alloc(N * (size_t)MAXPSS), c->h2Py.Alloc(N), c->h2PropContrib.Alloc(N * (size_t)CONTRIB_WORDS), c->h2Step.Alloc(N);
        c->h2Items.Alloc(2 * N, false), c->h2BinOf.Alloc(2 * N, false), c->h2Counts.Alloc(2 * 3 * H2_COUNT_WORDS);
        MalaPipe &M = c->MP;
        M.rec = c->h2Rec.p, M.gout = c->h2Out.p, M.offset = c->h2Offset.p, M.py = c->h2Py.p, M.propContrib = c->h2PropContrib.p, M.step = c->h2Step.p;
        for (int st = 0; st < 2; st++) M.bins[st] = H2Bins{c->h2Items.p + (size_t)st * N, c->h2Counts.p + H2_COUNT_WORDS * st, c->h2Counts.p + H2_COUNT_WORDS * (2 + st), c->h2Counts.p + H2_COUNT_WORDS * (4 + st), c->h2BinOf.p + (size_t)st * N};
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, c->device));
        c->h2HessGrid = prop.multiProcessorCount * 4;  // persistent, grid-stride over the tasks
        if (const char *e = getenv("LMC_MALA_GRAD_GRID")) c->h2HessGrid = std::max(1, atoi(e));
    } else {
        c->MP = MalaPipe{};
    }
    for (int b = 0; b < 2; b++) {
        for (int k = 0; k < 3; k++) c->lists[b][k].Alloc(N, false);
        c->listCounts[b].Alloc(4);
    }
    c->listScratch.Alloc(N, false), c->sortBins.Alloc(((size_t)N / 2048 + 2) * 64);
    if (c->sortPlain == 4) c->listScratch2.Alloc(N, false), c->sortBins2.Alloc(((size_t)N / 2048 + 2) * 64);
    c->parity = 0;
    // every chain begins with a forced large step (mlt.h:121: the resampled init states only feed the outlier reset)
    LaunchInitLists((int)N, c->lists[0][0].p, c->listCounts[0].p, s);
    HIP_CHECK(hipMemsetAsync(c->nextKind.p, NEXT_LARGE, N, s));  // ... and so does A.nextKind say, which the resident launch reads (RunResident)
    HIP_CHECK(hipMemsetAsync(c->film.p, 0, c->film.n * sizeof(float), s));
    if (c->filmExact) c->filmFx.Alloc(c->film.n + 1);  // zeroed; the last word is the film_overflow counter
    else
        c->filmFx.Free();
    LayersAlloc(c);  // "film_layers": the layers and the labels of the pending lists
    HIP_CHECK(hipStreamSynchronize(s));
    WarmStepLaunches(c);
    c->chainsSince = std::chrono::steady_clock::now();
}

namespace {
// the ranks of one job run the four phases in lock step; `g` = the member contexts this process drives (one for an RCCL rank)
void RunInit(const std::vector<lmc_ctx *> &g, long long numInitSamples, int numChainsTotal, int initThreads, const std::vector<std::pair<int, int>> &ranges,
             long long perChain, long long chainsNeedExtra) {
    if (numInitSamples <= 0) throw std::runtime_error("lmc_chains_init: no init samples");
    for (lmc_ctx *c : g) LayersCheckInit(c, g.size() > 1 ? "lmc_group_chains_init" : "lmc_chains_init");  // before anything changes
    std::vector<std::unique_ptr<InitJob>> jobs;
    for (size_t k = 0; k < g.size(); k++) {
        lmc_ctx *c = g[k];
        if (numChainsTotal <= 0 || ranges[k].first < 0 || ranges[k].second > numChainsTotal || ranges[k].second <= ranges[k].first) throw std::runtime_error("bad chain range");
        std::unique_ptr<InitJob> J(new InitJob);
        J->V = std::max(1, initThreads);
        J->numInitSamples = numInitSamples, J->perThread = numInitSamples / J->V, J->extra = numInitSamples % J->V;
        J->numChainsTotal = numChainsTotal, J->chainBegin = ranges[k].first, J->chainEnd = ranges[k].second, J->perChain = perChain, J->chainsNeedExtra = chainsNeedExtra;
        J->world = c->world, J->rank = c->rank;
        c->numInitSamples = numInitSamples, c->initThreads = J->V;
        jobs.push_back(std::move(J));
    }
    auto jobOf = [&](lmc_ctx *c) -> InitJob & {
        for (size_t k = 0; k < g.size(); k++)
            if (g[k] == c) return *jobs[k];
        throw std::runtime_error("internal: context outside its group");
    };
    // The init phases of the members run one after the other on the calling thread: each allocates, frees and synchronises (hipMalloc / hipFree /
    // hipStreamSynchronize), and with a host thread per member -- as the step loop has, where nothing is allocated -- the runtime aborted the
    // process once in eight runs of the group tests on one device (profiles/r05_final_note_group_init_abort.txt).  MLTInit is not in any timed region.
    for (size_t k = 0; k < g.size(); k++) InitPhase1(g[k], *jobs[k]);
    AllGatherBlocks(g, [&](lmc_ctx *c) { return (void *)jobOf(c).count.p; }, [&](lmc_ctx *c) { return (void *)jobOf(c).gatherCount.p; }, (size_t)jobs[0]->maxLocalSamples);
    for (size_t k = 0; k < g.size(); k++) InitPhase2(g[k], *jobs[k]);
    AllGatherBlocks(g, [&](lmc_ctx *c) { return (void *)jobOf(c).outCL.p; }, [&](lmc_ctx *c) { return (void *)jobOf(c).gatherCL.p; }, (size_t)jobs[0]->maxLocalContribs);
    AllGatherBlocks(g, [&](lmc_ctx *c) { return (void *)jobOf(c).outLs.p; }, [&](lmc_ctx *c) { return (void *)jobOf(c).gatherLs.p; }, (size_t)jobs[0]->maxLocalContribs * sizeof(float));
    for (size_t k = 0; k < g.size(); k++) InitPhase3(g[k], *jobs[k]);
    AllGatherBlocks(g, [&](lmc_ctx *c) { return (void *)jobOf(c).sendCk.p; }, [&](lmc_ctx *c) { return (void *)jobOf(c).gatherCk.p; }, (size_t)std::max(jobs[0]->maxOwned, 1) * 2 * sizeof(uint64_t));
    for (size_t k = 0; k < g.size(); k++) InitPhase4(g[k], *jobs[k]);
}
}  // namespace

// What the film merge of an in-process group needs, set up ONCE when the group is: direct peer access between the members' devices (checked
// with hipDeviceCanAccessPeer, enabled once per ordered pair; without it the runtime stages every peer copy through the host), every member's
// staging for the slices it pulls, the events the merge is ordered by.  Nothing is allocated inside lmc_group_film_reduce.
// the words lmc_group_film_reduce sums: the film, or with "film_layers" every layer and the overflow word behind them
static size_t MergeWords(const lmc_ctx *c) { return c->filmLayers ? (size_t)c->filmNLayers * c->film.n + 1 : c->film.n; }
static long long *MergeFx(lmc_ctx *c) { return c->filmLayers ? c->filmLayersFx.p : c->filmFx.p; }
void lmc_host::GroupSetUpMerge(const std::vector<lmc_ctx *> &g) {
    const size_t n = g.size();
    std::vector<int> devs;
    for (lmc_ctx *c : g)
        if (std::find(devs.begin(), devs.end(), c->device) == devs.end()) devs.push_back(c->device);
    int pairs = 0, enabled = 0;
    for (int a : devs)
        for (int b : devs) {
            if (a == b) continue;
            pairs++;
            int can = 0;
            HIP_CHECK(hipDeviceCanAccessPeer(&can, a, b));
            if (!can) continue;
            HIP_CHECK(hipSetDevice(a));
            const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
            if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) enabled++;
            (void)hipGetLastError();  // "already enabled" is not an error to carry into the next check
        }
    for (lmc_ctx *c : g) {
        HIP_CHECK(hipSetDevice(c->device));
        c->groupDevices = (int)devs.size(), c->groupPeerPairs = pairs, c->groupPeerEnabled = enabled;
        if (n > 1) {
            const size_t slice = (MergeWords(c) + n - 1) / n;
            if (c->filmExact) c->filmStageFx.Alloc(slice * (n - 1), false), c->filmStage.Free();
            else
                c->filmStage.Alloc(slice * (n - 1), false), c->filmStageFx.Free();
            c->weightStage.Alloc(n, false);
        }
        for (hipEvent_t *e : {&c->filmReadyEvent, &c->sliceReducedEvent, &c->weightsCopiedEvent})
            if (!*e) HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
}

extern "C" {

int lmc_chains_init(lmc_ctx *c, long long numInitSamples, int numChainsTotal, int initThreads, int chainBegin, int chainEnd, long long perChain,
                    long long chainsNeedExtra) {
    LMC_TRY
    if (c->group.size() > 1) throw std::runtime_error("lmc_chains_init: this context is a member of an in-process group, use lmc_group_chains_init");
    RunInit({c}, numInitSamples, numChainsTotal, initThreads, {{chainBegin, chainEnd}}, perChain, chainsNeedExtra);
    return 0;
    LMC_CATCH(-1)
}

// In-process group: the n contexts (one per GPU, or several on one GPU for bring-up and tests) become the ranks 0 .. n-1 of one job; its
// collectives are device copies between the members.  Chains are split into n contiguous, equal ranges (the last takes the rest).
int lmc_group_chains_init(lmc_ctx **ctxs, int n, long long numInitSamples, int numChainsTotal, int initThreads, long long perChain, long long chainsNeedExtra) {
    LMC_TRY
    if (n < 1) throw std::runtime_error("lmc_group_chains_init: empty group");
    std::vector<lmc_ctx *> g(ctxs, ctxs + n);
    std::vector<std::pair<int, int>> ranges;
    for (int r = 0; r < n; r++)
        if (g[r]->comm) throw std::runtime_error("lmc_group_chains_init: a member already belongs to an RCCL job");
    for (int r = 1; r < n; r++)  // before anything changes: the refused contexts stay as they were
        if (g[r]->filmExact != g[0]->filmExact)
            throw std::runtime_error("lmc_group_chains_init: the members differ in film_exact (member 0: " + std::to_string((int)g[0]->filmExact) + ", member " + std::to_string(r) + ": " + std::to_string((int)g[r]->filmExact) + "); a group's films are merged in one format");
    for (int r = 1; r < n; r++)
        if (g[r]->filmLayers != g[0]->filmLayers)
            throw std::runtime_error("lmc_group_chains_init: the members differ in film_layers (member 0: " + std::to_string(g[0]->filmLayers) + ", member " + std::to_string(r) + ": " + std::to_string(g[r]->filmLayers) + "); a group's films are merged layer by layer");
    for (int r = 0; r < n; r++) LayersCheckInit(g[r], "lmc_group_chains_init");
    for (int r = 0; r < n; r++) {
        for (lmc_ctx *peer : g[r]->group)  // leaving an earlier group: its other members must not keep a pointer to this context as a peer
            if (peer != g[r]) peer->group.clear(), peer->world = 1, peer->rank = 0;
        g[r]->world = n, g[r]->rank = r, g[r]->group = g;
        ranges.push_back({(int)((long long)numChainsTotal * r / n), (int)((long long)numChainsTotal * (r + 1) / n)});
    }
    try {
        RunInit(g, numInitSamples, numChainsTotal, initThreads, ranges, perChain, chainsNeedExtra);
        GroupSetUpMerge(g);
    } catch (...) {  // a failed init (too few contributions, a bad range) must not leave the contexts marked as ranks of an n-rank job
        for (lmc_ctx *c : g) c->group.clear(), c->world = 1, c->rank = 0, c->N = 0;
        throw;
    }
    return 0;
    LMC_CATCH(-1)
}

// out4 = [distinct devices among the members, ordered pairs of distinct member devices, ... of which have direct peer access enabled (the rest
// of the peer copies are staged by the runtime), host threads that drive the group's steps]
int lmc_group_info(lmc_ctx **ctxs, int n, long long *out4) {
    LMC_TRY
    if (n < 1 || ctxs[0]->group.size() != (size_t)n) throw std::runtime_error("lmc_group_info: not a group lmc_group_chains_init set up");
    out4[0] = ctxs[0]->groupDevices, out4[1] = ctxs[0]->groupPeerPairs, out4[2] = ctxs[0]->groupPeerEnabled, out4[3] = GroupThreads() ? n : 1;
    return 0;
    LMC_CATCH(-1)
}

long long lmc_init_contribs(lmc_ctx *c, long long cap, long long *sample, int *cl, float *ls) {
    const long long n = (long long)c->initCL.size();
    size_t g = 0;
    for (long long i = 0; i < n && i < cap; i++) {
        while (g + 1 < c->initOffsets.size() && c->initOffsets[g + 1] <= (unsigned long long)i) g++;
        sample[i] = (long long)g, cl[i] = c->initCL[i], ls[i] = c->initLs[i];
    }
    return n;
}

int lmc_init_result(lmc_ctx *c, float *normalization, long long *numContribs) {
    if (normalization) *normalization = c->normalization;
    if (numContribs) *numContribs = c->numInitContribs;
    return 0;
}

}  // extern "C"

// After every step, until all caches in use are full: apply the step's pushes (three small launches for all dims), read the
// four fill counts back and build the kd-tree of a dim that has just reached PSS_MAX_SIZE (global_cache.h:85-92), so
// that the next step already queries it -- the lock-step contract the oracle implements too.
// bit d: small steps of dimension d run the lean launch (MALA with that dim's cache ready and shallow enough for the LDS search)
static unsigned LeanDims(const lmc_ctx *c) {
    unsigned m = 0;
    if (c->S.opt.h2mc || !c->S.opt.mala || c->S.opt.useLightCoord || c->S.opt.sampleCache) return 0;  // light-coordinate sampling and chain.path (samplecache) live in the generic small step only
    for (int d = PSS_MIN_LENGTH; d <= PSS_MAX_LENGTH; d++)
        if (c->cacheDims[d].ready && !c->cacheHost.d[d].deep) m |= 1u << d;
    return m;
}
// The fill side of the global cache after a step, in three parts so that the ranks of a job can exchange their pushes in between:
//   CachePack         the step's pushes of THIS rank's chains, in chain order, into the rank's stage (kernels.hip k_push_*)
//   (exchange)        all-gather of the stages: RCCL, device copies inside an in-process group, nothing for a single rank
//   CacheApplyLaunch  the gathered rows appended in rank order = global chain-id order (k_push_apply), fill counts on their way to the host
//   CacheApplyFinish  the kd-tree and the existence grid of a dim that has just reached PSS_MAX_SIZE built (global_cache.h:85-92), so that
//                     the next step already queries it -- the lock-step contract the oracle implements too
// Every rank applies the same rows to the same cache, so "which dims are ready" is the same on all of them without asking.
bool lmc_host::CachePending(lmc_ctx *c) {
    bool anyPending = false;
    for (int d = 6; d <= PSS_MAX_LENGTH; d += 2) anyPending = anyPending || (c->cacheDims[d].relevant && !c->cacheDims[d].ready);
    if (!anyPending) {
        c->allCachesReady = true;
        bool anyDeep = false;
        for (int d = 2; d <= PSS_MAX_LENGTH; d++) anyDeep = anyDeep || (c->cacheDims[d].ready && c->cacheHost.d[d].deep);
        c->needGeneric = anyDeep || c->S.opt.useLightCoord || c->S.opt.sampleCache || c->S.opt.leanLightless;
        // leanLightless: the generic launch stays as the home of a state with l > 1 (possible, never seen: an environment light's
        // sub-paths almost never connect), but as a token launch of a few blocks -- 16384 workgroups that find an empty list still
        // queue for SIMD slots behind the hot launch's waves and cost it 1.3 % (profiles/r03_aa_ab_lean_lightless.jsonl)
        c->genericTokenOnly = c->S.opt.leanLightless && !(anyDeep || c->S.opt.useLightCoord || c->S.opt.sampleCache);
    }
    return anyPending;
}
// Only large steps push (dstep.h: the isLarge accept branch), so the pack is queued behind the large-step launch on ITS stream and runs
// beside the small-step launches instead of after them.
static void CachePack(lmc_ctx *c, hipStream_t s) {
    LaunchCachePush(c->A, c->stageT, c->pushTiles.p, reinterpret_cast<int *>(c->pushStage.p) /* the stage's row counts */, s);
}
// The device half of the apply, on stream s: the rows appended, and -- only when a pending dim can have reached PSS_MAX_SIZE -- the fill
// counts on their way to the host (countsEvent).  A single rank queues it behind its pack on the large-step stream: the rows of a dim that is
// not ready have no reader among the step's kernels, and the host then learns the counts long before the hot launch ends -- in all the steps
// in which no dim became ready it never waits for the step (0.15 ms per step of the fill phase at 2^20 chains, profiles/r04_fill_o_*).
static void CacheApplyLaunch(lmc_ctx *c, hipStream_t s) {
    const float *gathered = c->world > 1 ? c->pushGather.p : c->pushStage.p;
    // The fill counts are sent to the host (which has to know at the end of the step whether a dim became ready) only when a pending dim can
    // have reached PSS_MAX_SIZE since they last were: a step adds at most one row per chain of the job.  A render with few chains,
    // or a dim that fills slowly, does not pay a pipeline bubble per step (ADVICE r1 / VERDICT r2 item 8); the result is the same.
    c->stepsSinceCounts++;
    bool canBeFull = false;
    for (int sl = 0; sl < CACHE_SLOTS; sl++) {
        const CacheDimHost &cd = c->cacheDims[6 + 2 * sl];
        if (cd.relevant && !cd.ready && (long long)c->lastCounts[sl] + (long long)c->numChainsTotal * c->stepsSinceCounts >= PSS_MAX_SIZE) canBeFull = true;
    }
    c->countsInFlight = canBeFull;
    LaunchCachePushApply(gathered, (size_t)c->stageLayout.totalFloats, c->world, c->stageLayout, c->pushT, canBeFull ? c->hostCounts : nullptr, s);
    static const bool prefetch = !getenv("LMC_NO_ROWS_PREFETCH");
    for (int sl = 0; sl < CACHE_SLOTS && canBeFull && prefetch; sl++) {
        CacheDimHost &cd = c->cacheDims[6 + 2 * sl];
        c->rowsPrefetched[sl] = false;
        // expected to fill in this step at the rate of the last ones (twice the rate, to be on the safe side: a wrong guess costs one copy of 70-140 KB
        // or, the other way, the fetch after the counts as before)
        if (!cd.relevant || cd.ready || (long long)c->lastCounts[sl] + 2ll * c->lastDelta[sl] * c->stepsSinceCounts < PSS_MAX_SIZE) continue;
        if (!c->rowsPinned[sl]) HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&c->rowsPinned[sl]), (size_t)PSS_MAX_SIZE * PSS_MAX_LENGTH * sizeof(float)));
        HIP_CHECK(hipMemcpyAsync(c->rowsPinned[sl], cd.pss.p, cd.pss.n * sizeof(float), hipMemcpyDeviceToHost, s));
        c->rowsPrefetched[sl] = true;
    }
    if (canBeFull) HIP_CHECK(hipEventRecord(c->countsEvent, s));
}
// A dim whose rows, existence grid and kd-tree are in place (or on their way, in stream order) enters the host's copy of the cache struct: what
// CacheApplyFinish does when a dim fills up, and lmc_checkpoint_load for the dims its file holds ready
void lmc_host::PublishCacheDim(lmc_ctx *c, int d, const lmc::KdTreeResult &t, hipStream_t s) {
    CacheDimHost &cd = c->cacheDims[d];
    DCacheDim &D = c->cacheHost.d[d];
    D.gridWords = c->useOccFilter ? cd.gridWords.p : nullptr, D.gridCellStart = cd.gridCellStart.p, D.gridIdx = cd.gridIdx.p, D.gridG = cd.gridG, D.gridM = cd.gridM;
    for (int k = 0; k < 4; k++) D.gridCoord[k] = cd.gridCoord[k];
    if (t.depth >= KD_STACK) throw std::runtime_error("kd-tree deeper than the search stack (KD_STACK)");
    D.deep = 0;  // every kernel searches with KD_STACK private frames now; the field routed deep trees away from the former LDS search
    c->anyDeepCache = c->anyDeepCache || D.deep;
    D.ready = 1, D.nodes = cd.nodes.p, D.vind = cd.vind.p, D.pts = cd.pss.p, D.v1 = cd.v1.p, D.v2 = cd.v2.p;
    for (int k = 0; k < d; k++) D.rootLow[k] = t.rootLow[k], D.rootHigh[k] = t.rootHigh[k];
    D.extra = nullptr, D.weight = nullptr, D.distCdf = nullptr, D.scoreSum = 0, D.invSigmaSq = D.factor = 0.f;
    if (c->S.opt.sampleCache) {  // what LargeStepCache samples and evaluates (global_cache.h:57-58,84-90): on the host like the reference, once per dim
        std::vector<float> w = cd.weight.Download(), func, cdf;
        float funcInt = 0.f;
        lmc::BuildPiecewise1D(w.data(), PSS_MAX_SIZE, func, cdf, funcInt);  // data_distrib
        double scoreSum = 0;
        for (float x : w) scoreSum += x;  // score_sum: double, in push order
        HIP_CHECK(hipMemcpyAsync(cd.distCdf.p, cdf.data(), cdf.size() * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));
        D.extra = cd.extra.p, D.weight = cd.weight.p, D.distCdf = cd.distCdf.p, D.scoreSum = scoreSum;
        D.invSigmaSq = 1.0f / (0.15f * 0.15f);  // inverse(CACHE_SIG * CACHE_SIG)
        D.factor = lmcd::lexpf(d * (0.5f * lmcd::llogf(D.invSigmaSq) - 0.9189385332046727f));
    }
}
// The host half: the counts looked at, the kd-tree and the existence grid of a dim that has just become ready built (stream = the step stream)
static void CacheApplyFinish(lmc_ctx *c) {
    hipStream_t s = c->stream;
    if (!c->countsInFlight) return;
    c->countsInFlight = false;
    static const bool tlog = getenv("LMC_CACHE_LOG") != nullptr;  // measurement: host time of the transition's parts (stderr)
    const auto T0 = std::chrono::steady_clock::now();
    auto mark = [&](const char *what) {
        if (tlog) fprintf(stderr, "[lmc] cache transition: %-28s +%.3f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count());
    };
    HIP_CHECK(hipEventSynchronize(c->countsEvent));
    mark("counts on the host");
    for (int sl = 0; sl < CACHE_SLOTS; sl++) {
        c->lastDelta[sl] = (int)((c->hostCounts[sl] - c->lastCounts[sl] + c->stepsSinceCounts - 1) / std::max(1ll, c->stepsSinceCounts));
        c->lastCounts[sl] = c->hostCounts[sl];
    }
    c->stepsSinceCounts = 0;
    bool changed = false;
    // the dims that became ready in this step (often two at once: at 2^20 chains dims 10 and 12 fill in the same step): the existence
    // grids are started on the device first, the point rows are fetched, and the kd-trees are built side by side on host threads
    // (0.5 ms each; one after the other they made that step 1 ms longer, profiles/r03_o_step_timeline.jsonl step 22)
    int readyDims[CACHE_SLOTS], numReady = 0;
    for (int sl = 0; sl < CACHE_SLOTS; sl++) {
        const int d = 6 + 2 * sl;
        const CacheDimHost &cd = c->cacheDims[d];
        if (cd.relevant && !cd.ready && c->hostCounts[sl] >= PSS_MAX_SIZE) readyDims[numReady++] = d;
    }
    std::vector<std::vector<float>> ptsOf(numReady);
    std::vector<lmc::KdTreeResult> treeOf(numReady);
    // a single rank has applied the pushes on the large-step stream and is here while the hot launch still runs: the rows are fetched on that
    // stream (a blocking copy would wait for the step stream), and the kd-trees below are built beside the hot launch instead of after it
    // ... on the context's cache stream, that is: the large-step stream already holds the step's relocation behind the pushes, and the step stream
    // the hot launch -- waiting on either put the whole transition (rows down 0.05 ms, two kd-trees 0.5 ms, two grids 0.6 ms, trees up) BEHIND the
    // hot launch: the step in which dims 10 and 12 become ready took 2.6 ms instead of 1.75 (profiles/r05_final_step_durations_fill_phase.txt).
    // The pushes of this step are applied (countsEvent above), so nothing on that stream has to wait for anything.
    const bool beside = c->appliedEarly && c->overlap && c->cacheStream && !c->S.opt.sampleCache && !getenv("LMC_NO_CACHE_STREAM");
    hipStream_t cs = beside ? c->cacheStream : s;
    int toFetch = 0;
    for (int r = 0; r < numReady; r++) {
        const int sl = (readyDims[r] - 6) / 2;
        const DevBuf<float> &b = c->cacheDims[readyDims[r]].pss;
        if (c->rowsPrefetched[sl]) ptsOf[r].assign(c->rowsPinned[sl], c->rowsPinned[sl] + b.n);  // sent behind the apply (CacheApplyLaunch), complete since countsEvent
        else
            toFetch++;
    }
    if (tlog && numReady) fprintf(stderr, "[lmc] cache transition: %d of %d dims' rows were prefetched\n", numReady - toFetch, numReady);
    if (toFetch == 0) {
    } else if (beside || (c->appliedEarly && c->overlap)) {
        hipStream_t fs = beside ? cs : c->sideStream[0];
        for (int r = 0; r < numReady; r++) {
            if (!ptsOf[r].empty()) continue;
            const DevBuf<float> &b = c->cacheDims[readyDims[r]].pss;
            ptsOf[r].resize(b.n);
            HIP_CHECK(hipMemcpyAsync(ptsOf[r].data(), b.p, b.n * sizeof(float), hipMemcpyDeviceToHost, fs));
        }
        HIP_CHECK(hipStreamSynchronize(fs));
    } else {
        for (int r = 0; r < numReady; r++)
            if (ptsOf[r].empty()) ptsOf[r] = c->cacheDims[readyDims[r]].pss.Download();
    }
    for (int sl = 0; sl < CACHE_SLOTS; sl++) c->rowsPrefetched[sl] = false;
    if (numReady) mark("rows on the host");
    for (int r = 0; r < numReady; r++) {
        CacheDimHost &cd = c->cacheDims[readyDims[r]];
        lmc::ChooseGridCoords(ptsOf[r].data(), PSS_MAX_SIZE, readyDims[r], cd.gridM, cd.gridCoord);
        LaunchBuildCacheGrid(cd.pss.p, PSS_MAX_SIZE, readyDims[r], cd.gridG, cd.gridM, cd.gridCoord, c->gridScratchStart.p, c->gridScratchCursor.p, c->gridScratchWordCount.p, c->gridTileSums.p,
                             cd.gridWords.p, cd.gridCellStart.p, cd.gridIdx.p, cs);
    }
    if (numReady) mark("grid builds queued");
    {
        std::vector<std::thread> workers;
        std::vector<std::exception_ptr> failed(numReady);  // an exception must not leave a worker thread (std::terminate): re-thrown after the join
        for (int r = 1; r < numReady; r++)
            workers.emplace_back([&, r]() {
                try {
                    treeOf[r] = lmc::BuildKdTree(ptsOf[r].data(), PSS_MAX_SIZE, readyDims[r]);
                } catch (...) {
                    failed[r] = std::current_exception();
                }
            });
        try {
            if (numReady > 0) treeOf[0] = lmc::BuildKdTree(ptsOf[0].data(), PSS_MAX_SIZE, readyDims[0]);
        } catch (...) {
            failed[0] = std::current_exception();
        }
        for (auto &w : workers) w.join();
        for (auto &f : failed)
            if (f) std::rethrow_exception(f);
    }
    if (numReady) mark("kd-trees built");
    lmcd::UploadSegments treesUp;
    static_assert(sizeof(KdNode) % 4 == 0 && 2 * CACHE_SLOTS <= lmcd::UPLOAD_MAX_SEGMENTS, "the trees go up word by word, two segments per dim");
    for (int r = 0; r < numReady; r++) {
        const int d = readyDims[r];
        CacheDimHost &cd = c->cacheDims[d];
        lmc::KdTreeResult &t = treeOf[r];
        if (t.nodes.size() > KD_MAX_NODES) throw std::runtime_error("kd-tree larger than its preallocated node buffer");
        {
            const int sl = (d - 6) / 2;
            const size_t nodeBytes = t.nodes.size() * sizeof(KdNode), vindBytes = t.vind.size() * sizeof(int);
            if (!c->treePinned[sl]) HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&c->treePinned[sl]), (size_t)KD_MAX_NODES * sizeof(KdNode) + (size_t)PSS_MAX_SIZE * sizeof(int)));
            if (vindBytes > (size_t)PSS_MAX_SIZE * sizeof(int)) throw std::runtime_error("kd-tree point order larger than the cache");
            memcpy(c->treePinned[sl], t.nodes.data(), nodeBytes);
            memcpy(c->treePinned[sl] + (size_t)KD_MAX_NODES * sizeof(KdNode), t.vind.data(), vindBytes);
            treesUp.Add(cd.nodes.p, c->treePinned[sl], nodeBytes);
            treesUp.Add(cd.vind.p, c->treePinned[sl] + (size_t)KD_MAX_NODES * sizeof(KdNode), vindBytes);
        }
        PublishCacheDim(c, d, t, s);
        cd.ready = true;
        changed = true;
    }
    LaunchUploadSegments(treesUp, cs);  // one launch for all of them, behind the grid builds on the same stream (upload.h)
    if (numReady) mark("trees on their way up");
    if (changed && beside) {  // the next step's launches (stream s and its forks) read the trees and the grids built on the cache stream
        if (!c->treesUpEvent) HIP_CHECK(hipEventCreateWithFlags(&c->treesUpEvent, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(c->treesUpEvent, cs));
        HIP_CHECK(hipStreamWaitEvent(s, c->treesUpEvent, 0));
    }
    if (changed && !beside) HIP_CHECK(hipStreamSynchronize(s));  // the struct is replaced by a blocking copy below: nothing of this step may still read it
    if (changed) UploadCacheStruct(c, beside ? s : nullptr);
    if (numReady) mark("cache struct refreshed");  // beside: the step's launches are still running and read the struct as it was; `s` is behind all of them (StepPhase1's joins)
}

namespace {
void CheckSteppable(lmc_ctx *c) {
    if (c->N <= 0) throw std::runtime_error("lmc_chains_step before lmc_chains_init");
    // the chain state (H2MC Gaussian buffers, cache bookkeeping, work lists) is laid out for the mutation in force at init
    if (c->mutationAtInit != MutationKey(c))
        throw std::runtime_error("the 'mala' / 'h2mc' / 'samplecache' / 'uselightcoordinatesampling' options changed after lmc_chains_init: initialise the chains again before stepping");
    if (c->S.opt.sampleCache && !c->scene->options.largeStepMultiplexed)
        throw std::runtime_error("samplecache needs largestepmultiplexed (mutation_large_cache.h:33)");
}
}  // namespace
StepParams lmc_host::MakeStepParams(const lmc_ctx *c) {
    StepParams P;
    P.normalization = c->normalization, P.numChains = c->numChainsTotal, P.chainBegin = c->chainBegin, P.useGradient = c->useGradient, P.maxDervDepth = c->maxDervDepth, P.expFlags = c->expFlags;
    const bool mux = c->scene->options.largeStepMultiplexed;
    P.lengthCount = mux ? (int)c->lengthFunc.size() : 0, P.lengthFuncInt = c->lengthFuncInt;
    for (int k = 0; k < P.lengthCount; k++) P.lengthFunc[k] = c->lengthFunc[k];
    for (int k = 0; k <= P.lengthCount; k++) P.lengthCdf[k] = c->lengthCdf[k];
    return P;
}
namespace {
// which large-step / generic small-step kernel the options in force select (cnt: the three list lengths on the device)
Film StepFilm(lmc_ctx *c) { return c->filmExact ? FilmFx(c->filmFx.p, c->S.cam.width, c->S.cam.height) : Film{c->film.p, c->S.cam.width, c->S.cam.height}; }
// "film_layers": every launch below takes its layered form (device/step_*_layers.hip) with the film LayeredFilm(c) instead; `film` is then not used
void LaunchLarge(lmc_ctx *c, const Film &film, const StepParams &P, int cur, const int *cnt, const NextLists &next, hipStream_t sL) {
    const bool mux = c->scene->options.largeStepMultiplexed;
    if (c->filmLayers) {
        (c->S.opt.sampleCache ? LaunchStepLargeCacheLayers : mux ? LaunchStepLargeMuxLayers : LaunchStepLargeLayers)(c->S, c->cacheDev.p, c->A, LayeredFilm(c), P, c->lists[cur][0].p, cnt + 0, next, c->gradBuf.p, c->gradStride, c->S.glossy != 0, c->stepGrid, c->largeLdsStack ? c->bvhDepth : 1 << 30, c->largeBlock, sL);
        return;
    }
    (c->S.opt.sampleCache ? LaunchStepLargeCache : mux ? LaunchStepLargeMux : LaunchStepLarge)(c->S, c->cacheDev.p, c->A, film, P, c->lists[cur][0].p, cnt + 0, next, c->gradBuf.p, c->gradStride, c->S.glossy != 0, c->stepGrid, c->largeLdsStack ? c->bvhDepth : 1 << 30, c->largeBlock, sL);
}
void LaunchGeneric(lmc_ctx *c, const Film &film, const StepParams &P, int cur, const int *cnt, const NextLists &next, hipStream_t sG) {
    if (c->needGeneric && c->S.opt.h2mc) {  // the H2MC small step: lane-per-chain phases around the wave-cooperative Hessian / eigen-solve launches (device/dh2coop.h)
        const int *list = c->lists[cur][1].p, *n = cnt + 1;
        const int N = (int)c->N, laneGrid = c->stepGrid * 4;
        const lmcd::H2MCParam param = lmcd::MakeH2MCParam(c->S.opt.perturbStdDev);
        // One launch owns the GPU at a time inside a pipeline (the Hessian launch's waves take a SIMD's whole register file; the lane-per-chain
        // phases wait for memory), so TWO halves of the chain population run it side by side, each on its own stream: the tail of one half's launch
        // is filled by the other half's (measured as two contexts on one device before it was built, profiles/r05_s_h2mc_two_halves.jsonl:
        // veach-door +6 %, torus +9 %; four parts: nothing).  Same chains, same arithmetic: every chain's trajectory is untouched.
        const int parts = c->overlap ? c->h2Parts : 1;
        constexpr int MP = lmc_ctx::H2_MAX_PARTS;
        const int *lists[MP] = {list, list, list, list}, *counts[MP] = {n, n, n, n};
        hipStream_t streams[MP] = {sG, sG, sG, sG};
        if (parts >= 2) {
            // the list was cut into its halves when it was built (StepPhase2); cut here only on the first use of a list that was not (warm-up).  At the head
            // of the step the cut sat 1.5 ms in the queue beside the large-step launch, with the whole pipeline behind it (profiles/r05_x_h2mc_step_timeline_*.txt)
            if (c->h2SplitOf != list) LaunchSplitList(list, n, parts, c->h2SubList.p, c->h2PartStride, c->h2SubCount.p, laneGrid + 1, sG);
            c->h2SplitOf = nullptr;
            HIP_CHECK(hipEventRecord(c->partFork, sG));
            for (int h = 1; h < parts; h++) {
                HIP_CHECK(hipStreamWaitEvent(c->partStream[h - 1], c->partFork, 0));
                streams[h] = c->partStream[h - 1];
            }
            for (int h = 0; h < parts; h++) lists[h] = c->h2SubList.p + (size_t)h * c->h2PartStride, counts[h] = c->h2SubCount.p + h;
        }
        for (int h = 0; h < parts; h++) {
            hipStream_t sp = streams[h];
            H2Arrays H = c->H2;
            H.bins[0] = c->h2Bins[h][0], H.bins[1] = c->h2Bins[h][1];
            const int grid = laneGrid / parts + 1;
            HIP_CHECK(hipMemsetAsync(c->h2Bins[h][0].count, 0, 2 * 3 * H2_COUNT_WORDS * sizeof(int), sp));  // both stages' tables of this part are contiguous
            LaunchH2Begin(c->S, c->A, P, H, lists[h], counts[h], grid, sp);
            // The large-step launch starts behind every part's k_h2_begin: released together with the pipelines it won the race for the machine by microseconds
            // and the pipelines' first launch -- a memset -- waited 1.5 ms for a slot with everything else behind it (profiles/r06_final_h2mc_timeline_door.txt).
            // LMC_H2_LARGE_AFTER: 0 = at once (veach-door 88.2 M), 1 = behind the begins (91.3 M), 2 = behind the first Hessian launches too (90.6 M); torus 73.1 / 72.6 / 72.5
            static const int largeAfter = getenv("LMC_H2_LARGE_AFTER") ? atoi(getenv("LMC_H2_LARGE_AFTER")) : 1;
            if (largeAfter == 1 && c->overlap) {
                if (!c->h2HeadDone[h]) HIP_CHECK(hipEventCreateWithFlags(&c->h2HeadDone[h], hipEventDisableTiming));
                HIP_CHECK(hipEventRecord(c->h2HeadDone[h], sp));
                c->h2HeadParts = h + 1;
            }
            LaunchBinsCompact(H.bins[0], lists[h], counts[h], grid, sp);
            for (int stage = 0; stage < 2; stage++) {
                if (!LMC_EXP(P.expFlags, 64)) LaunchH2Hess(H.rec, H.bins[stage], N, c->S.sceneParams, H.hout, c->h2HessGrid, sp);
                if (stage == 0 && largeAfter == 2 && c->overlap) {
                    if (!c->h2HeadDone[h]) HIP_CHECK(hipEventCreateWithFlags(&c->h2HeadDone[h], hipEventDisableTiming));
                    HIP_CHECK(hipEventRecord(c->h2HeadDone[h], sp));
                    c->h2HeadParts = h + 1;
                }
                LaunchH2Gauss(H.bins[stage], N, H.hout, param, P.expFlags, c->A.flags, stage, H.gauss, H.offset, H.px, c->h2GaussGrid, sp);
                if (stage == 0) {
                    LaunchH2Sample(lists[h], counts[h], N, c->A.flags, H.kind, c->A.curContrib, H.gauss, param.sigma, H.offset, H.py, grid, sp);
                    LaunchH2Perturb(c->S, c->A, P, H, lists[h], counts[h], c->bvhDepth, grid, sp);
                    LaunchBinsCompact(H.bins[1], lists[h], counts[h], grid, sp);
                }
            }
            LaunchH2Finish(c->S, c->cacheDev.p, c->A, film, P, H, lists[h], counts[h], grid, sp);
        }
        for (int h = 1; h < parts; h++) {  // the generic slot of the launch plan ends when every part has
            HIP_CHECK(hipEventRecord(c->partJoin[h - 1], c->partStream[h - 1]));
            HIP_CHECK(hipStreamWaitEvent(sG, c->partJoin[h - 1], 0));
        }
    } else if (c->needGeneric && c->MP.rec && !c->allCachesReady && !c->S.opt.useLightCoord) {
        // while a cache fills: the gradient steps as a pipeline, the path program wave-cooperative between lane-per-chain phases
        const int *list = c->lists[cur][1].p, *n = cnt + 1;
        static const int laneGridEnv = getenv("LMC_MALA_LANE_GRID") ? atoi(getenv("LMC_MALA_LANE_GRID")) : 0;
        const int N = (int)c->N, laneGrid = laneGridEnv > 0 ? std::min(laneGridEnv, c->stepGrid * 4) : c->stepGrid * 4;
        const MalaPipe &M = c->MP;  // the bin counts: zero-filled at set-up, zeroed again by k_mala_finish
        LaunchMalaBegin(c->S, c->cacheDev.p, c->A, P, M, list, n, laneGrid, sG);
        LaunchBinsCompact(M.bins[0], list, n, laneGrid, sG);
        LaunchMalaGrad(M.rec, M.bins[0], N, c->S.sceneParams, M.gout, c->h2HessGrid, sG);
        LaunchMalaMid(c->S, c->cacheDev.p, c->A, P, M, list, n, c->bvhDepth, c->S.glossy != 0, laneGrid, sG);
        LaunchBinsCompact(M.bins[1], list, n, laneGrid, sG);
        LaunchMalaGrad(M.rec, M.bins[1], N, c->S.sceneParams, M.gout, c->h2HessGrid, sG);
        if (c->filmLayers) LaunchMalaFinishLayers(c->S, c->cacheDev.p, c->A, LayeredFilm(c), P, M, list, n, laneGrid, sG);
        else
            LaunchMalaFinish(c->S, c->cacheDev.p, c->A, film, P, M, list, n, laneGrid, sG);
    } else if (c->needGeneric && c->leanGrad && !c->anyDeepCache && !c->S.opt.useLightCoord && !c->S.opt.sampleCache && c->bvhDepth <= BVH_LDS_STACK) {
        if (c->filmLayers) LaunchStepSmallLeanGradLayers(c->S, c->cacheDev.p, c->A, LayeredFilm(c), P, c->lists[cur][1].p, cnt + 1, next, c->gradBuf.p, c->gradStride, c->S.glossy != 0, c->genericTokenOnly ? 64 : c->stepGrid * 4, 64, c->bvhDepth, sG);
        else
            LaunchStepSmallLeanGrad(c->S, c->cacheDev.p, c->A, film, P, c->lists[cur][1].p, cnt + 1, next, c->gradBuf.p, c->gradStride, c->S.glossy != 0, c->genericTokenOnly ? 64 : c->stepGrid * 4, 64, c->bvhDepth, sG);
    } else if (c->needGeneric) {
        if (c->filmLayers) LaunchStepSmallGradLayers(c->S, c->cacheDev.p, c->A, LayeredFilm(c), P, c->lists[cur][1].p, cnt + 1, next, c->gradBuf.p, c->gradStride, c->S.glossy != 0, c->stepGrid, sG);
        else
            LaunchStepSmallGrad(c->S, c->cacheDev.p, c->A, film, P, c->lists[cur][1].p, cnt + 1, next, c->gradBuf.p, c->gradStride, c->S.glossy != 0, c->stepGrid, sG);
    }
}
void LaunchLean(lmc_ctx *c, const Film &film, const StepParams &P, const int *list, const int *cnt, const NextLists &next, hipStream_t s) {
    if (c->filmLayers) LaunchStepSmallPlainLayers(c->S, c->cacheDev.p, c->A, LayeredFilm(c), P, list, cnt, next, c->bvhDepth, c->S.glossy != 0, c->leanLdsStack, c->leanBlock, c->profileLean, s);
    else
        LaunchStepSmallPlain(c->S, c->cacheDev.p, c->A, film, P, list, cnt, next, c->bvhDepth, c->S.glossy != 0, c->leanLdsStack, c->leanBlock, c->profileLean, s);
}
// first half of one step: the three step launches; then, while a cache is filling, this rank's pushes into its stage.
// Returns whether the ranks have pushes to exchange.
bool StepPhase1(lmc_ctx *c, lmc_ctx::StepEvents &ev) {
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    c->filmReduced = false;
    const Film film = StepFilm(c);
    const StepParams P = MakeStepParams(c);
    if (c->timing) {
        if (c->eventPool.empty()) {
            for (auto &e : ev.e) HIP_CHECK(hipEventCreate(&e));
        } else {
            ev = c->eventPool.back();
            c->eventPool.pop_back();
        }
        HIP_CHECK(hipEventRecord(ev.e[0], s));
    }
    const int cur = c->parity, nxt = 1 - c->parity;
    if (c->diag) DiagStepBegin(c, cur);  // ahead of the fork: the relocation on the large-step stream rewrites A.chainId
    NextLists next{c->lists[nxt][0].p, c->lists[nxt][1].p, c->lists[nxt][2].p, c->listCounts[nxt].p};
    HIP_CHECK(hipMemsetAsync(c->listCounts[nxt].p, 0, 4 * sizeof(int), s));
    const int *cnt = c->listCounts[cur].p;
    hipStream_t sL = c->overlap ? c->sideStream[0] : s, sG = c->overlap ? c->sideStream[1] : s;
    if (c->overlap) {
        HIP_CHECK(hipEventRecord(c->forkEvent, s));
        HIP_CHECK(hipStreamWaitEvent(sL, c->forkEvent, 0));
        if (c->needGeneric) HIP_CHECK(hipStreamWaitEvent(sG, c->forkEvent, 0));
    }
    // H2MC: the pipeline of the small steps goes first -- its first launch (k_h2_begin) is short and everything behind it waits for
    // it; launched behind the large steps it sat in the queue for the whole large-step launch (r04_c kernel trace)
    const bool genericFirst = c->S.opt.h2mc != 0;
    const bool exchange = !c->allCachesReady && CachePending(c);
    c->appliedEarly = false;
    c->h2HeadParts = 0;
    auto large = [&] {
        for (int h = 0; h < c->h2HeadParts; h++) HIP_CHECK(hipStreamWaitEvent(sL, c->h2HeadDone[h], 0));
        if (c->timing) HIP_CHECK(hipEventRecord(ev.e[4], sL));
        LaunchLarge(c, film, P, cur, cnt, next, sL);
        if (c->timing) HIP_CHECK(hipEventRecord(ev.e[5], sL));
        if (exchange) {
            CachePack(c, sL);
            if (c->world == 1 && c->earlyApply) CacheApplyLaunch(c, sL), c->appliedEarly = true;
            // An RCCL rank (one context per process) does the same with the collective in between: the all-gather of the ranks' stages is queued HERE, on the
            // large-step stream behind the pack, and runs beside the hot launch -- on the step stream it sat behind every launch of the step, with the apply,
            // the counts' way to the host and the next step's lists behind it (a collective's latency + 1.3 MB per rank, every step of the fill phase).
            // Every rank reaches this point in every step of the fill phase (`exchange` is a function of the cache's state, which is the same on all of
            // them), so the collectives of a communicator keep one order: one all-gather per step here, the film's all-reduce at the end on the step stream.
            // LMC_RCCL_EARLY_EXCHANGE=0: behind the step's launches as before (A/B).  In-process groups keep their event-ordered copies (RunSteps).
            else if (c->world > 1 && c->group.size() <= 1 && c->comm && c->earlyApply && RcclEarlyExchange() && c->stageLayout.totalFloats > 0) {
                RcclCheck(GetRccl().AllGather(c->pushStage.p, c->pushGather.p, (size_t)c->stageLayout.totalFloats * sizeof(float), ncclUint8, (ncclComm_t)c->comm, sL),
                          "ncclAllGather(cache pushes, large-step stream)");
                CacheApplyLaunch(c, sL), c->appliedEarly = true;
            }
        }
        // the chains this launch gave a new technique move to the slots of their technique (relocate.hip) -- on this stream, beside the small-step
        // launches, whose chains it does not touch, and behind the pack, which reads the pushes of these very chains (in chain order: A.slotOf)
        if (c->relocate) {
            // the staging buffer is 3-4 KB per record.  Only the first relocation (every chain took a large step: the full sort) can
            // need N records; from the third step on it holds N / 2 (the most movers seen in a later step: 0.3 N, step 1 of a fresh population);
            // the move kernels skip a step that would need more (relocate.hip).  The free is a device-wide wait, once, in the second step.
            if (c->relocations == 2 && c->RB.capacity == (int)c->N && c->N >= 65536 && c->resortEvery == 0 && !getenv("LMC_RELOC_STAGING_FULL")) {  // (the full re-sort moves every chain: N records stay)
                // the members of an in-process group reach this point in the same step, each on its own host thread; concurrent hipFree /
                // hipMalloc is the pattern that aborted the group's threaded init one run in eight (RunInit), so the re-allocation is serialised
                // process-wide, and RB never points at a freed buffer: it is cleared first and set only after a successful Alloc
                static std::mutex stagingMutex;
                std::lock_guard<std::mutex> lock(stagingMutex);
                HIP_CHECK(hipStreamSynchronize(sL));
                const size_t cap = c->N / 2;
                c->RB.staging = nullptr, c->RB.capacity = 0;
                c->relocStaging.Alloc(cap * RelocRecordWords(c->S.opt.maxDepth), false);
                c->RB.staging = c->relocStaging.p, c->RB.capacity = (int)cap;
            }
            if (c->relocFine) LaunchRelocateFine(c->A, c->S.opt.maxDepth, c->RB, c->RS, c->S.opt.h2mc != 0, sL);
            else
                LaunchRelocate(c->A, c->S.opt.maxDepth, c->RB, c->S.opt.h2mc != 0, sL);
            c->relocations++;
        }
    };
    if (!genericFirst) large();
    // the generic small-step launch: chains that evaluate a gradient (until their dim's cache is ready) or whose
    // cache tree is too deep for the lean kernel; its list is empty once every cache is ready and shallow
    if (c->timing) HIP_CHECK(hipEventRecord(ev.e[6], sG));
    LaunchGeneric(c, film, P, cur, cnt, next, sG);
    if (c->timing) HIP_CHECK(hipEventRecord(ev.e[7], sG));
    if (genericFirst) large();
    if (c->timing) HIP_CHECK(hipEventRecord(ev.e[1], s));
    // every small step of an H2MC render runs the pipeline: the lean list is empty by construction (QueueNext, LeanDims), and its launch of
    // four-wave blocks sat in the queue for the length of the large-step launch
    if (!c->S.opt.h2mc) LaunchLean(c, film, P, c->lists[cur][2].p, cnt + 2, next, s);
    if (c->timing) HIP_CHECK(hipEventRecord(ev.e[2], s));
    if (c->overlap) {
        HIP_CHECK(hipEventRecord(c->joinEvent[0], sL));
        HIP_CHECK(hipStreamWaitEvent(s, c->joinEvent[0], 0));
        if (c->needGeneric) {
            HIP_CHECK(hipEventRecord(c->joinEvent[1], sG));
            HIP_CHECK(hipStreamWaitEvent(s, c->joinEvent[1], 0));
        }
    }
    return exchange;
}
// Experiment (lmc_set_option "exp_resort"): every chain re-placed in the order of a fine key, worked out on the host.  Stream s is behind all of the
// step's launches here (StepPhase1's joins) and the next step's lists are not built yet.
void DebugResort(lmc_ctx *c) {
    hipStream_t s = c->stream;
    const int mode = c->pendingResort;
    c->pendingResort = 0;
    const size_t N = c->N;
    HIP_CHECK(hipStreamSynchronize(s));
    if (c->RB.capacity < (int)N) {
        c->relocStaging.Alloc(N * RelocRecordWords(c->S.opt.maxDepth), false);
        c->RB.staging = c->relocStaging.p, c->RB.capacity = (int)N;
    }
    DevBuf<unsigned long long> keys;
    keys.Alloc(N, false);
    LaunchRelocFineKey(c->A, c->leafPosOfTri.p, c->S.numTris, mode, keys.p, c->S.tris, c->S.materials, s);
    HIP_CHECK(hipStreamSynchronize(s));
    const std::vector<unsigned long long> k = keys.Download();
    std::vector<int> perm(N);
    for (size_t i = 0; i < N; i++) perm[i] = (int)i;
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return k[a] < k[b]; });
    LaunchRelocIota((int)N, c->relocMembers.p, s);
    HIP_CHECK(hipMemcpyAsync(c->relocSorted.p, perm.data(), N * sizeof(int), hipMemcpyHostToDevice, s));
    const int cnt = (int)N;
    HIP_CHECK(hipMemcpyAsync(c->relocCount.p, &cnt, sizeof(int), hipMemcpyHostToDevice, s));
    LaunchRelocMove(c->A, c->S.opt.maxDepth, c->RB, s);
    HIP_CHECK(hipStreamSynchronize(s));
}
// second half: the gathered pushes applied (a cache that becomes ready at the end of this step -- mlt.cpp: push() flips is_ready
// inside the step -- is seen by the list build: chains whose next step no longer needs a gradient go to the lean launch right
// away), then the work lists of the next step
void StepPhase2(lmc_ctx *c, lmc_ctx::StepEvents &ev, bool exchanged) {
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int nxt = 1 - c->parity;
    if (exchanged) {
        if (!c->appliedEarly) CacheApplyLaunch(c, s);
        CacheApplyFinish(c);
    }
    if (c->diag) DiagStepEnd(c);
    if (c->pendingResort && c->relocate) DebugResort(c);
    // the periodic full re-sort (relocate.hip): stream s is behind all of the step's launches here (StepPhase1's joins) and the next step's lists are not built yet
    if (c->relocate && c->resortEvery > 0 && c->RB.capacity >= (int)c->N && c->stepsSinceInit >= c->resortFirst && (c->stepsSinceInit - c->resortFirst) % c->resortEvery == 0) {
        static const bool log = getenv("LMC_RESORT_LOG") != nullptr;
        std::chrono::steady_clock::time_point t0;
        if (log) {
            HIP_CHECK(hipStreamSynchronize(s));
            t0 = std::chrono::steady_clock::now();
        }
        LaunchRelocFullSort(c->A, c->S.opt.maxDepth, c->RB, c->RS, s);
        c->resorts++;
        if (log) {
            HIP_CHECK(hipStreamSynchronize(s));
            fprintf(stderr, "[lmc] full re-sort after step %lld: %.3f ms\n", c->stepsSinceInit, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
    }
    c->stepsSinceInit++;
    BuildNextLists(c, nxt);
    c->parity = nxt;
    if (c->timing) {
        HIP_CHECK(hipEventRecord(ev.e[3], s));
        c->events.push_back(ev);
    }
}
}  // namespace
// the work lists of the step that runs next, into lists[nxt] (their counts zeroed by the caller), on the step stream
void lmc_host::BuildNextLists(lmc_ctx *c, int nxt) {
    hipStream_t s = c->stream;
    NextLists next{c->lists[nxt][0].p, c->lists[nxt][1].p, c->lists[nxt][2].p, c->listCounts[nxt].p};
    const int sortPlain = c->relocate ? 0 : c->sortPlain;  // relocated chains are grouped already, and in place
    LaunchBuildLists(c->A, next, sortPlain == 4 ? 0 : sortPlain, LeanDims(c) | (c->S.opt.leanLightless ? 1u << 31 : 0u), s);
    if (sortPlain == 4) {  // A/B: the lean list grouped by technique over the WHOLE list (a wave then retraces one technique; its lanes' state lines are anywhere)
        LaunchSortByTechnique(c->A.nextKind, c->lists[nxt][2].p, c->listScratch2.p, c->listCounts[nxt].p + 2, c->sortBins2.p, (int)c->N, s);
        std::swap(c->lists[nxt][2].p, c->listScratch2.p);
    }
    // group the chains of the generic launch by technique: always for H2MC (a wave then runs ONE (c,l) program with one pass
    // count instead of the longest of 64; LMC_SORT_H2MC=0 for the A/B), optional for the gradient launch of LMC
    if (c->needGeneric && !c->genericTokenOnly && (c->S.opt.h2mc ? c->sortH2mc : (c->sortGeneric && c->S.opt.mala && !c->relocate))) {  // relocated chains are grouped already (LMC: every chain moves; H2MC: chains holding a Gaussian stay, the sort still pays: 58.9 vs 61.7 M)
        LaunchSortByTechnique(c->A.nextKind, c->lists[nxt][1].p, c->listScratch.p, c->listCounts[nxt].p + 1, c->sortBins.p, (int)c->N, s);
        std::swap(c->lists[nxt][1].p, c->listScratch.p);
    }
    if (c->needGeneric && c->S.opt.h2mc && c->overlap && c->h2Parts >= 2) {  // the two halves of the H2MC pipeline's list (LaunchGeneric), while nothing else runs
        LaunchSplitList(c->lists[nxt][1].p, c->listCounts[nxt].p + 1, c->h2Parts, c->h2SubList.p, c->h2PartStride, c->h2SubCount.p, c->stepGrid * 4 + 1, s);
        c->h2SplitOf = c->lists[nxt][1].p;
    }
}
// The first launch of a kernel on a stream pays one-time runtime work (code object upload, the private-memory ring of the queue:
// between 4 ms and, on a cold box, 140 ms for the lean kernel at 2^20 chains, profiles/r03_o_step_timeline.jsonl step 0).  MLTInit
// ends by launching the step kernels of the options in force once with EMPTY work lists, so that this is paid at set-up and not
// inside the first mutation of a render (first step 6.5 -> 2.3 ms on a warm box; LMC_NO_WARM_LAUNCH=1 for the A/B).
static void WarmStepLaunches(lmc_ctx *c) {
    if (getenv("LMC_NO_WARM_LAUNCH")) return;
    const Film film = StepFilm(c);
    const StepParams P = MakeStepParams(c);
    c->warmCounts.Alloc(4);  // zero-filled: three empty lists
    // DevBuf::Alloc zeroes with hipMemset on the null stream, which returns before the words are written, and the side streams are created
    // hipStreamNonBlocking: they do not wait for the null stream.  A warm launch that read a count before its zero had landed would step whatever the
    // (uninitialised) generic list names.  Seen once as an illegal access in this function, in a layered context, whose film's zeroing is queued in front.
    HIP_CHECK(hipStreamSynchronize(nullptr));
    NextLists next{c->lists[1][0].p, c->lists[1][1].p, c->lists[1][2].p, c->listCounts[1].p};
    hipStream_t s = c->stream, sL = c->overlap ? c->sideStream[0] : s, sG = c->overlap ? c->sideStream[1] : s;
    const int *cnt = c->warmCounts.p;
    LaunchLarge(c, film, P, 0, cnt, next, sL);
    LaunchGeneric(c, film, P, 0, cnt, next, sG);
    if (c->MP.rec && !c->allCachesReady) {  // ... and the launch that takes the generic slot once the caches are ready (first launched in the step after the fill phase: 1.2 ms, profiles/r04_fill_s_*)
        c->allCachesReady = true;
        LaunchGeneric(c, film, P, 0, cnt, next, sG);
        c->allCachesReady = false;
    }
    LaunchLean(c, film, P, c->lists[0][2].p, cnt + 2, next, s);
    HIP_CHECK(hipStreamSynchronize(sL));
    HIP_CHECK(hipStreamSynchronize(sG));
    HIP_CHECK(hipStreamSynchronize(s));
}
namespace {
// ---- the resident schedule (lmc_set_option "resident_steps" = K; device/step_resident.h)
// Cap of K: one resident launch runs at most kResidentBudget chain-steps and at most kResidentMaxK steps per chain, so that it stays in the tens of
// milliseconds -- it holds its waves for the whole launch, and a render is cut into launches the host can stop between.  Measured
// (profiles/r07_resident_sweep*.jsonl): a resident step of the slowest workload (veach-door LMC) takes 1.1 ms at 2^14 chains and 1.3 ms at 2^16, a
// launch of 2^21 chain-steps 25 .. 45 ms at 2^16 .. 2^20; K = 128 gained at most 5 % over 32 while its launches took 100 .. 240 ms.
// The number of active lanes per wave (ResidentLanes): 32 up to 2^16 chains, where a wave slot is free and fewer lanes mean less large / small and
// path-length divergence per wave (veach-door LMC +12 %, plain MLT +14 % at 2^16 against 64); 64 above (at 2^18 32 lanes cost 35 .. 45 %).
constexpr long long kResidentBudget = 1ll << 21;
constexpr int kResidentMaxK = 32;
int ResidentLanes(const lmc_ctx *c) { return c->residentLanes ? c->residentLanes : c->N <= 65536 ? 32 : 64; }
}  // namespace
int lmc_host::ResidentK(const lmc_ctx *c) {
    if (c->residentSteps <= 0 || c->N <= 0) return 0;
    const long long byBudget = std::max(1ll, kResidentBudget / (long long)c->N);
    return (int)std::min<long long>({(long long)c->residentSteps, (long long)kResidentMaxK, byBudget});
}
namespace {
// May this member's remaining steps run resident?  Not while a relevant cache dim is filling: the lock-step contract orders the pushes by step
// (mlt.cpp:120-127).  CachePending is what StepPhase1 would ask at the head of this very step (it sets allCachesReady from the step in which the
// last cache became ready); plain MLT never fills a cache, so its chains run resident from the first step.
bool ResidentEligible(lmc_ctx *c) {
    if (c->residentSteps <= 0 || c->S.opt.h2mc) return false;
    if (c->filmLayers) return false;  // the resident launch is not layered: lock step, by that schedule's contract the same trajectories
    if (c->diag && DiagNeedsLockStep(c)) return false;  // a resident launch cannot be observed between its mutations
    for (const lmc_ctx *m : c->group)                    // ... and the members of a group take the same schedule (RunSteps: they meet at barriers in lock step)
        if (m->diag && DiagNeedsLockStep(m)) return false;
    return c->allCachesReady || !CachePending(c);
}
// `steps` mutations of every chain as ceil(steps / K) resident launches on the step stream, then the hand-back to lock step: the next step's work
// lists from A.nextKind (every resident step ended with QueueNext) and stepsSinceInit advanced by the steps run.
void RunResident(lmc_ctx *c, int steps) {
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    c->filmReduced = false;
    const int K = ResidentK(c);
    const Film film = StepFilm(c);
    const StepParams P = MakeStepParams(c);
    const int mux = c->S.opt.sampleCache ? 2 : c->scene->options.largeStepMultiplexed ? 1 : 0;
    static const bool resortBetween = getenv("LMC_RESIDENT_RESORT") && atoi(getenv("LMC_RESIDENT_RESORT")) != 0;  // A/B: the full re-sort between resident launches
    std::pair<hipEvent_t, hipEvent_t> ev;
    HIP_CHECK(hipEventCreate(&ev.first));
    HIP_CHECK(hipEventCreate(&ev.second));
    c->residentEvents.push_back(ev);
    HIP_CHECK(hipEventRecord(ev.first, s));
    for (int done = 0; done < steps;) {
        const int k = std::min(K, steps - done);
        LaunchStepResident(c->S, c->cacheDev.p, c->A, film, P, k, ResidentLanes(c), c->residentGuard.p, c->S.glossy != 0, mux, c->largeLdsStack ? c->bvhDepth : 1 << 30, s);
        HIP_CHECK(hipGetLastError());
        c->residentLaunches++;
        c->stepsSinceInit += k;
        done += k;
        if (resortBetween && done < steps && c->relocate && c->resortEvery > 0 && c->RB.capacity >= (int)c->N) LaunchRelocFullSort(c->A, c->S.opt.maxDepth, c->RB, c->RS, s), c->resorts++;
    }
    HIP_CHECK(hipEventRecord(ev.second, s));
    const int nxt = 1 - c->parity;
    HIP_CHECK(hipMemsetAsync(c->listCounts[nxt].p, 0, 4 * sizeof(int), s));
    BuildNextLists(c, nxt);
    c->parity = nxt;
    // The resident launches skipped the per-step relocation: the chains' slots no longer follow their techniques.  Slot order is a performance matter
    // only (every result is per chain; lmc_chain_summary reports rows in chain order), so the re-sort waits for the next lock step (ResumeLockStep).
    c->residentResortPending = c->relocate;
}
// ahead of a lock step after resident launches: the full re-sort (relocate.hip) the resident run left due, and the lists rebuilt for the new slots
void ResumeLockStep(lmc_ctx *c) {
    if (!c->residentResortPending) return;
    c->residentResortPending = false;
    if (!c->relocate || c->resortEvery <= 0 || c->RB.capacity < (int)c->N) return;
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    LaunchRelocFullSort(c->A, c->S.opt.maxDepth, c->RB, c->RS, s);
    c->resorts++;
    HIP_CHECK(hipMemsetAsync(c->listCounts[c->parity].p, 0, 4 * sizeof(int), s));
    BuildNextLists(c, c->parity);
}
void RunSteps(const std::vector<lmc_ctx *> &g, int nSteps) {
    for (lmc_ctx *c : g) CheckSteppable(c);
    typedef std::chrono::steady_clock Clock;
    const size_t stageBytes = (size_t)g[0]->stageLayout.totalFloats * sizeof(float);
    if (g.size() == 1 || !GroupThreads()) {  // one rank (of an RCCL job or on its own), or the A/B form of a group: every member from this thread
        std::vector<lmc_ctx::StepEvents> ev(g.size());
        for (int it = 0; it < nSteps; it++) {
            bool resident = true;  // equal on all members: they hold the same cache at every step
            for (lmc_ctx *c : g) resident = ResidentEligible(c) && resident;
            if (resident) {
                for (lmc_ctx *c : g) RunResident(c, nSteps - it);
                break;
            }
            for (lmc_ctx *c : g) ResumeLockStep(c), c->lockSteps++;
            const auto t0 = Clock::now();
            bool exchange = false;
            for (size_t k = 0; k < g.size(); k++) {
                const bool e = StepPhase1(g[k], ev[k]);
                if (k > 0 && e != exchange) throw std::runtime_error("internal: the ranks of a job disagree on the state of the global cache");
                exchange = e;
            }
            if (exchange && g[0]->world > 1) ExchangeStagesAsync(g, stageBytes);
            for (size_t k = 0; k < g.size(); k++) StepPhase2(g[k], ev[k], exchange);
            const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
            for (lmc_ctx *c : g) c->hostIssueMs += ms / (double)g.size(), c->hostIssueSteps++;
        }
    } else {
        // in-process group: a host thread per member.  The members only meet while a gradient cache is filling (the exchange of the step's pushes:
        // two barriers of the host threads around the copies' queueing, none of the streams'); afterwards every thread runs ahead on its own.
        GroupBarrier bar((int)g.size());
        std::vector<char> wants(g.size(), 0);
        ForEachMember(g.size(), [&](size_t k) {
            lmc_ctx *c = g[k];
            lmc_ctx::StepEvents ev;
            for (int it = 0; it < nSteps; it++) {
                if (ResidentEligible(c)) {  // the same step on every member (same cache); from here on no member meets another
                    RunResident(c, nSteps - it);
                    break;
                }
                ResumeLockStep(c);
                c->lockSteps++;
                const auto t0 = Clock::now();
                const bool fill = !c->allCachesReady;  // equal on all members: they hold the same cache at every step
                const bool e = StepPhase1(c, ev);
                if (fill) {
                    wants[k] = e ? 1 : 0;
                    if (!bar.Wait()) return;
                    for (size_t q = 0; q < g.size(); q++)
                        if ((wants[q] != 0) != e) throw std::runtime_error("internal: the ranks of a job disagree on the state of the global cache");
                    if (e && stageBytes) {
                        ExchangeStagePartA(c);
                        if (!bar.Wait()) return;
                        ExchangeStagePartB(c, stageBytes);
                        if (!bar.Wait()) return;
                        ExchangeStagePartC(c);
                    }
                    if (!bar.Wait()) return;  // wants[] is rewritten by the next step
                } else if (e) {
                    throw std::runtime_error("internal: a cache push after every cache became ready");
                }
                StepPhase2(c, ev, e);
                c->hostIssueMs += std::chrono::duration<double, std::milli>(Clock::now() - t0).count(), c->hostIssueSteps++;
            }
        }, &bar);
    }
    for (lmc_ctx *c : g) {
        HIP_CHECK(hipSetDevice(c->device));
        HIP_CHECK(hipGetLastError());
        c->stepsDone += nSteps;
    }
}
}  // namespace

extern "C" {

int lmc_chains_step(lmc_ctx *c, int nSteps) {
    LMC_TRY
    if (c->group.size() > 1) throw std::runtime_error("lmc_chains_step: this context is a member of an in-process group, use lmc_group_chains_step");
    RunSteps({c}, nSteps);
    return 0;
    LMC_CATCH(-1)
}
int lmc_group_chains_step(lmc_ctx **ctxs, int n, int nSteps) {
    LMC_TRY
    std::vector<lmc_ctx *> g(ctxs, ctxs + n);
    for (lmc_ctx *c : g)
        if (c->group != g) throw std::runtime_error("lmc_group_chains_step: not the group lmc_group_chains_init set up");
    RunSteps(g, nSteps);
    return 0;
    LMC_CATCH(-1)
}

int lmc_sync(lmc_ctx *c) {
    LMC_TRY
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
    LMC_CATCH(-1)
}

int lmc_step_timing(lmc_ctx *c, double *kernelMs, long long *launches) {
    LMC_TRY
    HIP_CHECK(hipStreamSynchronize(c->stream));
    double ms = 0;
    c->smallMs = c->largeMs = c->largeOnlyMs = c->genericMs = 0;
    for (auto &ev : c->events) {
        float t = 0;
        HIP_CHECK(hipEventElapsedTime(&t, ev.e[0], ev.e[3]));
        ms += t;
        HIP_CHECK(hipEventElapsedTime(&t, ev.e[1], ev.e[2]));
        c->smallMs += t;
        HIP_CHECK(hipEventElapsedTime(&t, ev.e[4], ev.e[5]));
        c->largeMs += t, c->largeOnlyMs += t;
        HIP_CHECK(hipEventElapsedTime(&t, ev.e[6], ev.e[7]));
        c->largeMs += t, c->genericMs += t;
        c->eventPool.push_back(ev);
    }
    if (kernelMs) *kernelMs = ms;
    if (launches) *launches = (long long)c->events.size();
    c->events.clear();
    return 0;
    LMC_CATCH(-1)
}

int lmc_kernel_timing(lmc_ctx *c, double *out3) {
    LMC_TRY
    HIP_CHECK(hipStreamSynchronize(c->stream));
    out3[0] = c->smallMs, out3[1] = c->largeMs;
    out3[2] = (double)c->counters.Download()[7];
    return 0;
    LMC_CATCH(-1)
}

// the three step launches separately: [lean small-step ms, large-step ms, generic small-step ms (cache-filling gradient steps / all H2MC
// small steps), cumulative chain-steps of the lean kernel]
int lmc_kernel_timing_split(lmc_ctx *c, double *out4) {
    LMC_TRY
    HIP_CHECK(hipStreamSynchronize(c->stream));
    out4[0] = c->smallMs, out4[1] = c->largeOnlyMs, out4[2] = c->genericMs;
    out4[3] = (double)c->counters.Download()[7];
    return 0;
    LMC_CATCH(-1)
}

// region cycle sums of the lean kernel's profiling instantiation since the last call (LMC_PROF=1): out16[0..PR_COUNT) = wave cycles per
// region (dsmall.h PR_*), out16[PR_COUNT] = waves
int lmc_prof_read(lmc_ctx *c, unsigned long long *out16) {
    LMC_TRY
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (c->prof.n == 0) throw std::runtime_error("lmc_prof_read before lmc_chains_init");
    std::vector<unsigned long long> h = c->prof.Download();
    for (int k = 0; k < 16; k++) out16[k] = h[k];
    HIP_CHECK(hipMemset(c->prof.p, 0, 16 * sizeof(unsigned long long)));
    return 0;
    LMC_CATCH(-1)
}

// The film merge of an in-process job (mlt.cpp:203-207 MergeBuffer over the per-thread films; here: over the per-GPU films of the group's
// members), the in-process counterpart of lmc_film_allreduce (same semantics: in place, once per stepped film).  A direct reduce-scatter +
// all-gather over the point-to-point links: member k owns slice k of the film; it pulls slice k of every peer's film (n - 1 copies from n - 1
// different peers, i.e. over different xGMI links at once) into its staging and adds them in rank order, then every member pulls the finished
// slices of the others.  Per member 2 (n - 1) / n films cross the links, none of them through one member's links only, and nothing waits on
// the host in between: the copies and adds are ordered by events among the members' streams (filmReady -> pulls; sliceReduced -> the pulls of
// that slice, which also guarantees that the owner has finished reading the slice it is about to be overwritten with... of its peers).
// The weight sums: every member copies all n scalars, then adds them in rank order (the same double on every member).
// Staging, events and peer access were set up with the group (GroupSetUpMerge); out_ms (may be NULL): wall time of the merge.
int lmc_group_film_reduce(lmc_ctx **ctxs, int n, double *out_ms) {
    LMC_TRY
    std::vector<lmc_ctx *> g(ctxs, ctxs + n);
    for (lmc_ctx *c : g) {
        if (c->group != g) throw std::runtime_error("lmc_group_film_reduce: not the group lmc_group_chains_init set up");
        if (c->filmReduced) throw std::runtime_error("lmc_group_film_reduce: the films already hold the sum over the members; step or clear them first");
        if (c->film.n != g[0]->film.n) throw std::runtime_error("lmc_group_film_reduce: the members' films differ in size");
        if (c->filmExact != g[0]->filmExact) throw std::runtime_error("lmc_group_film_reduce: the members differ in film_exact");
        if (c->filmLayers != g[0]->filmLayers) throw std::runtime_error("lmc_group_film_reduce: the members differ in film_layers");
    }
    const bool exact = g[0]->filmExact;  // int64 slices, integer adds: the sum is the same in any order
    if (out_ms)  // only so that the reported time is the merge's own: the merge is stream-ordered behind the members' steps either way
        for (lmc_ctx *c : g) {
            HIP_CHECK(hipSetDevice(c->device));
            HIP_CHECK(hipStreamSynchronize(c->stream));
        }
    const auto t0 = std::chrono::steady_clock::now();
    const size_t total = MergeWords(g[0]), slice = (total + n - 1) / n;  // "film_layers": layer by layer, the layers being one array
    auto sliceLen = [&](int k) { return (size_t)k * slice >= total ? (size_t)0 : std::min(slice, total - (size_t)k * slice); };
    if (n > 1) {
        for (lmc_ctx *c : g) {  // every member's film (and weight sum) is final once its stream gets here
            HIP_CHECK(hipSetDevice(c->device));
            HIP_CHECK(hipEventRecord(c->filmReadyEvent, c->stream));
        }
        for (int k = 0; k < n; k++) {  // reduce-scatter: slice k summed on member k, peers added in rank order
            lmc_ctx *c = g[k];
            HIP_CHECK(hipSetDevice(c->device));
            int slot = 0;
            for (int m = 0; m < n; m++) {
                if (m != k) HIP_CHECK(hipStreamWaitEvent(c->stream, g[m]->filmReadyEvent, 0));
                HIP_CHECK(hipMemcpyPeerAsync(c->weightStage.p + m, c->device, g[m]->weightSum.p, g[m]->device, sizeof(double), c->stream));
                if (m == k || sliceLen(k) == 0) continue;
                if (exact) {
                    long long *st = c->filmStageFx.p + (size_t)slot * slice;
                    HIP_CHECK(hipMemcpyPeerAsync(st, c->device, MergeFx(g[m]) + (size_t)k * slice, g[m]->device, sliceLen(k) * sizeof(long long), c->stream));
                    LaunchAddIntoI64(MergeFx(c) + (size_t)k * slice, st, sliceLen(k), c->stream);
                } else {
                    float *st = c->filmStage.p + (size_t)slot * slice;
                    HIP_CHECK(hipMemcpyPeerAsync(st, c->device, g[m]->film.p + (size_t)k * slice, g[m]->device, sliceLen(k) * sizeof(float), c->stream));
                    LaunchAddInto(c->film.p + (size_t)k * slice, st, sliceLen(k), c->stream);
                }
                slot++;
            }
            HIP_CHECK(hipEventRecord(c->sliceReducedEvent, c->stream));
            HIP_CHECK(hipEventRecord(c->weightsCopiedEvent, c->stream));
        }
        for (int k = 0; k < n; k++) {  // all-gather: the finished slices of the peers; the weight sums once every member has read the old ones
            lmc_ctx *c = g[k];
            HIP_CHECK(hipSetDevice(c->device));
            for (int m = 0; m < n; m++) {
                if (m == k) continue;
                HIP_CHECK(hipStreamWaitEvent(c->stream, g[m]->sliceReducedEvent, 0));  // == weightsCopiedEvent of m: m has read this member's scalar
                if (sliceLen(m) && exact) HIP_CHECK(hipMemcpyPeerAsync(MergeFx(c) + (size_t)m * slice, c->device, MergeFx(g[m]) + (size_t)m * slice, g[m]->device, sliceLen(m) * sizeof(long long), c->stream));
                else if (sliceLen(m)) HIP_CHECK(hipMemcpyPeerAsync(c->film.p + (size_t)m * slice, c->device, g[m]->film.p + (size_t)m * slice, g[m]->device, sliceLen(m) * sizeof(float), c->stream));
            }
            LaunchSumF64(c->weightSum.p, c->weightStage.p, n, c->stream);
        }
    }
    for (lmc_ctx *c : g) {
        HIP_CHECK(hipSetDevice(c->device));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        c->filmReduced = true;
    }
    if (out_ms) *out_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
    LMC_CATCH(-1)
}

// host time spent queueing the launches of this context's steps since the last call, and the steps it covers (an in-process group: per member)
int lmc_host_issue_timing(lmc_ctx *c, double *ms, long long *steps) {
    LMC_TRY
    if (ms) *ms = c->hostIssueMs;
    if (steps) *steps = c->hostIssueSteps;
    c->hostIssueMs = 0, c->hostIssueSteps = 0;
    return 0;
    LMC_CATCH(-1)
}

int lmc_film_read(lmc_ctx *c, float *rgb) {
    LMC_TRY
    HIP_CHECK(hipSetDevice(c->device));
    SyncLayerSum(c);  // "film_layers": filmFx = the sum of the layers
    if (c->filmFx.p) LaunchFilmFixedToFloat(c->filmFx.p, c->film.p, c->film.n, c->stream);  // exact mode: converted on the device, float(double(q) * 2^-32)
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(rgb, c->film.p, c->film.n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}
// exact mode only: the raw fixed-point words (W*H*3, unit 2^-32 of the float film's unit) / the splats dropped for a component of 2^30 or more
int lmc_film_read_fixed(lmc_ctx *c, long long *out) {
    LMC_TRY
    if (!c->filmFx.p) throw std::runtime_error("lmc_film_read_fixed: this context's film is the float film (set film_exact before lmc_chains_init)");
    HIP_CHECK(hipSetDevice(c->device));
    SyncLayerSum(c);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(out, c->filmFx.p, c->film.n * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}
int lmc_film_overflow(lmc_ctx *c, long long *n) {
    LMC_TRY
    if (!n) throw std::runtime_error("lmc_film_overflow: n is NULL");
    *n = 0;
    if (!c->filmFx.p) return 0;  // the float film drops nothing
    HIP_CHECK(hipSetDevice(c->device));
    SyncLayerSum(c);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(n, c->filmFx.p + c->film.n, sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}

int lmc_direct_read(lmc_ctx *c, float *rgb) {
    LMC_TRY
    if (c->directFilm.n == 0) throw std::runtime_error("lmc_direct_read before lmc_direct_lighting");
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(rgb, c->directFilm.p, c->directFilm.n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}


int lmc_comm_unique_id(unsigned char *out128) {
    LMC_TRY
    ncclUniqueId id;
    memset(&id, 0, sizeof(id));
    RcclCheck(GetRccl().GetUniqueId(&id), "ncclGetUniqueId");
    memcpy(out128, &id, 128);
    return 0;
    LMC_CATCH(-1)
}

int lmc_comm_init(lmc_ctx *c, int nranks, int rank, const unsigned char *id128) {
    LMC_TRY
    HIP_CHECK(hipSetDevice(c->device));
    if (c->comm) throw std::runtime_error("lmc_comm_init: communicator already initialised");
    // the chain state is laid out for the job's rank count at lmc_chains_init (sharded MLTInit, the gather buffer of the cache pushes:
    // world x stage): a communicator that appears afterwards would make the next cache-filling step gather world stages into a
    // one-stage buffer
    // (a one-rank communicator changes nothing about the layout and is accepted at any time)
    if (c->N > 0 && nranks != 1) throw std::runtime_error("lmc_comm_init after lmc_chains_init: create the communicator first, then initialise the chains");
    if (c->group.size() > 1) throw std::runtime_error("lmc_comm_init: this context is a member of an in-process group");
    if (nranks < 1 || rank < 0 || rank >= nranks) throw std::runtime_error("lmc_comm_init: rank out of range");
    ncclUniqueId id;
    memcpy(&id, id128, 128);
    ncclComm_t comm = nullptr;
    RcclCheck(GetRccl().CommInitRank(&comm, nranks, id, rank), "ncclCommInitRank");
    c->comm = comm;
    c->world = nranks, c->rank = rank;
    c->commScratch.Alloc(LMC_COMM_MAX_SCALARS);
    return 0;
    LMC_CATCH(-1)
}

// Host scalars reduced over the ranks of the job (op 0 sum, 1 max, 2 min), through the job's own communicator on the step stream: what a
// driver needs around the data path (max-over-ranks timing, per-rank figures gathered as a sum of one-hot vectors) without a second
// communication library.  Blocks until the result is back.
int lmc_comm_allreduce_f64(lmc_ctx *c, double *vals, int n, int op) {
    LMC_TRY
    HIP_CHECK(hipSetDevice(c->device));
    if (!c->comm) throw std::runtime_error("lmc_comm_allreduce_f64 before lmc_comm_init");
    if (n < 1 || n > LMC_COMM_MAX_SCALARS) throw std::runtime_error("lmc_comm_allreduce_f64: between 1 and LMC_COMM_MAX_SCALARS values");
    if (op < 0 || op > 2) throw std::runtime_error("lmc_comm_allreduce_f64: op is 0 (sum), 1 (max) or 2 (min)");
    const ncclRedOp_t ops[3] = {ncclSum, ncclMax, ncclMin};
    HIP_CHECK(hipMemcpyAsync(c->commScratch.p, vals, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    RcclCheck(GetRccl().AllReduce(c->commScratch.p, c->commScratch.p, (size_t)n, ncclFloat64, ops[op], (ncclComm_t)c->comm, c->stream), "ncclAllReduce(host scalars)");
    HIP_CHECK(hipMemcpyAsync(vals, c->commScratch.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    return 0;
    LMC_CATCH(-1)
}
// every rank's queued work is done when this returns on any rank: own stream drained, then a one-word all-reduce
int lmc_comm_barrier(lmc_ctx *c) {
    double one = 1.0;
    if (lmc_sync(c) != 0) return -1;
    return lmc_comm_allreduce_f64(c, &one, 1, 0);
}

int lmc_film_allreduce(lmc_ctx *c) {
    LMC_TRY
    HIP_CHECK(hipSetDevice(c->device));
    if (!c->comm) throw std::runtime_error("lmc_film_allreduce before lmc_comm_init");
    if (c->world > 1) RefuseLayered(c, "lmc_film_allreduce", "in this version a layered film is merged inside one process only (lmc_group_film_reduce); nothing was reduced");
    if (c->filmReduced) throw std::runtime_error("lmc_film_allreduce: the film already holds the sum over ranks (a second in-place sum would count every rank's splats again); step or clear the film first");
    c->filmReduced = true;
    // in place on the device film, on the stream the step kernels run on: ordered after the last splat, no host staging
    // (exact mode: the int64 words and, behind them, the overflow counter -- integer sums, the same on every rank whatever the order)
    if (c->filmLayers) RcclCheck(GetRccl().AllReduce(c->filmLayersFx.p, c->filmLayersFx.p, c->filmLayersFx.n, ncclInt64, ncclSum, (ncclComm_t)c->comm, c->stream), "ncclAllReduce(film layers, int64)");  // one rank: the identity
    else if (c->filmFx.p) RcclCheck(GetRccl().AllReduce(c->filmFx.p, c->filmFx.p, c->filmFx.n, ncclInt64, ncclSum, (ncclComm_t)c->comm, c->stream), "ncclAllReduce(film, int64)");
    else
        RcclCheck(GetRccl().AllReduce(c->film.p, c->film.p, c->film.n, ncclFloat32, ncclSum, (ncclComm_t)c->comm, c->stream), "ncclAllReduce(film)");
    // the scalars that normalise the merged image: sum of splat weights (double) -- `normalization` itself is identical on
    // every rank (each runs the same MLTInit), so it is not reduced
    RcclCheck(GetRccl().AllReduce(c->weightSum.p, c->weightSum.p, 1, ncclFloat64, ncclSum, (ncclComm_t)c->comm, c->stream), "ncclAllReduce(weightSum)");
    return 0;
    LMC_CATCH(-1)
}

void *lmc_film_device_ptr(lmc_ctx *c, long long *nFloats) {
    LMC_TRY
    if (nFloats) *nFloats = (long long)c->film.n;
    if (c->filmLayers && c->filmLayersFx.p) {  // "film_layers": the sum of the layers as it stands now; a failed sum returns NULL with lmc_last_error set
        HIP_CHECK(hipSetDevice(c->device));
        SyncLayerSum(c);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    if (c->filmFx.p) return c->filmFx.p;  // exact mode: int64 words, the same count
    return c->film.p;
    LMC_CATCH(nullptr)
}

int lmc_film_clear(lmc_ctx *c) {
    LMC_TRY
    HIP_CHECK(hipMemsetAsync(c->film.p, 0, c->film.n * sizeof(float), c->stream));
    if (c->filmFx.p) HIP_CHECK(hipMemsetAsync(c->filmFx.p, 0, c->filmFx.n * sizeof(long long), c->stream));  // the words and the overflow counter
    if (c->filmLayersFx.p) HIP_CHECK(hipMemsetAsync(c->filmLayersFx.p, 0, c->filmLayersFx.n * sizeof(long long), c->stream));  // "film_layers": every layer
    c->filmReduced = false;
    return 0;
    LMC_CATCH(-1)
}

int lmc_stats(lmc_ctx *c, long long *out8, double *weightSum) {
    LMC_TRY
    HIP_CHECK(hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> h = c->counters.Download();
    for (int k = 0; k < 7; k++) out8[k] = (long long)h[k];
    long long mask = 0;
    for (int d = 2; d <= PSS_MAX_LENGTH; d++)
        if (c->cacheDims[d].ready) mask |= 1ll << d;
    out8[7] = mask;
    if (weightSum) *weightSum = c->weightSum.Download()[0];
    return 0;
    LMC_CATCH(-1)
}

int lmc_relocation_stats(lmc_ctx *c, long long *out4) {
    LMC_TRY
    if (!c->relocate || c->N <= 0) return -1;
    HIP_CHECK(hipStreamSynchronize(c->stream));
    const size_t N = c->N;
    std::vector<float> con(2 * N);
    HIP_CHECK(hipMemcpy(con.data(), c->curContrib.p, 2 * N * sizeof(float), hipMemcpyDeviceToHost));
    long long breaks = 0;
    int prev = -1;
    for (size_t i = 0; i < N; i++) {
        int cc, ll;
        memcpy(&cc, &con[i], 4), memcpy(&ll, &con[N + i], 4);
        const int key = TechniqueKey(cc, ll);
        if (i && key != prev) breaks++;
        prev = key;
    }
    out4[0] = c->relocations, out4[1] = c->relocations ? c->relocCount.Download()[0] : 0, out4[2] = breaks, out4[3] = (long long)N;
    return 0;
    LMC_CATCH(-2)
}

int lmc_resident_stats(lmc_ctx *c, long long *out4, double *kernelMs) {
    LMC_TRY
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    for (auto &e : c->residentEvents) {
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, e.first, e.second));
        c->residentMs += ms;
        (void)hipEventDestroy(e.first), (void)hipEventDestroy(e.second);
    }
    c->residentEvents.clear();
    out4[0] = c->residentLaunches, out4[1] = c->residentGuard.p ? (long long)c->residentGuard.Download()[0] : 0, out4[2] = c->lockSteps, out4[3] = ResidentK(c);
    if (kernelMs) *kernelMs = c->residentMs;
    return 0;
    LMC_CATCH(-1)
}

long long lmc_relocation_skipped(lmc_ctx *c) {
    LMC_TRY
    if (!c->relocate || c->N <= 0) return -1;
    HIP_CHECK(hipStreamSynchronize(c->stream));
    return c->relocations ? c->relocCount.Download()[1] : 0;
    LMC_CATCH(-2)
}

// test probe: where the chains live.  slot_of[chain] and chain_id[slot] as they stand (N ints each, either may be NULL); -1 when relocation is off
int lmc_chain_slots(lmc_ctx *c, int *slot_of, int *chain_id) {
    LMC_TRY
    if (!c->relocate || c->N <= 0) return -1;
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipDeviceSynchronize());  // the relocation runs on the large-step stream: every stream of the context, not just the main one
    if (slot_of) HIP_CHECK(hipMemcpy(slot_of, c->slotOf.p, (size_t)c->N * sizeof(int), hipMemcpyDeviceToHost));
    if (chain_id) HIP_CHECK(hipMemcpy(chain_id, c->chainId.p, (size_t)c->N * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-2)
}

int lmc_chain_summary(lmc_ctx *c, int which, float *out, int stride) {
    LMC_TRY
    HIP_CHECK(hipStreamSynchronize(c->stream));
    const size_t N = c->N;  // current states and init states of THIS rank's chains (the init arrays are per rank since round 3)
    std::vector<float> path = (which == 0 ? c->curPath : c->initPath).Download();
    std::vector<float> path1;
    if (which == 0) path1 = c->pathBuf1.Download();
    std::vector<float> con = (which == 0 ? c->curContrib : c->initContrib).Download();
    std::vector<float> ss = (which == 0 ? c->scoreSum : c->initScoreSum).Download();
    std::vector<int> fl, sidx, nspl;
    if (which == 0) fl = c->flags.Download(), sidx = c->sampleIdx.Download(), nspl = c->curSplatCount.Download();
    std::vector<int> idOf;  // relocation: slot -> chain; the rows go out in chain order
    if (which == 0 && c->relocate) idOf = c->chainId.Download();
    for (size_t i = 0; i < N; i++) {
        float *o = out + (idOf.empty() ? i : (size_t)idOf[i]) * stride;
        memset(o, 0, stride * sizeof(float));
        DPath p;
        float *w = reinterpret_cast<float *>(&p);
        const std::vector<float> &src = (which == 0 && (fl[i] & F_SEL)) ? path1 : path;  // the chain's current buffer
        for (int k = 0; k < DPATH_WORDS; k++) w[k] = src[(size_t)k * N + i];
        int cc, ll;
        memcpy(&cc, &con[0 * N + i], 4), memcpy(&ll, &con[1 * N + i], 4);
        o[0] = which == 0 ? float(fl[i] & F_VALID ? 1 : 0) : 0.f;
        o[1] = (float)cc, o[2] = (float)ll, o[3] = con[7 * N + i], o[4] = con[8 * N + i], o[5] = ss[i], o[6] = p.time;
        if (which == 0) o[7] = (fl[i] & F_GAUSS) ? 1.f : 0.f, o[8] = (fl[i] & F_BUFFERED) ? 1.f : 0.f, o[9] = (float)sidx[i], o[15] = (float)nspl[i];
        o[10] = con[2 * N + i], o[11] = con[3 * N + i], o[12] = con[4 * N + i], o[13] = con[5 * N + i], o[14] = con[6 * N + i];
        // GetPathPss on the host copy (same ordering as device/dpath.h)
        int k = 0;
        float pss[2 * MAXPSS + 16];  // a long state has more primary samples than a row has room for: the row keeps the first stride - 16
        if (p.lgtDepth > 1) {
            pss[k++] = p.lgtPos0, pss[k++] = p.lgtPos1, pss[k++] = p.lgtDir0, pss[k++] = p.lgtDir1;
            for (int d = 0; d < p.lgtCount - 1; d++) pss[k++] = p.lgt[d].rnd0, pss[k++] = p.lgt[d].rnd1;
        }
        if (!(p.lgtDepth > 1 && p.camDepth == 1)) {
            pss[k++] = p.screen0, pss[k++] = p.screen1;
            for (int d = 0; d < p.camCount; d++) {
                if (d == p.camCount - 1) {
                    if (p.lgtDepth == 1) pss[k++] = p.cam[d].dirRnd0, pss[k++] = p.cam[d].dirRnd1;
                    break;
                }
                pss[k++] = p.cam[d].rnd0, pss[k++] = p.cam[d].rnd1;
            }
        }
        for (int q = 0; q < k && 16 + q < stride; q++) o[16 + q] = pss[q];
    }
    return (int)N;
    LMC_CATCH(-1)
}

}  // extern "C"
