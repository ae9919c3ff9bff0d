// The passes beside the Markov chains (include/lmc_abi.h): direct lighting and the path-traced cross-checks into the direct film, the mc integrator
// into the mc film (float or exact; host/mcfilm.h has the exact film's coverage, chunking and file format).  Host logic only: the kernels are in
// device/kernels.hip and device/mc.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/lmc_abi.h"
#include "../device/kernels.h"
#include "context.h"
#include "hostutil.h"
#include "mcfilm.h"
#include "scene.h"

// DirectLighting(scene, directBuffer), direct.cpp:4-54 (skipped when mindepth > 2 or maxdepth < 1, :6-8)
static int PathTracePass(lmc_ctx *c, int spp, int minDepth, int maxDepth);
extern "C" {
int lmc_direct_lighting(lmc_ctx *c, int directSpp) {
    if (c->S.opt.minDepth > 2 || c->S.opt.maxDepth < 1) directSpp = 0;
    return PathTracePass(c, directSpp, std::min(c->S.opt.minDepth, 2), std::min(c->S.opt.maxDepth, 2));
}
// GeneratePath with the scene's own depth range: the reference's "mc" integrator kernel (pathtrace.cpp uses the same
// generator); here a cross-check of the MLT result, not a product path
int lmc_path_trace(lmc_ctx *c, int spp) { return PathTracePass(c, spp, c->S.opt.minDepth, c->S.opt.maxDepth); }
// plain Monte Carlo over GeneratePathBidir samples (paths of length >= 3), `spp` samples per pixel on average; result
// (already scaled to radiance) through lmc_direct_read.  Cross-check estimator for tests / DESIGN.md, not a product path.
int lmc_bidir_mc(lmc_ctx *c, int spp) {
    LMC_TRY
    HIP_CHECK(hipSetDevice(c->device));
    const int W = c->S.cam.width, H = c->S.cam.height;
    c->directFilm.Alloc((size_t)W * H * 3);
    const int nThreads = 65536;
    const long long total = (long long)spp * W * H;
    const int per = (int)((total + nThreads - 1) / nThreads);
    DevBuf<uint32_t> tab;
    DevBuf<float> contrib;
    tab.Alloc((size_t)nThreads * 64, false), contrib.Alloc((size_t)nThreads * MAXCONTRIB * CONTRIB_WORDS, false);
    Film film{c->directFilm.p, W, H};
    LaunchBidirMC(c->S, film, nThreads, per, tab.p, contrib.p, c->stream);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    std::vector<float> h = c->directFilm.Download();
    const float scale = (float)((double)W * H / ((double)per * nThreads));
    for (auto &v : h) v *= scale;
    HIP_CHECK(hipMemcpy(c->directFilm.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
    LMC_CATCH(-1)
}
}  // extern "C"
static int PathTracePass(lmc_ctx *c, int directSpp, int minDepth, int maxDepth) {
    LMC_TRY
    HIP_CHECK(hipSetDevice(c->device));
    const int W = c->S.cam.width, H = c->S.cam.height;
    c->directFilm.Alloc((size_t)W * H * 3);
    if (directSpp <= 0) return 0;
    const int nTiles = ((W + 15) / 16) * ((H + 15) / 16);
    DevBuf<uint32_t> tab;
    tab.Alloc((size_t)nTiles * 64, false);
    Film film{c->directFilm.p, W, H};
    const char *e = getenv("LMC_DIRECT_WAVE");  // =0: the one-thread-per-tile kernel (A/B, and the checker of the wave kernel)
    LaunchDirect(c->S, film, directSpp, minDepth, maxDepth, c->bvhDepth, !e || atoi(e) != 0, tab.p, c->stream);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipGetLastError());
    return 0;
    LMC_CATCH(-1)
}

// The mc integrator (PathTrace, pathtrace.cpp:14-78; device/mc.hip): stream ids [begin, end) of nTiles * spp into the MC film.
// Generator, depth range and seed offset are the scene's (<dpt bidirectional / mindepth / maxdepth / seedoffset>).
// Float mode: the film is cleared and every contribution added as contrib / spp.  Exact mode ("mc_film_exact", INTEGRATION.md "Exact mc film"): the film is
// the integer sum of the unweighted contributions, knows which stream ids it holds (host/mcfilm.h McCoverage) and is divided by spp when it is read, so
// calls can add to it (lmc_mc_accumulate), members' films can be summed in any order (lmc_group_mc_render) and a file can carry it (lmc_mc_save / _load).
// Either mode runs a call as launches of at most "mc_launch_streams" stream ids on the context's stream.
// Layered ("mc_layers", INTEGRATION.md "Layered mc film"): the launches add to mcLayersF / mcLayersFx, one film per path length or technique, and every call ends
// with the sum of the layers in mcFilm / mcFilmFx (overflow word included), so whatever reads the film below reads the total and needs no second form.
namespace {
long long McTiles(const lmc_ctx *c) { return (long long)((c->S.cam.width + 15) / 16) * ((c->S.cam.height + 15) / 16); }
size_t McWords(const lmc_ctx *c) { return (size_t)c->S.cam.width * c->S.cam.height * 3; }

void McCheckRange(const char *what, lmc_ctx *c, int spp, long long &begin, long long &end) {
    if (spp < 1) throw std::runtime_error(std::string(what) + ": spp >= 1 expected");
    const long long total = McTiles(c) * spp;
    if (end == -1) end = total;
    if (begin < 0 || begin > end || end > total)
        throw std::runtime_error(std::string(what) + ": stream range [" + std::to_string(begin) + ", " + std::to_string(end) + ") outside [0, " + std::to_string(total) + ")");
}

// the film of a context set to layer mode `mode` (the option's value): the layer count, the buffer allocated if its size changed, and cleared
void McStartLayers(const char *what, lmc_ctx *c, int mode, bool exact) {
    c->mcLayerMode = 0, c->mcNLayers = 0;  // (a refusal below leaves an unlayered context)
    if (mode == 0) {
        c->mcLayersF.Free(), c->mcLayersFx.Free();
        return;
    }
    const int D = c->S.opt.maxDepth;
    if (D < 1 || D > 12) throw std::runtime_error(std::string(what) + ": mc_layers = " + std::to_string(mode) + " needs a maxdepth of 1 .. 12, the scene's is " + std::to_string(D));
    const int n = McLayerCount(mode, D);
    if ((unsigned long long)n * c->S.cam.width * c->S.cam.height * 3 > 0x7fffffffull)
        throw std::runtime_error(std::string(what) + ": mc_layers = " + std::to_string(mode) + ": " + std::to_string(n) + " layers of this film size exceed 2^31 words");
    const size_t words = (size_t)n * McWords(c) + (exact ? 1 : 0), bytes = words * (exact ? sizeof(long long) : sizeof(float));
    try {
        if (exact) {
            c->mcLayersF.Free();
            if (c->mcLayersFx.n != words) c->mcLayersFx.Alloc(words, false);
        } else {
            c->mcLayersFx.Free();
            if (c->mcLayersF.n != words) c->mcLayersF.Alloc(words, false);
        }
    } catch (const std::exception &e) {
        throw std::runtime_error(std::string(what) + ": cannot allocate the " + std::to_string(bytes) + " bytes of the layered mc film (mc_layers = " + std::to_string(mode) + ", " +
                                 std::to_string(n) + " layers): " + e.what());
    }
    HIP_CHECK(hipMemsetAsync(exact ? (void *)c->mcLayersFx.p : (void *)c->mcLayersF.p, 0, bytes, c->stream));
    c->mcLayerMode = mode, c->mcNLayers = n;
}

// the launches of one call: [begin, end) in chunks (mcfilm.h McChunks), one table scratch sized for the largest of them, one wait at the end; a layered
// film's launches go to the layers, and their sum is made before the wait
void McRunLaunches(lmc_ctx *c, Film film, int spp, long long begin, long long end) {
    const std::vector<lmc::McRange> chunks = lmc::McChunks(begin, end, McTiles(c), c->mcLaunchStreams);
    long long maxThreads = 0;
    for (const lmc::McRange &r : chunks) maxThreads = std::max(maxThreads, MCThreads(c->S, r.first, r.second));
    DevBuf<uint32_t> tab;  // written only by a stream that ticks (once per 2^32 draws)
    tab.Alloc((size_t)((maxThreads + 63) / 64 * 64) * 64, false);
    const bool exact = (film.H & FILM_EXACT) != 0;
    if (c->mcLayerMode) film.rgb = exact ? reinterpret_cast<float *>(c->mcLayersFx.p) : c->mcLayersF.p;
    for (const lmc::McRange &r : chunks)
        LaunchMC(c->S, film, c->mcLayerMode, c->mcNLayers, c->scene->options.bidirectional, spp, c->S.opt.minDepth, c->S.opt.maxDepth, r.first, r.second, tab.p, c->mcCounters.p,
                 c->stream);
    if (c->mcLayerMode && exact) {
        LaunchMCSumLayers(c->mcLayersFx.p, c->mcFilmFx.p, McWords(c), c->mcNLayers, c->stream);
        HIP_CHECK(hipMemcpyAsync(c->mcFilmFx.p + McWords(c), c->mcLayersFx.p + (size_t)c->mcNLayers * McWords(c), sizeof(long long), hipMemcpyDeviceToDevice, c->stream));
    } else if (c->mcLayerMode) {
        LaunchMCSumLayers(c->mcLayersF.p, c->mcFilm.p, McWords(c), c->mcNLayers, c->stream);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));
    c->mcLaunches = (int)chunks.size();
}

// an empty exact film: words, overflow word, counters and coverage cleared; layered as the option says
void McStartExact(const char *what, lmc_ctx *c) {
    McStartLayers(what, c, c->mcLayersOpt, true);
    if (c->mcFilmFx.n != McWords(c) + 1) c->mcFilmFx.Alloc(McWords(c) + 1, false);
    if (c->mcCounters.n != 2) c->mcCounters.Alloc(2, false);
    HIP_CHECK(hipMemsetAsync(c->mcFilmFx.p, 0, c->mcFilmFx.n * sizeof(long long), c->stream));
    HIP_CHECK(hipMemsetAsync(c->mcCounters.p, 0, 2 * sizeof(unsigned long long), c->stream));
    c->mcCoverage.Clear();
    c->mcFilmIsExact = true;
    c->mcDivisor = 0;
}

// adds [begin, end) to the exact film the context holds; refused, the film untouched, if the range would count a sample twice
void McAccumulate(const char *what, lmc_ctx *c, int spp, long long begin, long long end) {
    const long long total = McTiles(c) * spp;
    if (c->mcCoverage.End() > total)
        throw std::runtime_error(std::string(what) + ": the film holds stream ids up to " + std::to_string(c->mcCoverage.End()) + ", beyond the " + std::to_string(total) +
                                 " of " + std::to_string(spp) + " spp");
    if (c->mcCoverage.Overlaps(begin, end))
        throw std::runtime_error(std::string(what) + ": stream range [" + std::to_string(begin) + ", " + std::to_string(end) +
                                 ") overlaps what the film already holds (its samples would be counted twice); the film is unchanged");
    McRunLaunches(c, FilmFx(c->mcFilmFx.p, c->S.cam.width, c->S.cam.height), spp, begin, end);  // (a layered film: into its layers, mcFilmFx their sum)
    c->mcCoverage.Add(begin, end);
    c->mcDivisor = spp;
}

lmc::McFileHeader McHeaderOf(lmc_ctx *c) {
    lmc::McFileHeader H;
    if (!c->sceneHash) c->sceneHash = HashSceneFiles(*c->scene);
    const lmc::DptOptions &o = c->scene->options;
    H.sceneHash = c->sceneHash;
    H.forceDiffuse = c->forceDiffuse, H.width = c->S.cam.width, H.height = c->S.cam.height, H.minDepth = o.minDepth, H.maxDepth = o.maxDepth, H.seedOffset = o.seedOffset;
    H.bidirectional = o.bidirectional ? 1 : 0;
    H.nTiles = McTiles(c);
    return H;
}
}  // namespace

extern "C" {

int lmc_mc_render(lmc_ctx *c, int spp, long long streamBegin, long long streamEnd) {
    LMC_TRY
    HIP_CHECK(hipSetDevice(c->device));
    McCheckRange("lmc_mc_render", c, spp, streamBegin, streamEnd);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (c->mcExactOpt) {
        McStartExact("lmc_mc_render", c);
        McAccumulate("lmc_mc_render", c, spp, streamBegin, streamEnd);
        return 0;
    }
    const int W = c->S.cam.width, H = c->S.cam.height;
    McStartLayers("lmc_mc_render", c, c->mcLayersOpt, false);
    c->mcFilmIsExact = false;
    c->mcCoverage.Clear();
    if (c->mcFilm.n != (size_t)W * H * 3) c->mcFilm.Alloc((size_t)W * H * 3, false);
    if (c->mcCounters.n != 2) c->mcCounters.Alloc(2, false);
    HIP_CHECK(hipMemsetAsync(c->mcFilm.p, 0, c->mcFilm.n * sizeof(float), c->stream));
    HIP_CHECK(hipMemsetAsync(c->mcCounters.p, 0, 2 * sizeof(unsigned long long), c->stream));
    McRunLaunches(c, Film{c->mcFilm.p, W, H}, spp, streamBegin, streamEnd);
    return 0;
    LMC_CATCH(-1)
}
int lmc_mc_accumulate(lmc_ctx *c, int spp, long long streamBegin, long long streamEnd) {
    LMC_TRY
    if (!c->mcExactOpt) throw std::runtime_error("lmc_mc_accumulate: the mc film is in float mode; only the exact film (lmc_set_option \"mc_film_exact\" = 1) can be added to");
    HIP_CHECK(hipSetDevice(c->device));
    McCheckRange("lmc_mc_accumulate", c, spp, streamBegin, streamEnd);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (c->mcFilmIsExact && c->mcLayerMode != c->mcLayersOpt)
        throw std::runtime_error("lmc_mc_accumulate: the film the context holds was rendered with mc_layers = " + std::to_string(c->mcLayerMode) + ", the option is now mc_layers = " +
                                 std::to_string(c->mcLayersOpt) + "; a film takes more samples in its own layer mode only, and is unchanged");
    if (!c->mcFilmIsExact) McStartExact("lmc_mc_accumulate", c);  // no exact film yet: an empty one
    McAccumulate("lmc_mc_accumulate", c, spp, streamBegin, streamEnd);
    return 0;
    LMC_CATCH(-1)
}
int lmc_mc_coverage(lmc_ctx *c, long long *ranges, int cap) {
    LMC_TRY
    if (!c->mcFilmIsExact) return 0;
    const std::vector<lmc::McRange> &r = c->mcCoverage.ranges;
    for (int k = 0; k < (int)r.size() && k < cap; k++) ranges[2 * k] = r[k].first, ranges[2 * k + 1] = r[k].second;
    return (int)r.size();
    LMC_CATCH(-1)
}
int lmc_mc_read(lmc_ctx *c, float *rgb) {
    LMC_TRY
    if (c->mcFilmIsExact ? c->mcFilmFx.n == 0 || c->mcDivisor < 1 : c->mcFilm.n == 0) throw std::runtime_error("lmc_mc_read before lmc_mc_render");
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (c->mcFilmIsExact) {  // converted on the device, float(double(q) * 2^-32 / double(spp))
        if (c->mcFilm.n != McWords(c)) c->mcFilm.Alloc(McWords(c), false);
        LaunchMCFixedToFloat(c->mcFilmFx.p, c->mcFilm.p, c->mcFilm.n, c->mcDivisor, c->stream);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    HIP_CHECK(hipMemcpy(rgb, c->mcFilm.p, c->mcFilm.n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}
int lmc_mc_read_fixed(lmc_ctx *c, long long *words) {
    LMC_TRY
    if (!c->mcFilmIsExact || c->mcFilmFx.n == 0) throw std::runtime_error("lmc_mc_read_fixed: the mc film is in float mode (lmc_set_option \"mc_film_exact\" = 1 before lmc_mc_render)");
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(words, c->mcFilmFx.p, McWords(c) * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}
int lmc_mc_overflow(lmc_ctx *c, long long *n) {
    LMC_TRY
    *n = 0;
    if (!c->mcFilmIsExact || c->mcFilmFx.n == 0) return 0;
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(n, c->mcFilmFx.p + McWords(c), sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}
int lmc_mc_stats(lmc_ctx *c, long long *out2) {
    LMC_TRY
    out2[0] = out2[1] = 0;
    if (c->mcCounters.n != 2) return 0;
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    const std::vector<unsigned long long> v = c->mcCounters.Download();
    out2[0] = (long long)v[0], out2[1] = (long long)v[1];
    return 0;
    LMC_CATCH(-1)
}

// The layers of the film the context holds (include/lmc_abi.h "Layered mc film")
int lmc_mc_layer_info(lmc_ctx *c, int *mode, int *nLayers, int *cl, int cap) {
    LMC_TRY
    const bool have = c->mcLayerMode != 0 && (c->mcFilmIsExact ? c->mcLayersFx.n != 0 : c->mcLayersF.n != 0);
    if (mode) *mode = have ? c->mcLayerMode : 0;
    if (nLayers) *nLayers = have ? c->mcNLayers : 0;
    if (!have || !cl) return 0;
    int k = 0;
    for (int L = 1; k < c->mcNLayers; L++)
        for (int l = 0; l <= (c->mcLayerMode == 2 ? L : 0) && k < c->mcNLayers; l++, k++)
            if (k < cap) cl[2 * k] = c->mcLayerMode == 2 ? L + 1 - l : L, cl[2 * k + 1] = c->mcLayerMode == 2 ? l : -1;
    return 0;
    LMC_CATCH(-1)
}
static void McCheckLayer(const char *what, lmc_ctx *c, int layer) {
    if (c->mcLayerMode == 0 || c->mcNLayers == 0) throw std::runtime_error(std::string(what) + ": the context holds no layered mc film (lmc_set_option \"mc_layers\" = 1 or 2 before lmc_mc_render)");
    if (layer < 0 || layer >= c->mcNLayers)
        throw std::runtime_error(std::string(what) + ": layer " + std::to_string(layer) + " outside [0, " + std::to_string(c->mcNLayers) + ") of the film (mc_layers = " + std::to_string(c->mcLayerMode) + ")");
}
int lmc_mc_read_layer(lmc_ctx *c, int layer, float *rgb) {
    LMC_TRY
    McCheckLayer("lmc_mc_read_layer", c, layer);
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    const size_t words = McWords(c);
    if (!c->mcFilmIsExact) {
        HIP_CHECK(hipMemcpy(rgb, c->mcLayersF.p + (size_t)layer * words, words * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    }
    if (c->mcDivisor < 1) throw std::runtime_error("lmc_mc_read_layer before lmc_mc_render");
    DevBuf<float> conv;  // converted on the device like lmc_mc_read, float(double(q) * 2^-32 / double(spp))
    conv.Alloc(words, false);
    LaunchMCFixedToFloat(c->mcLayersFx.p + (size_t)layer * words, conv.p, words, c->mcDivisor, c->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(rgb, conv.p, words * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}
int lmc_mc_read_layer_fixed(lmc_ctx *c, int layer, long long *out) {
    LMC_TRY
    if (!c->mcFilmIsExact) throw std::runtime_error("lmc_mc_read_layer_fixed: the mc film is in float mode (lmc_set_option \"mc_film_exact\" = 1 before lmc_mc_render)");
    McCheckLayer("lmc_mc_read_layer_fixed", c, layer);
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(out, c->mcLayersFx.p + (size_t)layer * McWords(c), McWords(c) * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}

}  // extern "C"

// [begin, end) split at begin + (end - begin) * k / n, the shards rendered concurrently (one host thread per member), then member 0's film += member k's for
// k = 1 .. n - 1 in that order on member 0's device: int64 words in exact mode, floats in float mode (the order a host loop over the members would add in)
// lmc_group_mc_accumulate: the same, but member 0 adds its shard to the exact film it holds (the others render theirs into cleared films), so member 0
// ends with what it held plus the whole range
static int GroupMcRender(const char *what_, bool accumulate, lmc_ctx **ctxs, int n, int spp, long long streamBegin, long long streamEnd) {
    LMC_TRY
    const std::string what(what_);
    if (n < 1 || !ctxs) throw std::runtime_error(what + ": empty group");
    std::vector<lmc_ctx *> g(ctxs, ctxs + n);
    for (int r = 0; r < n; r++) {
        if (!g[r]) throw std::runtime_error(what + ": null member");
        for (int q = 0; q < r; q++)
            if (g[q] == g[r]) throw std::runtime_error(what + ": a context is listed twice (a device may be, through a context of its own)");
        if (g[r]->mcLayersOpt != 0 || (accumulate && r == 0 && g[0]->mcFilmIsExact && g[0]->mcLayerMode != 0))
            throw std::runtime_error(what + ": member " + std::to_string(r) + " is set to mc_layers = " + std::to_string(g[r]->mcLayersOpt ? g[r]->mcLayersOpt : g[r]->mcLayerMode) +
                                     "; in this version a layered mc film is rendered by one context, not by a group (nothing was rendered)");
        if (g[r]->mcExactOpt != g[0]->mcExactOpt)
            throw std::runtime_error(what + ": the members differ in mc_film_exact (member 0: " + std::to_string((int)g[0]->mcExactOpt) + ", member " + std::to_string(r) + ": " +
                                     std::to_string((int)g[r]->mcExactOpt) + "); a group's films are summed in one format");
        if (g[r]->S.cam.width != g[0]->S.cam.width || g[r]->S.cam.height != g[0]->S.cam.height) throw std::runtime_error(what + ": the members differ in film size");
    }
    McCheckRange(what_, g[0], spp, streamBegin, streamEnd);
    if (accumulate && !g[0]->mcExactOpt) throw std::runtime_error(what + ": the mc film is in float mode; only the exact film (lmc_set_option \"mc_film_exact\" = 1) can be added to");
    if (accumulate && g[0]->mcFilmIsExact && g[0]->mcCoverage.Overlaps(streamBegin, streamEnd))
        throw std::runtime_error(what + ": stream range [" + std::to_string(streamBegin) + ", " + std::to_string(streamEnd) +
                                 ") overlaps what member 0's film already holds (its samples would be counted twice); the film is unchanged");
    const long long len = streamEnd - streamBegin;
    std::vector<int> rc(n, 0);
    std::vector<std::string> err(n);  // the last error is per thread
    std::vector<std::thread> th;
    for (int k = 0; k < n; k++)
        th.emplace_back([&, k] {
            const long long b = streamBegin + len * k / n, e = streamBegin + len * (k + 1) / n;
            rc[k] = accumulate && k == 0 ? lmc_mc_accumulate(g[k], spp, b, e) : lmc_mc_render(g[k], spp, b, e);
            if (rc[k] != 0) err[k] = lmc_last_error();
        });
    for (std::thread &t : th) t.join();
    for (int k = 0; k < n; k++)
        if (rc[k] != 0) throw std::runtime_error(what + ": member " + std::to_string(k) + ": " + err[k]);
    lmc_ctx *c = g[0];
    const bool exact = c->mcFilmIsExact;
    const size_t words = exact ? McWords(c) + 1 : McWords(c), bytes = words * (exact ? sizeof(long long) : sizeof(float));
    if (n > 1) {
        HIP_CHECK(hipSetDevice(c->device));
        DevBuf<unsigned char> stage;
        DevBuf<long long> counterStage;
        stage.Alloc(bytes, false), counterStage.Alloc(2, false);
        for (int k = 1; k < n; k++) {  // (every member's stream is idle: lmc_mc_render waits for its launches)
            HIP_CHECK(hipMemcpyPeerAsync(stage.p, c->device, exact ? (const void *)g[k]->mcFilmFx.p : (const void *)g[k]->mcFilm.p, g[k]->device, bytes, c->stream));
            HIP_CHECK(hipMemcpyPeerAsync(counterStage.p, c->device, g[k]->mcCounters.p, g[k]->device, 2 * sizeof(long long), c->stream));
            if (exact) LaunchAddIntoI64(c->mcFilmFx.p, reinterpret_cast<const long long *>(stage.p), words, c->stream);
            else
                LaunchAddInto(c->mcFilm.p, reinterpret_cast<const float *>(stage.p), words, c->stream);
            LaunchAddIntoI64(reinterpret_cast<long long *>(c->mcCounters.p), counterStage.p, 2, c->stream);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(c->stream));
        for (int k = 1; k < n; k++) {  // member 0 holds the whole; the others are left cleared
            lmc_ctx *m = g[k];
            if (exact)
                for (const lmc::McRange &r : m->mcCoverage.ranges) c->mcCoverage.Add(r.first, r.second);
            HIP_CHECK(hipSetDevice(m->device));
            if (exact) HIP_CHECK(hipMemsetAsync(m->mcFilmFx.p, 0, m->mcFilmFx.n * sizeof(long long), m->stream));
            else
                HIP_CHECK(hipMemsetAsync(m->mcFilm.p, 0, m->mcFilm.n * sizeof(float), m->stream));
            HIP_CHECK(hipMemsetAsync(m->mcCounters.p, 0, 2 * sizeof(unsigned long long), m->stream));
            HIP_CHECK(hipStreamSynchronize(m->stream));
            m->mcCoverage.Clear();
        }
        HIP_CHECK(hipSetDevice(c->device));
    }
    return 0;
    LMC_CATCH(-1)
}

extern "C" {

int lmc_group_mc_render(lmc_ctx **ctxs, int n, int spp, long long streamBegin, long long streamEnd) {
    return GroupMcRender("lmc_group_mc_render", false, ctxs, n, spp, streamBegin, streamEnd);
}
int lmc_group_mc_accumulate(lmc_ctx **ctxs, int n, int spp, long long streamBegin, long long streamEnd) {
    return GroupMcRender("lmc_group_mc_accumulate", true, ctxs, n, spp, streamBegin, streamEnd);
}

// The exact mc film as a file (host/mcfilm.h has the layout): the fingerprint of what the film was rendered from, its divisor, counters and coverage, the words.
int lmc_mc_save(lmc_ctx *c, const char *path) {
    LMC_TRY
    if (!path) throw std::runtime_error("lmc_mc_save: no path");
    if (c->mcLayerMode != 0)
        throw std::runtime_error("lmc_mc_save: the mc film is layered (mc_layers = " + std::to_string(c->mcLayerMode) + "); in this version a state file holds an unlayered film only (nothing was written)");
    if (!c->mcFilmIsExact || c->mcFilmFx.n == 0) throw std::runtime_error("lmc_mc_save: the context holds no exact mc film (lmc_set_option \"mc_film_exact\" = 1 before lmc_mc_render)");
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    lmc::McFileHeader H = McHeaderOf(c);
    const std::vector<long long> words = c->mcFilmFx.Download();
    const std::vector<unsigned long long> counters = c->mcCounters.Download();
    H.spp = c->mcDivisor, H.paths = (int64_t)counters[0], H.contributions = (int64_t)counters[1], H.overflow = words[McWords(c)];
    H.coverage = c->mcCoverage;
    lmc::McFileWrite(path, H, words.data());
    return 0;
    LMC_CATCH(-1)
}
int lmc_mc_load(lmc_ctx *c, const char *path) {
    LMC_TRY
    if (!path) throw std::runtime_error("lmc_mc_load: no path");
    if (c->mcLayersOpt != 0)
        throw std::runtime_error("lmc_mc_load: the context is set to mc_layers = " + std::to_string(c->mcLayersOpt) + "; in this version a state file holds an unlayered film only (the context is unchanged)");
    if (!c->mcExactOpt) throw std::runtime_error("lmc_mc_load: the mc film is in float mode; a state file holds an exact film (lmc_set_option \"mc_film_exact\" = 1)");
    std::vector<long long> words;
    const lmc::McFileHeader F = lmc::McFileRead(path, &words);
    if (const char *field = lmc::McFileMismatch(F, McHeaderOf(c)))
        throw std::runtime_error(std::string("lmc_mc_load: ") + path + " was written for another render: it differs in " + field);
    if (F.spp < 1 || F.spp > 0x7fffffff || F.coverage.End() > F.nTiles * F.spp) throw std::runtime_error(std::string("lmc_mc_load: ") + path + " has an inconsistent header (spp / coverage)");
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    words.push_back(F.overflow);
    const unsigned long long counters[2] = {(unsigned long long)F.paths, (unsigned long long)F.contributions};
    McStartExact("lmc_mc_load", c);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(c->mcFilmFx.p, words.data(), words.size() * sizeof(long long), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(c->mcCounters.p, counters, sizeof(counters), hipMemcpyHostToDevice));
    c->mcCoverage = F.coverage;
    c->mcDivisor = (int)F.spp;
    return 0;
    LMC_CATCH(-1)
}
// host only: the header of a state file as one JSON document (lmc_scene_dump's convention: at most cap - 1 characters + NUL, returns the full length, -1 on error)
long long lmc_mc_file_info(const char *path, char *out, long long cap) {
    LMC_TRY
    if (!path) throw std::runtime_error("lmc_mc_file_info: no path");
    const std::string j = lmc::McFileJson(lmc::McFileRead(path, nullptr));
    if (out && cap > 0) {
        const size_t n = std::min<size_t>(j.size(), (size_t)cap - 1);
        memcpy(out, j.data(), n);
        out[n] = 0;
    }
    return (long long)j.size();
    LMC_CATCH(-1)
}

}  // extern "C"
