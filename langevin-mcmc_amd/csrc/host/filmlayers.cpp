// The layered MLT film (include/lmc_abi.h "Layered MLT film"; dchain.h ChainFilmLayers): what context.cpp asks of the mode around the step path, the readers
// of the layers, and the test probe of the splat routine.  Host logic only: the step kernels are in device/step_*_layers.hip, the probe in device/filmlayers.hip.
#include <cstring>

#include "context.h"

namespace lmc_host {

ChainFilmLayers LayeredFilm(const lmc_ctx *c) {
    return ChainFilmLayers{reinterpret_cast<unsigned long long *>(c->filmLayersFx.p), c->splatLabels.p, c->S.cam.width, c->S.cam.height, c->filmNLayers, c->filmLayers};
}

void LayersCheckInit(const lmc_ctx *c, const char *what) {
    if (!c->filmLayers) return;
    if (!c->filmExact)
        throw std::runtime_error(std::string(what) + ": film_layers = " + std::to_string(c->filmLayers) + " needs film_exact = 1 (the layered MLT film is an exact film; set both before lmc_chains_init)");
    if (c->S.opt.h2mc) throw std::runtime_error(std::string(what) + ": film_layers is not available to an H2MC render in this version (its pipeline's splat launch is not layered)");
    const int D = c->S.opt.maxDepth;
    if (D < 1 || D > 12) throw std::runtime_error(std::string(what) + ": film_layers = " + std::to_string(c->filmLayers) + " needs a maxdepth of 1 .. 12, the scene's is " + std::to_string(D));
    const size_t words = (size_t)c->S.cam.width * c->S.cam.height * 3, n = (size_t)McLayerCount(c->filmLayers, D);
    if (n * words >= (1ull << 31)) throw std::runtime_error(std::string(what) + ": film_layers = " + std::to_string(c->filmLayers) + ": " + std::to_string(n) + " layers of this film size exceed 2^31 words");
}

void LayersAlloc(lmc_ctx *c) {
    if (!c->filmLayers) {
        c->filmLayersFx.Free(), c->splatLabels.Free();
        c->filmNLayers = 0;
        return;
    }
    c->filmNLayers = McLayerCount(c->filmLayers, c->S.opt.maxDepth);
    const size_t words = (size_t)c->filmNLayers * c->film.n + 1;
    try {
        c->filmLayersFx.Alloc(words);  // zeroed
        c->splatLabels.Alloc((size_t)MAXCONTRIB * (size_t)c->N);
        HIP_CHECK(hipStreamSynchronize(nullptr));  // the zeroing runs on the null stream, which the non-blocking side streams of the step do not wait for
    } catch (const std::exception &) {
        (void)hipGetLastError();
        throw std::runtime_error("lmc_chains_init: cannot allocate the " + std::to_string((unsigned long long)(words * sizeof(long long))) + " bytes of the layered film (film_layers = " +
                                 std::to_string(c->filmLayers) + ", " + std::to_string(c->filmNLayers) + " layers)");
    }
}

void SyncLayerSum(lmc_ctx *c) {
    if (!c->filmLayers || !c->filmLayersFx.p) return;
    LaunchMCSumLayers(c->filmLayersFx.p, c->filmFx.p, c->film.n, c->filmNLayers, c->stream);
    HIP_CHECK(hipMemcpyAsync(c->filmFx.p + c->film.n, c->filmLayersFx.p + (size_t)c->filmNLayers * c->film.n, sizeof(long long), hipMemcpyDeviceToDevice, c->stream));
}

void RefuseLayered(const lmc_ctx *c, const char *what, const char *why) {
    if (c->filmLayers) throw std::runtime_error(std::string(what) + ": this context is set to film_layers = " + std::to_string(c->filmLayers) + "; " + why);
}

namespace {
void CheckLayer(const char *what, const lmc_ctx *c, int layer) {
    if (!c->filmLayers || !c->filmLayersFx.p)
        throw std::runtime_error(std::string(what) + ": this context's film is not layered (lmc_set_option \"film_layers\" = 1 or 2, with \"film_exact\" = 1, before lmc_chains_init)");
    if (layer < 0 || layer >= c->filmNLayers)
        throw std::runtime_error(std::string(what) + ": layer " + std::to_string(layer) + " outside [0, " + std::to_string(c->filmNLayers) + ") of the film (film_layers = " + std::to_string(c->filmLayers) + ")");
}
}  // namespace

}  // namespace lmc_host

extern "C" {

int lmc_film_layer_info(lmc_ctx *c, int *mode, int *nLayers, int *cl, int cap) {
    LMC_TRY
    const bool have = c->filmLayers != 0 && c->filmLayersFx.p != nullptr;
    if (mode) *mode = have ? c->filmLayers : 0;
    if (nLayers) *nLayers = have ? c->filmNLayers : 0;
    if (!have || !cl) return 0;
    int k = 0;
    for (int L = 1; k < c->filmNLayers; L++)
        for (int l = 0; l <= (c->filmLayers == 2 ? L : 0) && k < c->filmNLayers; l++, k++)
            if (k < cap) cl[2 * k] = c->filmLayers == 2 ? L + 1 - l : L, cl[2 * k + 1] = c->filmLayers == 2 ? l : -1;
    return 0;
    LMC_CATCH(-1)
}

int lmc_film_read_layer(lmc_ctx *c, int layer, float *rgb) {
    LMC_TRY
    CheckLayer("lmc_film_read_layer", c, layer);
    if (!rgb) throw std::runtime_error("lmc_film_read_layer: rgb is NULL");
    HIP_CHECK(hipSetDevice(c->device));
    DevBuf<float> conv;  // converted on the device like lmc_film_read, float(double(q) * 2^-32)
    conv.Alloc(c->film.n, false);
    LaunchFilmFixedToFloat(c->filmLayersFx.p + (size_t)layer * c->film.n, conv.p, c->film.n, c->stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(rgb, conv.p, c->film.n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}

int lmc_film_read_layer_fixed(lmc_ctx *c, int layer, long long *words) {
    LMC_TRY
    CheckLayer("lmc_film_read_layer_fixed", c, layer);
    if (!words) throw std::runtime_error("lmc_film_read_layer_fixed: words is NULL");
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipMemcpy(words, c->filmLayersFx.p + (size_t)layer * c->film.n, c->film.n * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}

// test probe: n labelled splats through the device's layered splat routine into a fresh film of McLayerCount(mode, D) layers.  out_fixed: every layer's words,
// *overflow: the film's overflow word, *outside: the finite splats whose technique is outside the table (they are part of *overflow as well)
int lmc_film_layer_splat_probe(int W, int H, int mode, int D, int n, const float *screen_xy, const float *rgb, const int *cl, long long *out_fixed, long long *overflow, long long *outside) {
    LMC_TRY
    if (mode != 1 && mode != 2) throw std::runtime_error("lmc_film_layer_splat_probe: mode is 1 (by path length) or 2 (by technique)");
    if (D < 1 || D > 12) throw std::runtime_error("lmc_film_layer_splat_probe: D is 1 .. 12");
    if (W <= 0 || H <= 0 || n < 0 || (long long)W * H > (1ll << 20)) throw std::runtime_error("lmc_film_layer_splat_probe: bad film size or splat count");
    if (n > 0 && (!screen_xy || !rgb || !cl)) throw std::runtime_error("lmc_film_layer_splat_probe: screen_xy, rgb or cl is NULL");
    const int nLayers = McLayerCount(mode, D);
    const size_t words = (size_t)W * H * 3, total = (size_t)nLayers * words;
    DevBuf<long long> dFx;
    DevBuf<unsigned long long> dOutside;
    DevBuf<float> dXY, dRGB;
    DevBuf<int> dCL;
    dFx.Alloc(total + 1), dOutside.Alloc(1);
    if (n > 0) {
        dXY.Alloc(2 * (size_t)n, false), dRGB.Alloc(3 * (size_t)n, false), dCL.Alloc(2 * (size_t)n, false);
        HIP_CHECK(hipMemcpy(dXY.p, screen_xy, 2 * (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dRGB.p, rgb, 3 * (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dCL.p, cl, 2 * (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    }
    LaunchFilmLayerSplatProbe(ChainFilmLayers{reinterpret_cast<unsigned long long *>(dFx.p), nullptr, W, H, nLayers, mode}, n, dXY.p, dRGB.p, dCL.p, dOutside.p, 0);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    const std::vector<long long> h = dFx.Download();
    if (out_fixed) memcpy(out_fixed, h.data(), total * sizeof(long long));
    if (overflow) *overflow = h[total];
    if (outside) *outside = (long long)dOutside.Download()[0];
    return 0;
    LMC_CATCH(-1)
}

}  // extern "C"
