// Test helper: the oracle side of the LAYERED exact mc film (lmc_set_option "mc_layers"; INTEGRATION.md "Layered mc film").  Built by
// tests/test_mc_layers_abi.py against oracle/liblmc_oracle.so the way tests/test_mc_exact_abi.py builds mc_oracle_fx.cpp.  It is that helper's stream loop
// (the product's stream layout, the ids [begin, end) of nTiles * spp) over an int64 film of nLayers * H * W * 3 words; a contribution goes to the
// layer of SubpathContrib::camDepth / lightDepth = (c, l), path length L = c + l - 1:
//   mode 1 (by length)     D = maxdepth layers, layer L - 1
//   mode 2 (by technique)  D (D + 3) / 2 layers, layer (L - 1)(L + 2) / 2 + l for L = 1 .. D, l = 0 .. L
// (the unidirectional generator labels its contributions (2 + camDepth, 0 | 1)).  The exact mode's rules per contribution are mc_oracle_fx.cpp's.
// out: nLayers*H*W*3 int64 words (accumulated into, not cleared); counts: [paths traced, contributions counted, contributions dropped by the range
// rule, contributions outside the table (counted, not written)].  Returns the number of layers, -1 on error.
#include <cmath>
#include <cstring>
#include <string>

#include "../../oracle/render.h"

using namespace orc;

namespace {

constexpr float kLimit = 1073741824.0f;  // 2^30
constexpr double kScale = 4294967296.0;  // 2^32

int LayerCount(int mode, int D) { return mode == 1 ? D : D * (D + 3) / 2; }

struct McLayersFx {
    long long *words;
    int W, H, mode, D;
    long long splats = 0, dropped = 0, outside = 0;
    void Splat(const std::vector<SubpathContrib> &cs) {
        for (const SubpathContrib &c : cs) {
            if (Luminance(c.contrib) <= Float(1e-10)) continue;
            const Vector3 v = c.contrib;
            if (!v.allFinite()) continue;
            splats++;
            if (std::fabs((float)v[0]) >= kLimit || std::fabs((float)v[1]) >= kLimit || std::fabs((float)v[2]) >= kLimit) {
                dropped++;
                continue;
            }
            const int cd = c.camDepth, ld = c.lightDepth, L = cd + ld - 1;
            if (cd < 1 || ld < 0 || L < 1 || L > D) {
                outside++;
                continue;
            }
            const int layer = mode == 1 ? L - 1 : (L - 1) * (L + 2) / 2 + ld;
            const int ix = Clamp(int(c.screenPos[0] * W), 0, W - 1), iy = Clamp(int(c.screenPos[1] * H), 0, H - 1);  // image.h:66-77
            long long *px = words + (((size_t)layer * H + iy) * W + ix) * 3;
            for (int i = 0; i < 3; i++) px[i] += std::llrint((double)(float)v[i] * kScale);
        }
    }
};

}  // namespace

extern "C" int mc_oracle_layers_fx_count(int mode, int maxDepth) { return LayerCount(mode, maxDepth); }

extern "C" int mc_oracle_layers_fx_render(const char *xml, int forceDiffuse, int maxDepth, int width, int height, int seedOffset, int minDepth, int bidir, int spp,
                                          long long begin, long long end, int mode, int layerCap, long long *out, long long *counts, char *err, int errLen) {
    try {
        lmc::LoadOverrides ov;
        ov.forceDiffuse = forceDiffuse != 0, ov.maxDepth = maxDepth, ov.width = width, ov.height = height, ov.seedOffset = seedOffset;
        std::unique_ptr<RScene> scene = BuildRScene(lmc::ParseScene(xml, ov));
        const int W = scene->camera.pixelWidth, H = scene->camera.pixelHeight, md = scene->options->maxDepth;
        if (mode != 1 && mode != 2) throw std::runtime_error("mode 1 (length) or 2 (technique) expected");
        if (md < 1 || md > 12) throw std::runtime_error("maxdepth 1 .. 12 expected");
        const int nLayers = LayerCount(mode, md);
        if (nLayers > layerCap) throw std::runtime_error("out holds " + std::to_string(layerCap) + " layers, " + std::to_string(nLayers) + " needed");
        const int nX = (W + 15) / 16, nY = (H + 15) / 16;
        const long long nTiles = (long long)nX * nY;
        McLayersFx film{out, W, H, mode, md};
        long long paths = 0;
        if (end < 0) end = nTiles * spp;
        for (long long id = begin; id < end; id++) {
            RNG rng((uint64_t)(id + scene->options->seedOffset));
            const long long tile = id % nTiles;
            const int tx = (int)(tile % nX), ty = (int)(tile / nX);
            const int x0 = tx * 16, x1 = std::min(x0 + 16, W), y0 = ty * 16, y1 = std::min(y0 + 16, H);
            for (int y = y0; y < y1; y++)
                for (int x = x0; x < x1; x++) {
                    std::vector<SubpathContrib> cs;
                    if (bidir) {
                        Path path;
                        Clear(path);
                        GeneratePathBidir(scene.get(), x, y, minDepth, md, path, cs, rng);
                    } else {
                        GeneratePathUni(scene.get(), x, y, minDepth, md, cs, rng);
                    }
                    film.Splat(cs);
                    paths++;
                }
        }
        counts[0] = paths, counts[1] = film.splats, counts[2] = film.dropped, counts[3] = film.outside;
        return nLayers;
    } catch (const std::exception &e) {
        if (err && errLen > 0) {
            strncpy(err, e.what(), errLen - 1);
            err[errLen - 1] = 0;
        }
        return -1;
    }
}
