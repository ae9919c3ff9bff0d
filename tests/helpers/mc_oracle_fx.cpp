// Test helper: the oracle side of the EXACT mc film (lmc_set_option "mc_film_exact"; INTEGRATION.md "Exact mc film").  Built by
// tests/test_mc_exact_abi.py against oracle/liblmc_oracle.so the way tests/test_mc_abi.py builds mc_oracle.cpp.  The two loops of mc_oracle.cpp
// (literal = 0: the product's stream layout, the ids [begin, end) of nTiles * spp; literal = 1: the reference's PathTrace loop, one RNG(tile)
// per tile) restated over an int64 film under the exact mode's rules:
//   a contribution is skipped by the luminance test (<= 1e-10) and by the finite test of its UNWEIGHTED components; it is counted then;
//   a contribution with a component |v| >= 2^30 is dropped whole and counted in counts[2];
//   otherwise every component adds q = llrint((double)v * 2^32) to its word.  Nothing is divided by spp.
// out: W*H*3 int64 words (accumulated into, not cleared); counts: [paths traced, contributions counted, contributions dropped by the range rule].
#include <cmath>
#include <cstring>
#include <string>

#include "../../oracle/render.h"

using namespace orc;

namespace {

constexpr float kLimit = 1073741824.0f;    // 2^30
constexpr double kScale = 4294967296.0;    // 2^32

struct McFilmFx {
    long long *words;
    int W, H;
    long long splats = 0, dropped = 0;
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
            const int ix = Clamp(int(c.screenPos[0] * W), 0, W - 1), iy = Clamp(int(c.screenPos[1] * H), 0, H - 1);  // image.h:66-77
            long long *px = words + ((size_t)iy * W + ix) * 3;
            for (int i = 0; i < 3; i++) px[i] += std::llrint((double)(float)v[i] * kScale);
        }
    }
};

void Sample(const RScene *scene, bool bidir, int x, int y, int minDepth, int maxDepth, RNG &rng, McFilmFx &film) {
    std::vector<SubpathContrib> cs;
    if (bidir) {
        Path path;
        Clear(path);
        GeneratePathBidir(scene, x, y, minDepth, maxDepth, path, cs, rng);
    } else {
        GeneratePathUni(scene, x, y, minDepth, maxDepth, cs, rng);
    }
    film.Splat(cs);
}

}  // namespace

extern "C" int mc_oracle_fx_render(const char *xml, int forceDiffuse, int maxDepth, int width, int height, int seedOffset, int minDepth, int bidir, int spp,
                                   long long begin, long long end, int literal, long long *out, long long *counts, char *err, int errLen) {
    try {
        lmc::LoadOverrides ov;
        ov.forceDiffuse = forceDiffuse != 0, ov.maxDepth = maxDepth, ov.width = width, ov.height = height, ov.seedOffset = seedOffset;
        std::unique_ptr<RScene> scene = BuildRScene(lmc::ParseScene(xml, ov));
        const int W = scene->camera.pixelWidth, H = scene->camera.pixelHeight, md = scene->options->maxDepth;
        const int nX = (W + 15) / 16, nY = (H + 15) / 16;
        const long long nTiles = (long long)nX * nY;
        McFilmFx film{out, W, H};
        long long paths = 0;
        auto tileLoop = [&](long long tile, RNG &rng, int samplesPerPixel) {
            const int tx = (int)(tile % nX), ty = (int)(tile / nX);
            const int x0 = tx * 16, x1 = std::min(x0 + 16, W), y0 = ty * 16, y1 = std::min(y0 + 16, H);
            for (int y = y0; y < y1; y++)
                for (int x = x0; x < x1; x++)
                    for (int s = 0; s < samplesPerPixel; s++) {
                        Sample(scene.get(), bidir != 0, x, y, minDepth, md, rng, film);
                        paths++;
                    }
        };
        if (literal) {
            for (long long tile = 0; tile < nTiles; tile++) {
                RNG rng((uint64_t)tile);  // pathtrace.cpp:39-40
                tileLoop(tile, rng, spp);
            }
        } else {
            if (end < 0) end = nTiles * spp;
            for (long long id = begin; id < end; id++) {
                RNG rng((uint64_t)(id + scene->options->seedOffset));
                tileLoop(id % nTiles, rng, 1);
            }
        }
        counts[0] = paths, counts[1] = film.splats, counts[2] = film.dropped;
        return 0;
    } catch (const std::exception &e) {
        if (err && errLen > 0) {
            strncpy(err, e.what(), errLen - 1);
            err[errLen - 1] = 0;
        }
        return -1;
    }
}
