// Test helper: the oracle side of the "mc" integrator (lmc_mc_render).  Built by tests/test_mc_abi.py against oracle/liblmc_oracle.so with
// the oracle's own flags (-ffp-contract=off -mfma).  Two loops over the same generators (orc::GeneratePathBidir / GeneratePathUni with a
// fixed pixel), both splatting every contribution with luminance above 1e-10 as contrib / spp (pathtrace.cpp:57-66):
//   literal = 0  the product's stream layout: stream (t, s) = RNG(t + nTiles * s + seedOffset) draws sample s of every pixel of tile t, rows
//                y0..y1 then x0..x1; the stream ids [begin, end) of nTiles * spp
//   literal = 1  the reference's PathTrace loop as written (pathtrace.cpp:37-69): one RNG(tileIndex) per tile, the spp samples of a pixel in a
//                row (no seed offset, no stream range)
// out: W*H*3 floats (accumulated into, not cleared); counts: [paths traced, contributions splatted].
#include <cstring>
#include <string>

#include "../../oracle/render.h"

using namespace orc;

namespace {

struct McFilm {
    float *rgb;
    int W, H;
    int spp;
    long long splats = 0;
    void Splat(const std::vector<SubpathContrib> &cs) {
        for (const SubpathContrib &c : cs) {
            if (Luminance(c.contrib) <= Float(1e-10)) continue;
            const Vector3 contrib = c.contrib / Float(spp);
            const int ix = Clamp(int(c.screenPos[0] * W), 0, W - 1), iy = Clamp(int(c.screenPos[1] * H), 0, H - 1);  // image.h:66-77
            if (!contrib.allFinite()) continue;
            float *px = rgb + ((size_t)iy * W + ix) * 3;
            for (int i = 0; i < 3; i++) px[i] += contrib[i];
            splats++;
        }
    }
};

void Sample(const RScene *scene, bool bidir, int x, int y, int minDepth, int maxDepth, RNG &rng, McFilm &film) {
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

extern "C" int mc_oracle_render(const char *xml, int forceDiffuse, int maxDepth, int width, int height, int seedOffset, int minDepth, int bidir, int spp,
                                long long begin, long long end, int literal, float *out, long long *counts, char *err, int errLen) {
    try {
        lmc::LoadOverrides ov;
        ov.forceDiffuse = forceDiffuse != 0, ov.maxDepth = maxDepth, ov.width = width, ov.height = height, ov.seedOffset = seedOffset;
        std::unique_ptr<RScene> scene = BuildRScene(lmc::ParseScene(xml, ov));
        const int W = scene->camera.pixelWidth, H = scene->camera.pixelHeight, md = scene->options->maxDepth;
        const int nX = (W + 15) / 16, nY = (H + 15) / 16;
        const long long nTiles = (long long)nX * nY;
        McFilm film{out, W, H, spp};
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
        counts[0] = paths, counts[1] = film.splats;
        return 0;
    } catch (const std::exception &e) {
        if (err && errLen > 0) {
            strncpy(err, e.what(), errLen - 1);
            err[errLen - 1] = 0;
        }
        return -1;
    }
}
