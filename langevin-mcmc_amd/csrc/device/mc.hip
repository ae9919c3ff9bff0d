// The "mc" integrator: the reference's PathTrace (pathtrace.cpp:14-78) -- spp samples of every pixel, GeneratePathBidir with a fixed
// pixel when <dpt bidirectional> is true (the default), GeneratePath (DirectSample, ddirect.h) otherwise; every contribution with
// luminance above 1e-10 is splatted with weight 1 / spp.
//
// Streams.  Stream (t, s) = RNG(t + nTiles * s + seedOffset), t the 16x16 tile index (ty * nXTiles + tx, pathtrace.cpp:39-40), s in [0, spp)
// the sample index; it draws sample s of every pixel of tile t in the reference's pixel order (rows y0..y1, then x0..x1).  With spp = 1 and
// seedOffset 0 that is the reference's own loop (one RNG(tileIndex) per tile).  A launch renders a contiguous range [begin, end) of stream
// ids t + nTiles * s, so the image does not depend on the launch geometry or on how the range is split over devices.
//
// Lanes.  Thread g walks stream (t, s) = (g / nS, sBase + g % nS): the samples of one tile sit side by side in a wave and walk the same
// pixel at the same time.  A sample's camera-side contributions all land in its own pixel; they are summed in the lane and the lanes of a
// wave that share a pixel add once (wave reduction) instead of 64 times to the same three floats (MI355X_MICROARCH.md: many adders on one
// row run ~14x slower).  Light-tracing contributions (ConnectToCamera) land anywhere and are added on the spot.
//
// Films.  The sink is a type per film type (dchain.h Film / FilmFixed; LaunchMC picks through DispatchFilm), so the float kernels hold no trace
// of the exact film.  Exact mode ("mc_film_exact"): the film is the integer sum of the UNWEIGHTED contributions, q = llrint((double)v * 2^32)
// per component; a contribution with a component |v| >= 2^30 is dropped whole and counted in the film's overflow word (after the contribution
// counter, which therefore stays the float mode's).  Nothing is divided by spp on the device; lmc_mc_read does that once (k_mc_fixed_to_float).
// Either kernel only ever adds to the film: clearing it, or not, is the host's business (lmc_mc_render / lmc_mc_accumulate).
//
// Layers ("mc_layers", INTEGRATION.md "Layered mc film"): the same render into nLayers films side by side, a contribution going to the layer of its path
// length L = camDepth + lightDepth - 1 (mode 1) or of its technique (camDepth, lightDepth) (mode 2; McLayerOf, kernels.h).  FilmLayers / FilmFixedLayers
// are types of their own with sinks and k_mc instantiations of their own, so the unlayered kernels hold no trace of them.  A contribution outside the
// table (it cannot occur) is dropped, and in exact mode counted in the overflow word behind the last layer.  k_mc_sum_layers_* adds the layers up.
#include "kernels.h"
#include "ddirect.h"

using namespace lmcd;

namespace {

constexpr float kMcMinLuminance = 1e-10f;  // pathtrace.cpp:60

// where one sample's contributions go: the camera-side ones into the lane's own-pixel sum, the rest straight to the film
template <class FILM>
struct McSink;
template <>
struct McSink<Film> {
    Film film;
    float spp;  // contrib / spp: a division, as Eigen's vector / scalar in the reference
    V3 acc;
    int accPix;   // film index of the own-pixel sum, -1 while empty
    unsigned splats;
    LMC_D static int PixelOf(const Film &f, V2 sp) {  // Splat's nearest pixel (dchain.h)
        const int ix = Clampi((int)(sp.x * f.W), 0, f.W - 1), iy = Clampi((int)(sp.y * f.H), 0, f.H - 1);
        return iy * f.W + ix;
    }
    LMC_D void Add(bool ownPixel, V2 sp, V3 contrib) {
        if (Luminance(contrib) <= kMcMinLuminance) return;
        if (!AllFinite(contrib)) return;  // Splat drops it (image.h:66-77)
        const V3 c{contrib.x / spp, contrib.y / spp, contrib.z / spp};
        splats++;
        const int pix = PixelOf(film, sp);
        if (ownPixel && (accPix < 0 || accPix == pix)) {
            accPix = pix;
            acc = acc + c;
            return;
        }
        float *px = film.rgb + (size_t)pix * 3;
        unsafeAtomicAdd(px + 0, c.x), unsafeAtomicAdd(px + 1, c.y), unsafeAtomicAdd(px + 2, c.z);
    }
    LMC_D void Push(const Contrib &c) { Add(c.camDepth != 1, c.screenPos, c.contrib); }  // camDepth 1: ConnectToCamera (light tracing)
    LMC_D void operator()(V2 sp, V3 contrib) { Add(true, sp, contrib); }                 // GeneratePath: camera side only
};
// ... the exact film: the own-pixel sum is three int64 words of unweighted fixed-point contributions
template <>
struct McSink<FilmFixed> {
    FilmFixed film;
    unsigned long long ax, ay, az;  // two's complement: the unsigned add is the signed one
    int accPix;
    unsigned splats;
    LMC_D void Add(bool ownPixel, V2 sp, V3 contrib) {
        if (Luminance(contrib) <= kMcMinLuminance) return;
        if (!AllFinite(contrib)) return;
        splats++;
        if (fabsf(contrib.x) >= FILM_FX_LIMIT || fabsf(contrib.y) >= FILM_FX_LIMIT || fabsf(contrib.z) >= FILM_FX_LIMIT) {  // Splat(FilmFixed)'s range rule
            atomicAdd(film.fx + (size_t)film.W * film.H * 3, 1ull);
            return;
        }
        const unsigned long long qx = (unsigned long long)llrint((double)contrib.x * FILM_FX_SCALE), qy = (unsigned long long)llrint((double)contrib.y * FILM_FX_SCALE),
                                 qz = (unsigned long long)llrint((double)contrib.z * FILM_FX_SCALE);
        const int pix = McSink<Film>::PixelOf(Film{nullptr, film.W, film.H}, sp);
        if (ownPixel && (accPix < 0 || accPix == pix)) {
            accPix = pix;
            ax += qx, ay += qy, az += qz;
            return;
        }
        unsigned long long *px = film.fx + (size_t)pix * 3;
        atomicAdd(px + 0, qx), atomicAdd(px + 1, qy), atomicAdd(px + 2, qz);
    }
    LMC_D void Push(const Contrib &c) { Add(c.camDepth != 1, c.screenPos, c.contrib); }
    LMC_D void operator()(V2 sp, V3 contrib) { Add(true, sp, contrib); }
};
LMC_D McSink<Film> MakeSink(const Film &film, int spp) { return McSink<Film>{film, (float)spp, V3{0, 0, 0}, -1, 0u}; }
LMC_D McSink<FilmFixed> MakeSink(const FilmFixed &film, int) { return McSink<FilmFixed>{film, 0ull, 0ull, 0ull, -1, 0u}; }

// The layered films: nLayers films of W*H*3 words one after the other, in exact mode one overflow word behind them.
struct FilmLayers {
    float *rgb;
    int W, H, nLayers, mode;
};
struct FilmFixedLayers {
    unsigned long long *fx;
    int W, H, nLayers, mode;
};
// Their sinks keep the rules of the sinks above per contribution.  The own-pixel sum is keyed by (layer, pixel): key = layer * W*H + pixel, the film index
// of the sum.  A sample's camera-side contributions change layer as the path grows, so a sum is flushed (plain atomics) when the key changes; the one
// that is pending at the converged point goes through CommitOwnPixel's rounds like the unlayered one.
template <>
struct McSink<FilmLayers> {
    FilmLayers film;
    float spp;
    V3 acc;
    int accPix;  // key of the pending sum, -1 while empty
    unsigned splats;
    LMC_D void Add(bool ownPixel, V2 sp, V3 contrib, int camDepth, int lightDepth) {
        if (Luminance(contrib) <= kMcMinLuminance) return;
        if (!AllFinite(contrib)) return;
        const V3 c{contrib.x / spp, contrib.y / spp, contrib.z / spp};
        splats++;
        const int layer = McLayerOf(film.mode, camDepth, lightDepth);
        if (layer < 0 || layer >= film.nLayers) return;  // outside the table: never written (the float film has no overflow word to count it in)
        const int key = layer * (film.W * film.H) + McSink<Film>::PixelOf(Film{nullptr, film.W, film.H}, sp);
        if (ownPixel) {
            if (accPix == key) {
                acc = acc + c;
                return;
            }
            if (accPix >= 0) {
                float *px = film.rgb + (size_t)accPix * 3;
                unsafeAtomicAdd(px + 0, acc.x), unsafeAtomicAdd(px + 1, acc.y), unsafeAtomicAdd(px + 2, acc.z);
            }
            accPix = key;
            acc = c;
            return;
        }
        float *px = film.rgb + (size_t)key * 3;
        unsafeAtomicAdd(px + 0, c.x), unsafeAtomicAdd(px + 1, c.y), unsafeAtomicAdd(px + 2, c.z);
    }
    LMC_D void Push(const Contrib &c) { Add(c.camDepth != 1, c.screenPos, c.contrib, c.camDepth, c.lightDepth); }
    LMC_D void Technique(V2 sp, V3 contrib, int camDepth, int lightDepth) { Add(true, sp, contrib, camDepth, lightDepth); }  // GeneratePath (ddirect.h EmitContrib)
};
template <>
struct McSink<FilmFixedLayers> {
    FilmFixedLayers film;
    unsigned long long ax, ay, az;
    int accPix;
    unsigned splats;
    LMC_D void Add(bool ownPixel, V2 sp, V3 contrib, int camDepth, int lightDepth) {
        if (Luminance(contrib) <= kMcMinLuminance) return;
        if (!AllFinite(contrib)) return;
        splats++;
        const int layer = McLayerOf(film.mode, camDepth, lightDepth);
        if (fabsf(contrib.x) >= FILM_FX_LIMIT || fabsf(contrib.y) >= FILM_FX_LIMIT || fabsf(contrib.z) >= FILM_FX_LIMIT || layer < 0 || layer >= film.nLayers) {
            atomicAdd(film.fx + (size_t)film.nLayers * film.W * film.H * 3, 1ull);  // the range rule, or outside the table: dropped whole and counted
            return;
        }
        const unsigned long long qx = (unsigned long long)llrint((double)contrib.x * FILM_FX_SCALE), qy = (unsigned long long)llrint((double)contrib.y * FILM_FX_SCALE),
                                 qz = (unsigned long long)llrint((double)contrib.z * FILM_FX_SCALE);
        const int key = layer * (film.W * film.H) + McSink<Film>::PixelOf(Film{nullptr, film.W, film.H}, sp);
        if (ownPixel) {
            if (accPix == key) {
                ax += qx, ay += qy, az += qz;
                return;
            }
            if (accPix >= 0) {
                unsigned long long *px = film.fx + (size_t)accPix * 3;
                atomicAdd(px + 0, ax), atomicAdd(px + 1, ay), atomicAdd(px + 2, az);
            }
            accPix = key;
            ax = qx, ay = qy, az = qz;
            return;
        }
        unsigned long long *px = film.fx + (size_t)key * 3;
        atomicAdd(px + 0, qx), atomicAdd(px + 1, qy), atomicAdd(px + 2, qz);
    }
    LMC_D void Push(const Contrib &c) { Add(c.camDepth != 1, c.screenPos, c.contrib, c.camDepth, c.lightDepth); }
    LMC_D void Technique(V2 sp, V3 contrib, int camDepth, int lightDepth) { Add(true, sp, contrib, camDepth, lightDepth); }
};
LMC_D McSink<FilmLayers> MakeSink(const FilmLayers &film, int spp) { return McSink<FilmLayers>{film, (float)spp, V3{0, 0, 0}, -1, 0u}; }
LMC_D McSink<FilmFixedLayers> MakeSink(const FilmFixedLayers &film, int) { return McSink<FilmFixedLayers>{film, 0ull, 0ull, 0ull, -1, 0u}; }

LMC_D float WaveSum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// every lane of the wave arrives here (converged): the own-pixel sums of the wave committed, one add per pixel for the lanes that share one
template <class SINK>
LMC_D void CommitOwnPixelFloat(float *rgb, SINK &sink, int lane) {
    const int key = sink.accPix;
    unsigned long long pending = __ballot(key >= 0);
    for (int round = 0; pending && round < 4; round++) {
        const int leader = __ffsll((long long)pending) - 1;
        const int lk = __shfl(key, leader);
        const bool mine = key == lk && key >= 0;
        const unsigned long long group = __ballot(mine);
        if (__popcll(group) < 2) break;  // lanes on different pixels: plain atomics below
        const float rx = WaveSum(mine ? sink.acc.x : 0.f), ry = WaveSum(mine ? sink.acc.y : 0.f), rz = WaveSum(mine ? sink.acc.z : 0.f);
        if (lane == leader) {
            float *px = rgb + (size_t)lk * 3;
            unsafeAtomicAdd(px + 0, rx), unsafeAtomicAdd(px + 1, ry), unsafeAtomicAdd(px + 2, rz);
        }
        if (mine) sink.accPix = -1;
        pending &= ~group;
    }
    if (sink.accPix >= 0) {
        float *px = rgb + (size_t)sink.accPix * 3;
        unsafeAtomicAdd(px + 0, sink.acc.x), unsafeAtomicAdd(px + 1, sink.acc.y), unsafeAtomicAdd(px + 2, sink.acc.z);
    }
    sink.accPix = -1;
    sink.acc = V3{0, 0, 0};
}
LMC_D void CommitOwnPixel(const Film &film, McSink<Film> &sink, int lane) { CommitOwnPixelFloat(film.rgb, sink, lane); }
LMC_D void CommitOwnPixel(const FilmLayers &film, McSink<FilmLayers> &sink, int lane) { CommitOwnPixelFloat(film.rgb, sink, lane); }  // the key is the film index

LMC_D unsigned long long WaveSumU64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// ... the same rounds over the exact film: the group's three words summed in integers, one lane issues the three 64-bit atomics
template <class SINK>
LMC_D void CommitOwnPixelFixed(unsigned long long *fx, SINK &sink, int lane) {
    const int key = sink.accPix;
    unsigned long long pending = __ballot(key >= 0);
    for (int round = 0; pending && round < 4; round++) {
        const int leader = __ffsll((long long)pending) - 1;
        const int lk = __shfl(key, leader);
        const bool mine = key == lk && key >= 0;
        const unsigned long long group = __ballot(mine);
        if (__popcll(group) < 2) break;  // lanes on different pixels: plain atomics below
        const unsigned long long rx = WaveSumU64(mine ? sink.ax : 0ull), ry = WaveSumU64(mine ? sink.ay : 0ull), rz = WaveSumU64(mine ? sink.az : 0ull);
        if (lane == leader) {
            unsigned long long *px = fx + (size_t)lk * 3;
            atomicAdd(px + 0, rx), atomicAdd(px + 1, ry), atomicAdd(px + 2, rz);
        }
        if (mine) sink.accPix = -1;
        pending &= ~group;
    }
    if (sink.accPix >= 0) {
        unsigned long long *px = fx + (size_t)sink.accPix * 3;
        atomicAdd(px + 0, sink.ax), atomicAdd(px + 1, sink.ay), atomicAdd(px + 2, sink.az);
    }
    sink.accPix = -1;
    sink.ax = sink.ay = sink.az = 0ull;
}
LMC_D void CommitOwnPixel(const FilmFixed &film, McSink<FilmFixed> &sink, int lane) { CommitOwnPixelFixed(film.fx, sink, lane); }
LMC_D void CommitOwnPixel(const FilmFixedLayers &film, McSink<FilmFixedLayers> &sink, int lane) { CommitOwnPixelFixed(film.fx, sink, lane); }

// LMC_MC_MIN_WAVES: the waves per SIMD the register allocation must leave room for.  3 (at most 168 VGPRs): bidirectional renders at 64 spp
// take 13 % (torus) / 22 % (veach-door) less time than with the free allocation (208 VGPRs, 2 waves) and than 4 (128 VGPRs, more scratch traffic); the
// unidirectional kernel needs ~150 either way (profiles/r07_mc_ab_*.jsonl, scripts/build_variant.sh)
#ifndef LMC_MC_MIN_WAVES
#define LMC_MC_MIN_WAVES 3
#endif

// counters: [paths traced, contributions splatted]
template <bool GLOSSY, bool BIDIR, class FILM>
__global__ void __launch_bounds__(64, LMC_MC_MIN_WAVES) k_mc(DScene S, FILM film, int spp, int nXTiles, int nTiles, long long sBase, int nS, long long streamBegin,
                                           long long streamEnd, int minDepth, int maxDepth, uint32_t *tabScratch, unsigned long long *counters) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const long long t = g / nS, s = sBase + g % nS;
    const long long id = t + (long long)nTiles * s;
    const bool active = t < nTiles && id >= streamBegin && id < streamEnd;
    int x0 = 0, y0 = 0, tw = 0, th = 0;
    Rng rng;
    rng.tab = tabScratch + (size_t)g * 64;  // only written if the stream ticks (once per 2^32 draws)
    rng.ticks = 0;
    rng.state = 0;
    if (active) {
        const int tx = (int)(t % nXTiles), ty = (int)(t / nXTiles);
        x0 = tx * 16, y0 = ty * 16;
        tw = min(x0 + 16, S.cam.width) - x0, th = min(y0 + 16, S.cam.height) - y0;
        const uint64_t seed = (uint64_t)(id + S.opt.seedOffset);
        rng.SetSynth(seed);                    // the extension table synthesised from the seed (drng.h), not written to memory
        rng.state = PcgAdvance(rng.s0, 64);    // RNG(seed)'s first state: 64 LCG steps (the table fill) behind S0
    }
    const int nPix = tw * th;
    McSink<FILM> sink = MakeSink(film, spp);
    LocalStackT<GLOSSY> stk;
    DPath path;
    unsigned paths = 0;
    for (int k = 0; __ballot(k < nPix); k++) {
        if (k < nPix) {
            const int x = x0 + k % tw, y = y0 + k / tw;  // rows y0..y1, then x0..x1
            if (BIDIR) GeneratePathBidir(S, minDepth, maxDepth, path, sink, rng, stk, PixelScreen{x, y});
            else
                DirectSample(S, sink, x, y, minDepth, maxDepth, rng, stk);
            paths++;
        }
        CommitOwnPixel(film, sink, lane);
    }
    const unsigned long long np = WaveSumU64(paths), ns = WaveSumU64(sink.splats);
    if (lane == 0 && np) atomicAdd(counters + 0, np), atomicAdd(counters + 1, ns);
}

}  // namespace

void LaunchMC(const DScene &S, const Film &film, int layerMode, int nLayers, bool bidirectional, int spp, int minDepth, int maxDepth, long long streamBegin,
              long long streamEnd, uint32_t *tabScratch, unsigned long long *counters, hipStream_t s) {
    const int nX = (S.cam.width + 15) / 16, nY = (S.cam.height + 15) / 16, nTiles = nX * nY;
    if (streamEnd <= streamBegin) return;
    const long long sBase = streamBegin / nTiles, sLast = (streamEnd - 1) / nTiles;
    const int nS = (int)(sLast - sBase + 1);
    const long long nThreads = (long long)nTiles * nS;
    const dim3 grid((unsigned)((nThreads + 63) / 64)), block(64);
#define LMC_MC_ARGS S, f, spp, nX, nTiles, sBase, nS, streamBegin, streamEnd, minDepth, maxDepth, tabScratch, counters
    auto launch = [&](const auto &f) {
        using FILM = std::decay_t<decltype(f)>;
        if (S.glossy && bidirectional) hipLaunchKernelGGL((k_mc<true, true, FILM>), grid, block, 0, s, LMC_MC_ARGS);
        else if (S.glossy) hipLaunchKernelGGL((k_mc<true, false, FILM>), grid, block, 0, s, LMC_MC_ARGS);
        else if (bidirectional) hipLaunchKernelGGL((k_mc<false, true, FILM>), grid, block, 0, s, LMC_MC_ARGS);
        else
            hipLaunchKernelGGL((k_mc<false, false, FILM>), grid, block, 0, s, LMC_MC_ARGS);
    };
    DispatchFilm(film, [&](const auto &f) {  // the layered film is a type of its own, picked here like the exact one
        using FILM = std::decay_t<decltype(f)>;
        if (layerMode == 0) launch(f);
        else if constexpr (std::is_same_v<FILM, FilmFixed>) launch(FilmFixedLayers{f.fx, f.W, f.H, nLayers, layerMode});
        else
            launch(FilmLayers{f.rgb, f.W, f.H, nLayers, layerMode});
    });
#undef LMC_MC_ARGS
}
// total = the sum of the layers: int64 adds, or float adds in increasing layer index (a pure function of the layers)
__global__ void k_mc_sum_layers_fixed(const long long *layers, long long *total, size_t n, int nLayers) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        long long v = 0;
        for (int k = 0; k < nLayers; k++) v += layers[(size_t)k * n + i];
        total[i] = v;
    }
}
__global__ void k_mc_sum_layers_float(const float *layers, float *total, size_t n, int nLayers) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int k = 0; k < nLayers; k++) v += layers[(size_t)k * n + i];
        total[i] = v;
    }
}
void LaunchMCSumLayers(const long long *layers, long long *total, size_t n, int nLayers, hipStream_t s) {
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    if (n) hipLaunchKernelGGL(k_mc_sum_layers_fixed, dim3(blocks), dim3(256), 0, s, layers, total, n, nLayers);
}
void LaunchMCSumLayers(const float *layers, float *total, size_t n, int nLayers, hipStream_t s) {
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    if (n) hipLaunchKernelGGL(k_mc_sum_layers_float, dim3(blocks), dim3(256), 0, s, layers, total, n, nLayers);
}
// the exact mc film as floats (lmc_mc_read): float(double(q) * 2^-32 / double(spp)), the one division of the exact mode; numpy's
// np.float32(np.float64(q) * 2.0**-32 / spp) takes the same three steps
__global__ void k_mc_fixed_to_float(const long long *fx, float *rgb, size_t n, double spp) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) rgb[i] = (float)((double)fx[i] * (1.0 / FILM_FX_SCALE) / spp);
}
void LaunchMCFixedToFloat(const long long *fx, float *rgb, size_t n, int spp, hipStream_t s) {
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    if (n) hipLaunchKernelGGL(k_mc_fixed_to_float, dim3(blocks), dim3(256), 0, s, fx, rgb, n, (double)spp);
}
long long MCThreads(const DScene &S, long long streamBegin, long long streamEnd) {
    const int nTiles = ((S.cam.width + 15) / 16) * ((S.cam.height + 15) / 16);
    if (streamEnd <= streamBegin) return 0;
    return (long long)nTiles * ((streamEnd - 1) / nTiles - streamBegin / nTiles + 1);
}
