// Test probe of the layered MLT film's splat routine (dchain.h SplatT(ChainFilmLayers); lmc_film_layer_splat_probe): one caller-given splat per lane,
// 64-thread blocks so that many waves contend for a (pixel, layer).  The step kernels that splat into this film: device/step_*_layers.hip.
#include "kernels.h"

using namespace lmcd;

__global__ void __launch_bounds__(64) k_film_layer_splat_probe(ChainFilmLayers film, int n, const float *screenXY, const float *rgb, const int *cl, unsigned long long *outside) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 v{rgb[3 * (size_t)i], rgb[3 * (size_t)i + 1], rgb[3 * (size_t)i + 2]};
    const int c = cl[2 * (size_t)i], l = cl[2 * (size_t)i + 1];
    SplatT(film, V2{screenXY[2 * (size_t)i], screenXY[2 * (size_t)i + 1]}, v, c, l);
    // what the film's one overflow word cannot tell apart from a component out of range: counted here, by the routine's own test
    const int layer = McLayerOf(film.mode, c, l);
    if (AllFinite(v) && (layer < 0 || layer >= film.nLayers)) atomicAdd(outside, 1ull);
}
void LaunchFilmLayerSplatProbe(const ChainFilmLayers &film, int n, const float *screenXY, const float *rgb, const int *cl, unsigned long long *outside, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_film_layer_splat_probe, dim3((n + 63) / 64), dim3(64), 0, s, film, n, screenXY, rgb, cl, outside);
}
