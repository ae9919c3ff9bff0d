// TEST HELPER: the texture look-up and the BSDFs of the product (langevin-mcmc_amd/csrc/device/dshade.h, through shade_probe.h: the very lines the
// device probe runs per lane) compiled by the host compiler with the product's arithmetic contract (-ffp-contract=off), as the CPU side of the
// bit-equality test of lmc_shade_probe and for the checks against the float64 reference (tests/shade_ref.py).
// The entry takes lmc_shade_probe's arguments.  It packs the material rows itself -- texel pool, inline texture headers, as dscene.h LMC_TEX_INLINE
// describes them -- so the device's packing (host/context.cpp PackMaterials) is held against a second statement of it.
#include <algorithm>
#include <cstdint>
#include <cstring>
using std::max;
using std::min;
static inline int __float_as_int(float f) {
    int i;
    memcpy(&i, &f, 4);
    return i;
}
#include "../../langevin-mcmc_amd/csrc/device/shade_probe.h"

#include <vector>

using namespace lmcd;

extern "C" int lmc_test_shade_host(int op, int glossy, int n_mat, const float *materials, int n_bitmaps, const int *bitmap_wh, const float *bitmap_gamma,
                                   const float *texels, long long n_texels, int n, int n_rows, const int *case_ints, const float *case_in, int *out_ok, float *out) {
    if (op < 0 || op > 2 || n_mat < 1 || n < 1 || n_rows < n) return -1;
    std::vector<long long> off(n_bitmaps + 1, 0);
    for (int b = 0; b < n_bitmaps; b++) {
        if (bitmap_wh[2 * b] < 1 || bitmap_wh[2 * b + 1] < 1) return -1;
        off[b + 1] = off[b] + 3ll * bitmap_wh[2 * b] * bitmap_wh[2 * b + 1];
    }
    if (off[n_bitmaps] > n_texels) return -1;
    std::vector<DMaterial> mats(n_mat);
    std::vector<DBitmap> bitmaps(std::max(n_bitmaps, 1), DBitmap{nullptr, 0, 0, 1.f});
    for (int b = 0; b < n_bitmaps; b++) bitmaps[b] = DBitmap{texels + off[b], bitmap_wh[2 * b], bitmap_wh[2 * b + 1], bitmap_gamma[b]};
    for (int i = 0; i < n_mat; i++) {
        DMaterial &d = mats[i];
        memcpy(&d, materials + (size_t)i * 29, sizeof(d));
        if (d.type < 0 || d.type > 2) return -1;
        for (DTexRef *r : {&d.Kd, &d.Ks, &d.Kt, &d.expOrAlpha}) {
            if (r->bitmap < -1 || r->bitmap >= n_bitmaps) return -1;
#if LMC_TEX_INLINE
            if (r->bitmap >= 0) {
                const int b = r->bitmap;
                r->bitmap = (int)off[b];
                memcpy(&r->value[0], &bitmap_wh[2 * b], 4), memcpy(&r->value[1], &bitmap_wh[2 * b + 1], 4), r->value[2] = bitmap_gamma[b];
            }
#endif
        }
    }
    for (int i = 0; i < n; i++)
        if (case_ints[3 * i] < 0 || case_ints[3 * i] >= n_mat || (op == SHADE_OP_TEX && (case_ints[3 * i + 2] < 0 || case_ints[3 * i + 2] > 3))) return -1;
    DScene S;
    memset(&S, 0, sizeof(S));
    S.materials = mats.data(), S.bitmaps = bitmaps.data(), S.texPool = texels, S.numMaterials = n_mat;
    for (int i = 0; i < n; i++) {
        if (glossy) ShadeProbeCase<true>(S, op, case_ints + (size_t)i * SHADE_INT_WORDS, case_in + (size_t)i * SHADE_IN_WORDS, out_ok + i, out + (size_t)i * SHADE_OUT_WORDS);
        else
            ShadeProbeCase<false>(S, op, case_ints + (size_t)i * SHADE_INT_WORDS, case_in + (size_t)i * SHADE_IN_WORDS, out_ok + i, out + (size_t)i * SHADE_OUT_WORDS);
    }
    return 0;
}
