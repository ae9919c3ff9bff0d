// One case of the shading probe (shade_probe.hip k_shade_probe; tests/helpers/dshade_host.cpp compiles the same lines for the host): a texture look-up,
// BsdfEvaluate<G> or BsdfSample<G> of dshade.h, called as they stand on a caller-given material record, with every in / out word of the call taken
// from the case's row and written back, so that what a function leaves untouched shows as the caller's own bits.
//   ints  [material index, adjoint, texture slot (0 Kd, 1 Ks, 2 Kt, 3 expOrAlpha; read by SHADE_OP_TEX alone)]
//   in    [wi 0..2 | normal 3..5 | wo 6..8 | st 9..10 | rnd 11..12 | uDiscrete 13 | pdf 14 | revPdf 15 | cosWo 16 | contrib 17..19]
//   out   [wo 0..2 | contrib 3..5 | cosWo 6 | pdf 7 | revPdf 8]; SHADE_OP_TEX writes the texture's value to contrib
//   ok    BsdfSample's return value; 1 for the two other operations
#pragma once
#include "dshade.h"

namespace lmcd {

enum { SHADE_OP_TEX = 0, SHADE_OP_EVALUATE = 1, SHADE_OP_SAMPLE = 2 };
constexpr int SHADE_INT_WORDS = 3, SHADE_IN_WORDS = 20, SHADE_OUT_WORDS = 9;

template <bool GLOSSY>
LMC_D void ShadeProbeCase(const DScene &S, int op, const int *ints, const float *in, int *ok, float *out) {
    const DMaterial m = LoadMaterialIdx<GLOSSY>(S, ints[0]);
    const bool adjoint = ints[1] != 0;
    const V3 wi{in[0], in[1], in[2]}, normal{in[3], in[4], in[5]};
    V3 wo{in[6], in[7], in[8]};
    const V2 st{in[9], in[10]}, rnd{in[11], in[12]};
    const float uDiscrete = in[13];
    float pdf = in[14], revPdf = in[15], cosWo = in[16];
    V3 contrib{in[17], in[18], in[19]};
    int result = 1;
    if (op == SHADE_OP_TEX) {
        const int slot = ints[2];
        contrib = EvalTex(S, slot == 0 ? m.Kd : slot == 1 ? m.Ks : slot == 2 ? m.Kt : m.expOrAlpha, st);
    } else if (op == SHADE_OP_EVALUATE) {
        BsdfEvaluate<GLOSSY>(S, m, adjoint, wi, normal, wo, st, contrib, cosWo, pdf, revPdf);
    } else {
        result = BsdfSample<GLOSSY>(S, m, adjoint, wi, normal, st, rnd, uDiscrete, wo, contrib, cosWo, pdf, revPdf) ? 1 : 0;
    }
    *ok = result;
    out[0] = wo.x, out[1] = wo.y, out[2] = wo.z;
    out[3] = contrib.x, out[4] = contrib.y, out[5] = contrib.z;
    out[6] = cosWo, out[7] = pdf, out[8] = revPdf;
}

}  // namespace lmcd
