// Test probe of the shading functions (include/lmc_abi.h lmc_shade_probe): EvalTex, BsdfEvaluate<G> and BsdfSample<G> of device/dshade.h on caller-given
// material records and bitmaps, one case per lane (device/shade_probe.hip).  Host code only: the records go through PackMaterials (context.cpp), the
// packing UploadScene uses, so a probe's texture look-up reads what a render's would.  No context; device 0.  Everything the kernel trusts -- a case's
// material index, a record's type and bitmap indices, the bitmaps' sizes against the texel buffer -- is checked here, before the first device call.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/lmc_abi.h"
#include "../device/kernels.h"
#include "../device/shade_probe.h"
#include "context.h"
#include "hostutil.h"
#include "scene.h"

static_assert(sizeof(DMaterial) == LMC_SHADE_MAT_WORDS * 4, "include/lmc_abi.h: LMC_SHADE_MAT_WORDS is the word count of a DMaterial");
static_assert(SHADE_INT_WORDS == LMC_SHADE_INT_WORDS && SHADE_IN_WORDS == LMC_SHADE_IN_WORDS && SHADE_OUT_WORDS == LMC_SHADE_OUT_WORDS,
              "include/lmc_abi.h: the row lengths of lmc_shade_probe are those of device/shade_probe.h");

namespace {

[[noreturn]] void Refuse(const std::string &what) { throw std::runtime_error("lmc_shade_probe: " + what); }

// a 29-word row in DMaterial layout, `bitmap` an index into the caller's list -> the scene front end's record
lmc::Material MaterialOfRow(const float *row, int index, int n_bitmaps) {
    DMaterial d;
    memcpy(&d, row, sizeof(d));
    if (d.type < 0 || d.type > 2) Refuse("materials[" + std::to_string(index) + "]: type = " + std::to_string(d.type) + " is outside 0 .. 2");
    lmc::Material m;
    m.type = d.type, m.twoSided = d.twoSided != 0;
    const char *names[4] = {"Kd", "Ks", "Kt", "expOrAlpha"};
    const DTexRef *src[4] = {&d.Kd, &d.Ks, &d.Kt, &d.expOrAlpha};
    lmc::TextureRef *dst[4] = {&m.Kd, &m.Ks, &m.Kt, &m.expOrAlpha};
    for (int k = 0; k < 4; k++) {
        if (src[k]->bitmap < -1 || src[k]->bitmap >= n_bitmaps)
            Refuse("materials[" + std::to_string(index) + "]: " + names[k] + ".bitmap = " + std::to_string(src[k]->bitmap) + " is outside [-1, n_bitmaps)");
        dst[k]->bitmap = src[k]->bitmap, dst[k]->sScale = src[k]->sScale, dst[k]->tScale = src[k]->tScale;
        memcpy(dst[k]->value, src[k]->value, 12);
    }
    m.eta = d.eta, m.invEta = d.invEta, m.KsWeight = d.KsWeight;
    return m;
}

}  // namespace

extern "C" int lmc_shade_probe(int op, int glossy, int n_mat, const float *materials, int n_bitmaps, const int *bitmap_wh, const float *bitmap_gamma, const float *texels,
                               long long n_texels, int n, int n_rows, const int *case_ints, const float *case_in, int *out_ok, float *out) {
    LMC_TRY
    if (op != SHADE_OP_TEX && op != SHADE_OP_EVALUATE && op != SHADE_OP_SAMPLE) Refuse("op = " + std::to_string(op) + " is not 0 (EvalTex), 1 (BsdfEvaluate) or 2 (BsdfSample)");
    if (n_mat < 1) Refuse("n_mat = " + std::to_string(n_mat) + ": at least one material is required");
    if (!materials) Refuse("materials is null");
    if (n_bitmaps < 0) Refuse("n_bitmaps = " + std::to_string(n_bitmaps) + " is negative");
    if (n_bitmaps > 0 && !bitmap_wh) Refuse("bitmap_wh is null");
    if (n_bitmaps > 0 && !bitmap_gamma) Refuse("bitmap_gamma is null");
    if (n_bitmaps > 0 && !texels) Refuse("texels is null");
    if (n < 1) Refuse("n = " + std::to_string(n) + ": at least one case is required (n = 0 is not a call)");
    if (n_rows < n) Refuse("n_rows = " + std::to_string(n_rows) + " is smaller than n = " + std::to_string(n));
    if (!case_ints) Refuse("case_ints is null");
    if (!case_in) Refuse("case_in is null");
    if (!out_ok) Refuse("out_ok is null");
    if (!out) Refuse("out is null");
    std::vector<lmc::Bitmap> bitmaps((size_t)n_bitmaps);
    long long need = 0;
    for (int b = 0; b < n_bitmaps; b++) {
        const int W = bitmap_wh[2 * b], H = bitmap_wh[2 * b + 1];
        if (W < 1 || H < 1) Refuse("bitmap_wh[" + std::to_string(b) + "] = " + std::to_string(W) + " x " + std::to_string(H) + ": width and height must be at least 1");
        need += 3ll * W * H;
        if (need >= 1ll << 31) Refuse("bitmap_wh: the bitmaps hold more than 2^31 words");
    }
    if (n_texels < need) Refuse("n_texels = " + std::to_string(n_texels) + " is shorter than the bitmaps' 3 W H words, " + std::to_string(need));
    need = 0;
    for (int b = 0; b < n_bitmaps; b++) {
        lmc::Bitmap &bm = bitmaps[b];
        bm.img.width = bitmap_wh[2 * b], bm.img.height = bitmap_wh[2 * b + 1], bm.gamma = bitmap_gamma[b];
        const long long words = 3ll * bm.img.width * bm.img.height;
        bm.img.data.assign(texels + need, texels + need + words);
        need += words;
    }
    std::vector<lmc::Material> mats;
    for (int i = 0; i < n_mat; i++) mats.push_back(MaterialOfRow(materials + (size_t)i * LMC_SHADE_MAT_WORDS, i, n_bitmaps));
    for (int i = 0; i < n; i++) {
        const int *ci = case_ints + (size_t)i * SHADE_INT_WORDS;
        if (ci[0] < 0 || ci[0] >= n_mat) Refuse("case_ints[" + std::to_string(i) + "]: material = " + std::to_string(ci[0]) + " is outside [0, n_mat)");
        if (op == SHADE_OP_TEX && (ci[2] < 0 || ci[2] > 3)) Refuse("case_ints[" + std::to_string(i) + "]: texture slot = " + std::to_string(ci[2]) + " is outside 0 .. 3");
    }
    const PackedMaterials pm = PackMaterials(mats, bitmaps);  // (refuses an unknown type and a bitmap index beyond the list itself, too)

    EnsureDevice(0);
    uint32_t nanBits = LMC_SHADE_UNTOUCHED_BITS;
    float untouched;
    memcpy(&untouched, &nanBits, 4);
    DevBuf<DMaterial> dMats;
    DevBuf<float> dPool, dIn, dOut;
    DevBuf<DBitmap> dBitmaps;
    DevBuf<int> dInts, dOk;
    dMats.Upload(pm.mats), dPool.Upload(pm.pool), dBitmaps.Upload(BitmapHeaders(pm, bitmaps, dPool.p));
    dInts.Upload(case_ints, (size_t)n * SHADE_INT_WORDS), dIn.Upload(case_in, (size_t)n * SHADE_IN_WORDS);
    dOk.Upload(std::vector<int>((size_t)n_rows, LMC_PROBE_SENTINEL)), dOut.Upload(std::vector<float>((size_t)n_rows * SHADE_OUT_WORDS, untouched));
    DScene S;
    memset(&S, 0, sizeof(S));
    S.materials = dMats.p, S.bitmaps = dBitmaps.p, S.texPool = dPool.p, S.numMaterials = n_mat, S.glossy = pm.glossy;
    LaunchShadeProbe(S, op, glossy != 0, n, dInts.p, dIn.p, dOk.p, dOut.p, 0);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out_ok, dOk.p, (size_t)n_rows * sizeof(int), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(out, dOut.p, (size_t)n_rows * SHADE_OUT_WORDS * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
    LMC_CATCH(-1)
}
