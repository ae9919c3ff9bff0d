// Checkpoint records (host/ckpt.cpp lmc_checkpoint_save / _load; INTEGRATION.md "Checkpoint and resume"): every word the chain loop can read of a
// chain between two steps, as ONE record per chain in chain order -- whatever slot the chain lives in (relocate.hip) and whatever member of an
// in-process group holds it.  The relocation's staging record (relocate.hip RW_*) is the model; added here: the chain's init state (the outlier
// reset reads it, dchain.h ResetToInitState), `samplecache`'s chain.path / chain.spContrib and the dense Gaussian of an H2MC chain
// (dh2coop.h H2Arrays::gauss, per slot).  Scratch is left out: contribList, the unselected path and Gaussian buffers, the pipelines' hand-off state,
// pushDim / pushData (consumed by the step that wrote them), the relocation's own arrays.
//   k_ckpt_pack    chains [first, first + n) -> n records in a staging buffer (read through A.slotOf, or the identity)
//   k_ckpt_unpack  n records -> the slots [first, first + n) of a freshly set-up identity layout (slot = chain, as lmc_chains_init leaves it)
// Lane = chain: the SoA rows are read (written) unit-stride wherever the chains of a wave are neighbours in slot order; the record side is one
// word per lane and instruction, 64 lines touched per store.  That is the slow side and it does not matter: a chunk is packed in a fraction of the
// time its copy to the host takes, and the file takes an order of magnitude longer than both (DESIGN.md "Checkpoint").
// A record has a FIXED number of words per render (CkptLayout: a function of maxdepth, samplecache, h2mc), so that a file can be cut at any chain;
// words that are dead for a chain (vertices beyond its counts, splats beyond its count, a Gaussian it does not hold, the RNG table of a stream that
// has not ticked) are written as zeros and not read back.
#include "dstep.h"
#include "dh2coop.h"
#include "kernels.h"

namespace lmcd {
namespace {

enum : int { CK_FLAGS = 0, CK_SAMPLEIDX, CK_NUMSAMPLES, CK_ADJREJECT, CK_SPLATCOUNT, CK_NEXTKIND, CK_RNG_LO, CK_RNG_HI, CK_RNG_TICKED, CK_SCORESUM, CK_LASTSCORESUM, CK_LASTSCORE, CK_PATHWEIGHT, CK_INITSCORESUM, CK_SCALARS = 16 };

struct Layout {
    int nV, nS, sampleCache, h2mc;
    LMC_HD int PathWords() const { return DPATH_HEAD_WORDS + 2 * nV * DVERTEX_WORDS; }
    LMC_HD int Tab() const { return CK_SCALARS; }
    LMC_HD int Path() const { return Tab() + 64; }
    LMC_HD int Contrib() const { return Path() + PathWords(); }
    LMC_HD int Splats() const { return Contrib() + CONTRIB_WORDS; }
    LMC_HD int Vectors() const { return Splats() + nS * SPLAT_WORDS; }
    LMC_HD int Gauss() const { return Vectors() + 7 * MAXPSS; }
    LMC_HD int InitPath() const { return Gauss() + GAUSS_WORDS; }
    LMC_HD int InitContrib() const { return InitPath() + PathWords(); }
    LMC_HD int ChPath() const { return InitContrib() + CONTRIB_WORDS; }
    LMC_HD int ChContrib() const { return ChPath() + (sampleCache ? PathWords() : 0); }
    LMC_HD int H2Gauss() const { return ChContrib() + (sampleCache ? CONTRIB_WORDS : 0); }
    LMC_HD int Words() const { return H2Gauss() + (h2mc ? H2_GAUSS_AOS : 0); }
};

LMC_D float *VectorBase(const ChainArrays &A, int v) {
    float *const b[7] = {A.chV1, A.chV2, A.chCurrNewV2, A.chPropNewV1, A.chPropNewV2, A.chPss, A.chLastPss};
    return b[v];
}
LMC_D bool HasStoredGaussian(int flags) { return (flags & F_GAUSS) && !(flags & F_GAUSS_ISO); }
LMC_D int ClampCount(float word, int nV) { return min(max(__float_as_int(word), 0), nV); }

// SoA path rows of slot i -> the PathWords() words at r: head, nV camera vertices, nV light vertices (dead ones zero)
LMC_D void PackPath(const float *path, size_t N, int i, int nV, float *r) {
#pragma unroll 4
    for (int k = 0; k < DPATH_HEAD_WORDS; k++) r[k] = path[(size_t)k * N + i];
    const int cam = ClampCount(r[12], nV), lgt = ClampCount(r[13], nV);  // DPath: camCount, lgtCount
    for (int v = 0; v < nV; v++)
#pragma unroll
        for (int k = 0; k < DVERTEX_WORDS; k++) {
            r[DPATH_HEAD_WORDS + v * DVERTEX_WORDS + k] = v < cam ? path[(size_t)(DPATH_HEAD_WORDS + v * DVERTEX_WORDS + k) * N + i] : 0.f;
            r[DPATH_HEAD_WORDS + (nV + v) * DVERTEX_WORDS + k] = v < lgt ? path[(size_t)(DPATH_HEAD_WORDS + (MAXD + v) * DVERTEX_WORDS + k) * N + i] : 0.f;
        }
}
LMC_D void UnpackPath(float *path, size_t N, int i, int nV, const float *r) {
#pragma unroll 4
    for (int k = 0; k < DPATH_HEAD_WORDS; k++) path[(size_t)k * N + i] = r[k];
    const int cam = ClampCount(r[12], nV), lgt = ClampCount(r[13], nV);
    for (int v = 0; v < cam; v++)
#pragma unroll
        for (int k = 0; k < DVERTEX_WORDS; k++) path[(size_t)(DPATH_HEAD_WORDS + v * DVERTEX_WORDS + k) * N + i] = r[DPATH_HEAD_WORDS + v * DVERTEX_WORDS + k];
    for (int v = 0; v < lgt; v++)
#pragma unroll
        for (int k = 0; k < DVERTEX_WORDS; k++) path[(size_t)(DPATH_HEAD_WORDS + (MAXD + v) * DVERTEX_WORDS + k) * N + i] = r[DPATH_HEAD_WORDS + (nV + v) * DVERTEX_WORDS + k];
}

__global__ void __launch_bounds__(64) k_ckpt_pack(ChainArrays A, Layout R, const float *h2Gauss, int first, int n, float *staging) {
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= n || first + m >= A.N) return;
    const size_t N = A.N;
    const int c = first + m, i = A.slotOf ? A.slotOf[c] : c;  // the chain, the slot it lives in
    float *r = staging + (size_t)m * R.Words();
    const int flags = A.flags[i];
    const uint64_t rs = A.rngState[i];
    const int nSplat = min(max(A.curSplatCount[i], 0), R.nS);
    r[CK_FLAGS] = __int_as_float(flags), r[CK_SAMPLEIDX] = __int_as_float(A.sampleIdx[i]), r[CK_NUMSAMPLES] = __int_as_float(A.numSamples[i]);
    r[CK_ADJREJECT] = __int_as_float(A.adjacentReject[i]), r[CK_SPLATCOUNT] = __int_as_float(nSplat), r[CK_NEXTKIND] = __int_as_float((int)A.nextKind[i]);
    r[CK_RNG_LO] = __int_as_float((int)(uint32_t)rs), r[CK_RNG_HI] = __int_as_float((int)(uint32_t)(rs >> 32));
    const int ticked = A.rngTicked[i];  // the extension table travels only once the stream has ticked: until then it is a function of the chain's seed (drng.h)
    r[CK_RNG_TICKED] = __int_as_float(ticked);
    r[CK_SCORESUM] = A.scoreSum[i], r[CK_LASTSCORESUM] = A.lastScoreSum[i], r[CK_LASTSCORE] = A.lastScore[i], r[CK_PATHWEIGHT] = A.pathWeight[i];
    r[CK_INITSCORESUM] = A.initScoreSum[c];  // the init arrays are indexed by chain, not by slot (dchain.h ResetToInitState)
    r[CK_INITSCORESUM + 1] = 0.f, r[CK_INITSCORESUM + 2] = 0.f;
    for (int k = 0; k < 64; k++) r[R.Tab() + k] = ticked ? __int_as_float((int)A.rngTab[(size_t)i * 64 + k]) : 0.f;
    PackPath(CurPathBuf(A, flags), N, i, R.nV, r + R.Path());
#pragma unroll
    for (int k = 0; k < CONTRIB_WORDS; k++) r[R.Contrib() + k] = A.curContrib[(size_t)k * N + i];
    for (int k = 0; k < R.nS * SPLAT_WORDS; k++) r[R.Splats() + k] = k < nSplat * SPLAT_WORDS ? A.curSplat[(size_t)k * N + i] : 0.f;
    for (int v = 0; v < 7; v++) {  // zero by the invariant unless F_BUFFERED and F_VDIRTY (dchain.h ClearBuffered): copied as they are
        const float *src = VectorBase(A, v);
#pragma unroll 4
        for (int k = 0; k < MAXPSS; k++) r[R.Vectors() + v * MAXPSS + k] = src[(size_t)k * N + i];
    }
    {
        const bool has = HasStoredGaussian(flags);
        const float *G = CurGaussBuf(A, flags);
#pragma unroll 4
        for (int k = 0; k < GAUSS_WORDS; k++) r[R.Gauss() + k] = has ? G[(size_t)k * N + i] : 0.f;
    }
    PackPath(A.initPath, N, c, R.nV, r + R.InitPath());
#pragma unroll
    for (int k = 0; k < CONTRIB_WORDS; k++) r[R.InitContrib() + k] = A.initContrib[(size_t)k * N + c];
    if (R.sampleCache) {
        PackPath(A.chPath, N, i, R.nV, r + R.ChPath());
#pragma unroll
        for (int k = 0; k < CONTRIB_WORDS; k++) r[R.ChContrib() + k] = A.chContrib[(size_t)k * N + i];
    }
    if (R.h2mc) {  // the state's dense Gaussian: the buffer F_GSEL selects (h2gauss.hip)
        const bool has = (flags & F_GAUSS) != 0;
        const float *G = h2Gauss + ((flags & F_GSEL) ? N * H2_GAUSS_AOS : (size_t)0) + (size_t)i * H2_GAUSS_AOS;
        for (int k = 0; k < H2_GAUSS_AOS; k++) r[R.H2Gauss() + k] = has ? G[k] : 0.f;
    }
}

__global__ void __launch_bounds__(64) k_ckpt_unpack(ChainArrays A, Layout R, float *h2Gauss, int first, int n, const float *staging) {
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= n || first + m >= A.N) return;
    const size_t N = A.N;
    const int i = first + m;  // slot = chain
    const float *r = staging + (size_t)m * R.Words();
    const int flags = __float_as_int(r[CK_FLAGS]);
    const int nSplat = min(max(__float_as_int(r[CK_SPLATCOUNT]), 0), R.nS);
    A.flags[i] = flags, A.sampleIdx[i] = __float_as_int(r[CK_SAMPLEIDX]), A.numSamples[i] = __float_as_int(r[CK_NUMSAMPLES]);
    A.adjacentReject[i] = __float_as_int(r[CK_ADJREJECT]), A.curSplatCount[i] = nSplat, A.nextKind[i] = (unsigned char)__float_as_int(r[CK_NEXTKIND]);
    A.rngState[i] = (uint64_t)(uint32_t)__float_as_int(r[CK_RNG_LO]) | ((uint64_t)(uint32_t)__float_as_int(r[CK_RNG_HI]) << 32);
    const int ticked = __float_as_int(r[CK_RNG_TICKED]);
    A.rngTicked[i] = (unsigned char)(ticked != 0);
    A.scoreSum[i] = r[CK_SCORESUM], A.lastScoreSum[i] = r[CK_LASTSCORESUM], A.lastScore[i] = r[CK_LASTSCORE], A.pathWeight[i] = r[CK_PATHWEIGHT];
    A.initScoreSum[i] = r[CK_INITSCORESUM];
    A.pushDim[i] = 0;
    if (ticked)
        for (int k = 0; k < 64; k++) A.rngTab[(size_t)i * 64 + k] = (uint32_t)__float_as_int(r[R.Tab() + k]);
    UnpackPath(CurPathBuf(A, flags), N, i, R.nV, r + R.Path());
#pragma unroll
    for (int k = 0; k < CONTRIB_WORDS; k++) A.curContrib[(size_t)k * N + i] = r[R.Contrib() + k];
    for (int k = 0; k < nSplat * SPLAT_WORDS; k++) A.curSplat[(size_t)k * N + i] = r[R.Splats() + k];
    for (int v = 0; v < 7; v++) {
        float *dst = VectorBase(A, v);
#pragma unroll 4
        for (int k = 0; k < MAXPSS; k++) dst[(size_t)k * N + i] = r[R.Vectors() + v * MAXPSS + k];
    }
    if (HasStoredGaussian(flags)) {
        float *G = CurGaussBuf(A, flags);
#pragma unroll 4
        for (int k = 0; k < GAUSS_WORDS; k++) G[(size_t)k * N + i] = r[R.Gauss() + k];
    }
    UnpackPath(A.initPath, N, i, R.nV, r + R.InitPath());
#pragma unroll
    for (int k = 0; k < CONTRIB_WORDS; k++) A.initContrib[(size_t)k * N + i] = r[R.InitContrib() + k];
    if (R.sampleCache) {
        UnpackPath(A.chPath, N, i, R.nV, r + R.ChPath());
#pragma unroll
        for (int k = 0; k < CONTRIB_WORDS; k++) A.chContrib[(size_t)k * N + i] = r[R.ChContrib() + k];
    }
    if (R.h2mc && (flags & F_GAUSS)) {
        float *G = h2Gauss + ((flags & F_GSEL) ? N * H2_GAUSS_AOS : (size_t)0) + (size_t)i * H2_GAUSS_AOS;
        for (int k = 0; k < H2_GAUSS_AOS; k++) G[k] = r[R.H2Gauss() + k];
    }
}

}  // namespace
}  // namespace lmcd

using namespace lmcd;

static Layout MakeLayout(int maxDepth, bool sampleCache, bool h2mc) {
    Layout R;
    R.nV = std::min(MAXD, std::max(maxDepth, 1));
    R.nS = std::min(MAXCONTRIB, (maxDepth + 1) * (maxDepth + 2) / 2);  // the relocation's bounds (relocate.hip MakeRecordLayout)
    R.sampleCache = sampleCache ? 1 : 0, R.h2mc = h2mc ? 1 : 0;
    return R;
}
size_t CkptRecordWords(int maxDepth, bool sampleCache, bool h2mc) { return (size_t)MakeLayout(maxDepth, sampleCache, h2mc).Words(); }
void LaunchCkptPack(const ChainArrays &A, int maxDepth, bool sampleCache, const float *h2Gauss, int first, int n, float *staging, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ckpt_pack, dim3((n + 63) / 64), dim3(64), 0, s, A, MakeLayout(maxDepth, sampleCache, h2Gauss != nullptr), h2Gauss, first, n, staging);
}
void LaunchCkptUnpack(const ChainArrays &A, int maxDepth, bool sampleCache, float *h2Gauss, int first, int n, const float *staging, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ckpt_unpack, dim3((n + 63) / 64), dim3(64), 0, s, A, MakeLayout(maxDepth, sampleCache, h2Gauss != nullptr), h2Gauss, first, n, staging);
}
