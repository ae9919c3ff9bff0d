// Chain diagnostics (host/chaindiag.cpp; include/lmc_abi.h "Chain diagnostics"): what a chain looks like between two steps, read on the device
// instead of downloading every path buffer (lmc_chain_summary), and how the steps split over launch kinds and techniques.
//   k_latch_kind   head of a lock step: the launch that is about to run every chain, per rank-local CHAIN id (one byte per chain).  Read from the
//                  step's work lists themselves, not from A.nextKind: k_build_lists turns a generic entry whose cache became ready into a lean
//                  one (kernels.hip, leanDims) without writing A.nextKind back, and A.stepKind only exists with relocation on.  The lists are what
//                  the three launches run; keyed by chain, neither the per-step relocation nor the full re-sort has to be reasoned about.
//   k_chain_rows   one wave per requested chain -> one row of LMC_ROW_WORDS words: the 16 header words of lmc_chain_summary, the first 24 primary
//                  samples in the summary's order, the latched kind, adjacentReject, the flags word
//   k_step_table   behind a lock step, all N slots: chain-steps and accepted chain-steps per (launch kind, technique of the state after the step)
// All three read chain state only.  Integers and copied words: nothing here rounds.
#include "kernels.h"

namespace lmcd {
namespace {

constexpr int ROW_WORDS = 48;        // include/lmc_abi.h LMC_ROW_WORDS
constexpr int ROW_PSS = 24;          // words 16 .. 39
constexpr int TABLE_TECH = 13;       // c, l = 0 .. MAXD
constexpr int TABLE_KEYS = 3 * TABLE_TECH * TABLE_TECH;
static_assert(TABLE_TECH == MAXD + 1, "the step table holds every technique of a DPath");
// word offsets inside a DPath (dpath.h): the state arrays are word-major (word w of slot i at w * N + i)
enum : int { PW_TIME = 0, PW_SCREEN = 1, PW_LGTPOS = 3, PW_CAMDEPTH = 10, PW_LGTDEPTH = 11, PW_CAMCOUNT = 12, PW_LGTCOUNT = 13, VW_RND = 3, VW_DIRRND = 10 };
LMC_D int CamVertex(int d) { return DPATH_HEAD_WORDS + d * DVERTEX_WORDS; }
LMC_D int LgtVertex(int d) { return DPATH_HEAD_WORDS + (MAXD + d) * DVERTEX_WORDS; }

__global__ void k_latch_kind(ChainArrays A, const int *large, const int *generic, const int *lean, const int *counts, unsigned char *kindOf) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.N) return;
    const int *const lists[3] = {large, generic, lean};
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (t < counts[k]) {
            const int slot = lists[k][t];
            if (slot >= 0 && slot < A.N) kindOf[A.chainId ? A.chainId[slot] : slot] = (unsigned char)(k + 1);
        }
}

// Which word of the staged path is primary sample q of the state (the order of lmc_chain_summary, i.e. GetPathPss, dpath.h); -1: the state has fewer.
// q < ROW_PSS keeps every vertex index below MAXD whatever the counts say.
LMC_D int PssSource(const float *sP, int q) {
    const int camDepth = __float_as_int(sP[PW_CAMDEPTH]), lgtDepth = __float_as_int(sP[PW_LGTDEPTH]);
    const int camCount = __float_as_int(sP[PW_CAMCOUNT]), lgtCount = __float_as_int(sP[PW_LGTCOUNT]);
    const int nLight = lgtDepth > 1 ? 4 + 2 * max(lgtCount - 1, 0) : 0;
    if (q < nLight) return q < 4 ? PW_LGTPOS + q : LgtVertex((q - 4) >> 1) + VW_RND + ((q - 4) & 1);
    if (lgtDepth > 1 && camDepth == 1) return -1;
    const int t = q - nLight;
    if (t < 2) return PW_SCREEN + t;
    const int d = (t - 2) >> 1, e = (t - 2) & 1;
    if (d < camCount - 1) return CamVertex(d) + VW_RND + e;
    if (d == camCount - 1 && lgtDepth == 1) return CamVertex(d) + VW_DIRRND + e;
    return -1;
}

// which: 0 = current states (through A.slotOf, the chain's current path buffer by F_SEL), 1 = init states (indexed by chain).  ids: rank-local chain
// ids in [0, N), checked by the host.  kindOf: the latch (nullptr: word 40 = -1, outside a trace).
__global__ void __launch_bounds__(64) k_chain_rows(ChainArrays A, int which, const int *ids, int n, const unsigned char *kindOf, float *out) {
    constexpr int ROUNDS = (DPATH_WORDS + 63) / 64;
    __shared__ float sP[ROUNDS * 64];
    const int lane = threadIdx.x, r = blockIdx.x;
    if (r >= n) return;
    const size_t N = (size_t)A.N;
    const int chain = ids[r];
    const int i = which == 0 && A.slotOf ? A.slotOf[chain] : chain;
    const int fl = which == 0 ? A.flags[i] : 0;
    const float *path = which == 0 ? CurPathBuf(A, fl) : A.initPath;
    float v[ROUNDS];
#pragma unroll
    for (int j = 0; j < ROUNDS; j++) {  // all loads in flight before the first is used
        const int w = lane + 64 * j;
        v[j] = w < DPATH_WORDS ? path[(size_t)w * N + i] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < ROUNDS; j++) sP[lane + 64 * j] = v[j];
    __syncthreads();
    if (lane >= ROW_WORDS) return;
    const float *con = which == 0 ? A.curContrib : A.initContrib;
    float o = 0.f;
    if (lane == 0) o = (which == 0 && (fl & F_VALID)) ? 1.f : 0.f;
    else if (lane == 1 || lane == 2) o = (float)__float_as_int(con[(size_t)(lane - 1) * N + i]);
    else if (lane == 3 || lane == 4) o = con[(size_t)(lane + 4) * N + i];
    else if (lane == 5) o = (which == 0 ? A.scoreSum : A.initScoreSum)[i];
    else if (lane == 6) o = sP[PW_TIME];
    else if (lane == 7) o = (fl & F_GAUSS) ? 1.f : 0.f;
    else if (lane == 8) o = (fl & F_BUFFERED) ? 1.f : 0.f;
    else if (lane == 9) o = which == 0 ? (float)A.sampleIdx[i] : 0.f;
    else if (lane < 15) o = con[(size_t)(lane - 8) * N + i];
    else if (lane == 15) o = which == 0 ? (float)A.curSplatCount[i] : 0.f;
    else if (lane < 16 + ROW_PSS) {
        const int src = PssSource(sP, lane - 16);
        o = src >= 0 ? sP[src] : 0.f;
    } else if (which == 0) {
        if (lane == 40) o = kindOf ? (float)kindOf[chain] : -1.f;
        else if (lane == 41) o = (float)A.adjacentReject[i];
        else if (lane == 42) o = (float)fl;
    }
    out[(size_t)r * ROW_WORDS + lane] = o;
}

// Slots in blocks of 256.  Relocated slots are sorted by technique, so most lanes of a wave share a key: a wave first sums per key (leader's key,
// ballot of the lanes that hold it, popcounts -- the match-by-key rounds of mc.hip), then adds to the block's LDS bins; the non-zero bins go to the
// table as 64-bit atomics.  table: [3][13][13][2] = [kind - 1][c][l][steps | accepted].
__global__ void __launch_bounds__(256) k_step_table(ChainArrays A, const unsigned char *kindOf, unsigned long long *table) {
    __shared__ unsigned sBin[TABLE_KEYS * 2];
    for (int b = threadIdx.x; b < TABLE_KEYS * 2; b += 256) sBin[b] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const size_t N = (size_t)A.N;
    int key = -1;
    bool accepted = false;
    if (i < A.N) {
        const int kind = kindOf[A.chainId ? A.chainId[i] : i];
        const int c = __float_as_int(A.curContrib[i]), l = __float_as_int(A.curContrib[N + i]);
        if (kind >= 1 && kind <= 3 && c >= 0 && c < TABLE_TECH && l >= 0 && l < TABLE_TECH) {
            key = (kind - 1) * TABLE_TECH * TABLE_TECH + c * TABLE_TECH + l;
            accepted = A.adjacentReject[i] == 0;
        }
    }
    unsigned long long pending = __ballot(key >= 0);
    for (int round = 0; pending && round < 4; round++) {
        const int leader = __ffsll((long long)pending) - 1;
        const int lk = __shfl(key, leader);
        const bool mine = key == lk;
        const unsigned long long group = __ballot(mine), acc = __ballot(mine && accepted);
        if (lane == leader) {
            atomicAdd(&sBin[lk * 2], (unsigned)__popcll(group));
            if (acc) atomicAdd(&sBin[lk * 2 + 1], (unsigned)__popcll(acc));
        }
        if (mine) key = -1;
        pending &= ~group;
    }
    if (key >= 0) {  // what four rounds left over
        atomicAdd(&sBin[key * 2], 1u);
        if (accepted) atomicAdd(&sBin[key * 2 + 1], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < TABLE_KEYS * 2; b += 256) {
        const unsigned n = sBin[b];
        if (n) atomicAdd(&table[b], (unsigned long long)n);
    }
}

// The pending splat lists of n chosen chains (lmc_chain_splats), one lane per chain: counts[j] = the list length of chain ids[j] (through A.slotOf),
// out[(j * cap + k) * 6 ..] = x, y, r, g, b of entry k as stored and its label c * 16 + l (labels: the layered film's array, by chain id; nullptr: -1).
// Entries from min(length, cap) on are not written.  ids: rank-local chain ids in [0, N), checked by the host.
__global__ void __launch_bounds__(64) k_chain_splats(ChainArrays A, const unsigned char *labels, const int *ids, int n, int cap, float *out, int *counts) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int chain = ids[j];
    const int i = A.slotOf ? A.slotOf[chain] : chain;
    const size_t N = A.N;
    const int len = A.curSplatCount[i];
    counts[j] = len;
    const int m = len < cap ? (len < 0 ? 0 : len) : cap;
    for (int k = 0; k < m; k++) {
        float *o = out + ((size_t)j * cap + k) * 6;
        for (int w = 0; w < SPLAT_WORDS; w++) o[w] = A.curSplat[((size_t)k * SPLAT_WORDS + w) * N + i];
        o[5] = labels ? (float)labels[(size_t)k * N + chain] : -1.0f;
    }
}

}  // namespace
}  // namespace lmcd

using namespace lmcd;

void LaunchChainSplats(const ChainArrays &A, const unsigned char *labels, const int *ids, int n, int cap, float *out, int *counts, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_chain_splats, dim3((n + 63) / 64), dim3(64), 0, s, A, labels, ids, n, cap, out, counts);
}
void LaunchLatchKind(const ChainArrays &A, const int *large, const int *generic, const int *lean, const int *counts, unsigned char *kindOf, hipStream_t s) {
    if (A.N <= 0) return;
    (void)hipMemsetAsync(kindOf, 0, (size_t)A.N, s);  // a chain in no list does not step
    hipLaunchKernelGGL(k_latch_kind, dim3((A.N + 255) / 256), dim3(256), 0, s, A, large, generic, lean, counts, kindOf);
}
void LaunchChainRows(const ChainArrays &A, int which, const int *ids, int n, const unsigned char *kindOf, float *out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_chain_rows, dim3(n), dim3(64), 0, s, A, which, ids, n, kindOf, out);
}
void LaunchStepTable(const ChainArrays &A, const unsigned char *kindOf, unsigned long long *table, hipStream_t s) {
    if (A.N <= 0) return;
    hipLaunchKernelGGL(k_step_table, dim3((A.N + 255) / 256), dim3(256), 0, s, A, kindOf, table);
}
