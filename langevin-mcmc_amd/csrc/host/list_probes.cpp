// Test probes of the bookkeeping launches (include/lmc_abi.h "probes used by the parity tests"): the inclusive scan, the 24-bit radix sort, the work
// lists and their counting sorts, the cache-push pack and the plan of a relocation, each on caller-given arrays.  Host code only: every probe
// allocates device buffers, copies the arrays in, calls the launch function of device/kernels.hip / device/relocate.hip that the renderer calls,
// unchanged, on a stream of its own, waits and copies the results back.  The stand-in ChainArrays hold only the fields the launch reads.
// What a launch would write out of bounds on inconsistent arguments (a list entry beyond N, a bin count that disagrees with the list) is refused here.
// At the end: the three wave-cooperative derivative launches that CONSUME a stage's bins (k_mala_grad, k_h2_hess, k_h2_gauss) on a caller-given work list.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/lmc_abi.h"
#include "../device/kernels.h"
#include "../device/dh2coop.h"
#include "../device/dh2mc.h"
#include "hostutil.h"

using namespace lmcd;

static_assert(LMC_PROBE_BINS == H2_NBINS, "include/lmc_abi.h: LMC_PROBE_BINS is the number of bins of a pipeline stage");
static_assert(LMC_PROBE_CACHE_ROWS == PSS_MAX_SIZE, "include/lmc_abi.h: LMC_PROBE_CACHE_ROWS is the row count of a cache dim");
static_assert(PSS_MAX_LENGTH == 12 && CACHE_SLOTS == 4, "lmc_cache_push_probe lays its rows out for the dims 6, 8, 10, 12");

namespace {

template <class T>
struct Buf {  // device array of at least one element (unlike hostutil.h's DevBuf never a null pointer, and it has Fill)
    T *p = nullptr;
    size_t n = 0;
    Buf() {}
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() {
        if (p) (void)hipFree(p);
    }
    void Alloc(size_t count) {
        n = count;
        HIP_CHECK(hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T)));
    }
    void Fill(size_t count, T value) { Upload(std::vector<T>(count, value)); }
    void Upload(const std::vector<T> &v) { Upload(v.data(), v.size()); }
    void Upload(const T *v, size_t count) {
        Alloc(count);
        if (count) HIP_CHECK(hipMemcpy(p, v, count * sizeof(T), hipMemcpyHostToDevice));
    }
    void Download(T *out, size_t count) const {
        if (count) HIP_CHECK(hipMemcpy(out, p, count * sizeof(T), hipMemcpyDeviceToHost));
    }
    std::vector<T> Download() const {
        std::vector<T> v(n);
        Download(v.data(), n);
        return v;
    }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw std::runtime_error("no HIP device available: the MI355X back end has no CPU fallback");
        HIP_CHECK(hipSetDevice(0));
        HIP_CHECK(hipStreamCreate(&s));
    }
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
    void Finish() {  // a launch that was refused shows up here, one that failed at the synchronisation
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(s));
    }
};

void Require(bool ok, const char *what) {
    if (!ok) throw std::runtime_error(what);
}
constexpr int kSentinel = LMC_PROBE_SENTINEL;

}  // namespace

extern "C" {

int lmc_scan_probe(int n, const int *in, int *out) {
    LMC_TRY
    Require(n >= 1 && in && out, "lmc_scan_probe: n >= 1 and both arrays are required");
    Stream st;
    Buf<int> v, sums;
    v.Upload(in, n), sums.Fill((size_t)n / 2048 + 1, kSentinel);
    LaunchInclusiveScan(v.p, n, sums.p, st.s);
    st.Finish();
    v.Download(out, n);
    return 0;
    LMC_CATCH(-1)
}

int lmc_radix_sort_probe(int n, int n_max, const unsigned *keys, int *out_vals, unsigned *out_keys) {
    LMC_TRY
    Require(n_max >= 1 && n >= 0 && n <= n_max && keys && out_vals && out_keys, "lmc_radix_sort_probe: 0 <= n <= n_max, n_max >= 1 and all arrays are required");
    Stream st;
    const size_t nb = RelocSortBlocks(n_max);
    Buf<unsigned> k0, k1;
    Buf<int> v0, v1, hist, sums, outV, count;
    k0.Upload(keys, n_max), k1.Fill(n_max, (unsigned)kSentinel);
    v0.Fill(n_max, kSentinel), v1.Fill(n_max, kSentinel), outV.Fill(n_max, kSentinel);
    hist.Fill(256 * nb, kSentinel), sums.Fill(256 * nb / 2048 + 2, kSentinel);  // the sizes host/context.cpp allocates
    count.Upload(&n, 1);
    const RelocSortBuffers W{{k0.p, k1.p}, {v0.p, v1.p}, hist.p, sums.p};
    LaunchRadixSort24(W, count.p, n_max, outV.p, st.s);
    st.Finish();
    outV.Download(out_vals, n_max), k1.Download(out_keys, n_max);
    return 0;
    LMC_CATCH(-1)
}

int lmc_sort_by_technique_probe(int n_chains, const unsigned char *next_kind, int n_list, const int *list, int max_entries, int *out) {
    LMC_TRY
    Require(n_chains >= 1 && next_kind && n_list >= 0 && max_entries >= n_list && (n_list == 0 || (list && out)), "lmc_sort_by_technique_probe: bad arguments");
    for (int i = 0; i < n_list; i++) Require(list[i] >= 0 && list[i] < n_chains, "lmc_sort_by_technique_probe: list entry out of range");
    Stream st;
    Buf<unsigned char> nk;
    Buf<int> in, o, count, hist;
    nk.Upload(next_kind, n_chains), in.Upload(list, n_list), o.Fill(max_entries, kSentinel), count.Upload(&n_list, 1);
    hist.Fill((size_t)64 * ((max_entries + 2047) / 2048), kSentinel);
    LaunchSortByTechnique(nk.p, in.p, o.p, count.p, hist.p, max_entries, st.s);
    st.Finish();
    const std::vector<int> all = o.Download();
    for (int i = n_list; i < max_entries; i++) Require(all[i] == kSentinel, "lmc_sort_by_technique_probe: the launch wrote beyond the list's count");
    if (n_list) memcpy(out, all.data(), (size_t)n_list * sizeof(int));
    return 0;
    LMC_CATCH(-1)
}

int lmc_build_lists_probe(int N, const unsigned char *next_kind, int sort_plain, unsigned lean_dims, int want_step_kind, int *out_large, int *out_generic,
                          int *out_plain, int *out_counts, unsigned char *out_step_kind) {
    LMC_TRY
    Require(N >= 1 && next_kind && sort_plain >= 0 && sort_plain <= 3 && out_large && out_generic && out_plain && out_counts && (!want_step_kind || out_step_kind),
            "lmc_build_lists_probe: bad arguments");
    Stream st;
    Buf<unsigned char> nk, sk;
    Buf<int> large, generic, plain, counts;
    nk.Upload(next_kind, N), sk.Fill((size_t)N + 4, (unsigned char)0xee);
    large.Fill(N, kSentinel), generic.Fill(N, kSentinel), plain.Fill(N, kSentinel), counts.Fill(4, 0);
    ChainArrays A;
    memset(&A, 0, sizeof(A));
    A.N = N, A.nextKind = nk.p, A.stepKind = want_step_kind ? sk.p : nullptr;
    LaunchBuildLists(A, NextLists{large.p, generic.p, plain.p, counts.p}, sort_plain, lean_dims, st.s);
    st.Finish();
    large.Download(out_large, N), generic.Download(out_generic, N), plain.Download(out_plain, N), counts.Download(out_counts, 3);
    if (want_step_kind) sk.Download(out_step_kind, N);
    return 0;
    LMC_CATCH(-1)
}

int lmc_bins_compact_probe(int N, const int *bin_of, const int *count, int n_list, const int *list, int grid_blocks, int *out_items, int *out_start) {
    LMC_TRY
    Require(N >= 1 && bin_of && count && n_list >= 0 && n_list <= N && (n_list == 0 || list) && grid_blocks >= 1 && grid_blocks <= 65536 && out_items && out_start,
            "lmc_bins_compact_probe: bad arguments");
    // the scatter trusts the counts: they must be the list's own
    std::vector<int> seen(H2_NBINS, 0), padded(H2_COUNT_WORDS, 0);
    for (int j = 0; j < n_list; j++) {
        Require(list[j] >= 0 && list[j] < N, "lmc_bins_compact_probe: list entry out of range");
        const int b = bin_of[list[j]];
        Require(b >= -1 && b < H2_NBINS, "lmc_bins_compact_probe: bin out of range");
        if (b >= 0) seen[b]++;
    }
    for (int b = 0; b < H2_NBINS; b++) Require(seen[b] == count[b], "lmc_bins_compact_probe: count[] is not the list's number of entries per bin"), padded[b] = count[b];
    Stream st;
    Buf<int> items, cnt, start, cursor, binOf, dList, dN;
    items.Fill(N, kSentinel), cnt.Upload(padded), start.Fill(H2_COUNT_WORDS, kSentinel), cursor.Fill(H2_COUNT_WORDS, kSentinel), binOf.Upload(bin_of, N);
    dList.Upload(list, n_list), dN.Upload(&n_list, 1);
    LaunchBinsCompact(H2Bins{items.p, cnt.p, start.p, cursor.p, binOf.p}, dList.p, dN.p, grid_blocks, st.s);
    st.Finish();
    items.Download(out_items, N), start.Download(out_start, H2_NBINS);
    return 0;
    LMC_CATCH(-1)
}

int lmc_split_list_probe(int n_list, const int *list, int parts, int stride, int grid_blocks, int *out_sub, int *out_sub_count) {
    LMC_TRY
    Require(n_list >= 0 && (n_list == 0 || list) && parts >= 1 && parts <= 4 && grid_blocks >= 1 && grid_blocks <= 65536 && out_sub && out_sub_count,
            "lmc_split_list_probe: bad arguments");
    const int groups = (n_list + 63) / 64;  // a part receives at most ceil(groups / parts) groups of 64
    Require(stride >= 1 && stride >= (groups + parts - 1) / parts * 64, "lmc_split_list_probe: stride too small for the list");
    Stream st;
    Buf<int> dList, dN, sub, subCount;
    dList.Upload(list, n_list), dN.Upload(&n_list, 1), sub.Fill((size_t)parts * stride, kSentinel), subCount.Fill(parts, kSentinel);
    LaunchSplitList(dList.p, dN.p, parts, sub.p, stride, subCount.p, grid_blocks, st.s);
    st.Finish();
    sub.Download(out_sub, (size_t)parts * stride), subCount.Download(out_sub_count, parts);
    return 0;
    LMC_CATCH(-1)
}

int lmc_cache_push_probe(int N, const int *push_dim, const float *push_data, const int *slot_of, const int *initial_counts, float *out_rows, float *out_weights,
                         int *out_counts, int *out_push_dim) {
    LMC_TRY
    Require(N >= 1 && push_dim && push_data && initial_counts && out_rows && out_weights && out_counts && out_push_dim, "lmc_cache_push_probe: bad arguments");
    for (int sl = 0; sl < CACHE_SLOTS; sl++) Require(initial_counts[sl] >= 0 && initial_counts[sl] <= PSS_MAX_SIZE, "lmc_cache_push_probe: initial count out of range");
    if (slot_of) {
        std::vector<char> hit(N, 0);
        for (int i = 0; i < N; i++) {
            Require(slot_of[i] >= 0 && slot_of[i] < N && !hit[slot_of[i]], "lmc_cache_push_probe: slot_of is not a permutation");
            hit[slot_of[i]] = 1;
        }
    }
    constexpr int ROW = 3 * PSS_MAX_LENGTH + 1;
    std::vector<float> soa((size_t)(3 * MAXPSS + 1) * N, 0.f);  // A.pushData: [word][slot], pss / v1 / v2 at words 0 / MAXPSS / 2 MAXPSS, the weight last
    for (int i = 0; i < N; i++) {
        const float *r = push_data + (size_t)i * ROW;
        for (int a = 0; a < 3; a++)
            for (int k = 0; k < PSS_MAX_LENGTH; k++) soa[(size_t)(a * MAXPSS + k) * N + i] = r[a * PSS_MAX_LENGTH + k];
        soa[(size_t)(3 * MAXPSS) * N + i] = r[3 * PSS_MAX_LENGTH];
    }
    uint32_t nanBits = 0x7fc0beefu;
    float untouched;
    memcpy(&untouched, &nanBits, 4);
    Stream st;
    Buf<int> dDim, dSlotOf, dCount, stageCounts;
    Buf<float> dData, rows[CACHE_SLOTS][3], weight[CACHE_SLOTS];
    Buf<unsigned long long> tiles;
    dDim.Upload(push_dim, N), dData.Upload(soa), dCount.Upload(initial_counts, CACHE_SLOTS), stageCounts.Fill(16, kSentinel);
    if (slot_of) dSlotOf.Upload(slot_of, N);
    tiles.Fill((size_t)(N + 1023) / 1024, ~0ull);
    CachePushTargets T;
    memset(&T, 0, sizeof(T));
    for (int sl = 0; sl < CACHE_SLOTS; sl++) {
        const int dim = 6 + 2 * sl;
        for (int a = 0; a < 3; a++) rows[sl][a].Fill((size_t)PSS_MAX_SIZE * dim, untouched);
        weight[sl].Fill(PSS_MAX_SIZE, untouched);
        T.pss[sl] = rows[sl][0].p, T.v1[sl] = rows[sl][1].p, T.v2[sl] = rows[sl][2].p, T.weight[sl] = weight[sl].p;
    }
    T.count = dCount.p;
    ChainArrays A;
    memset(&A, 0, sizeof(A));
    A.N = N, A.pushDim = dDim.p, A.pushData = dData.p, A.slotOf = slot_of ? dSlotOf.p : nullptr;
    LaunchCachePush(A, T, tiles.p, stageCounts.p, st.s);
    st.Finish();
    for (int v : stageCounts.Download()) Require(v == 0, "lmc_cache_push_probe: the launch did not zero the stage's row counts");
    for (size_t k = 0; k < (size_t)CACHE_SLOTS * 3 * PSS_MAX_SIZE * PSS_MAX_LENGTH; k++) out_rows[k] = untouched;
    for (int sl = 0; sl < CACHE_SLOTS; sl++) {
        const int dim = 6 + 2 * sl;
        for (int a = 0; a < 3; a++) {
            const std::vector<float> r = rows[sl][a].Download();
            for (int row = 0; row < PSS_MAX_SIZE; row++)
                memcpy(out_rows + ((size_t)(sl * 3 + a) * PSS_MAX_SIZE + row) * PSS_MAX_LENGTH, r.data() + (size_t)row * dim, (size_t)dim * sizeof(float));
        }
        weight[sl].Download(out_weights + (size_t)sl * PSS_MAX_SIZE, PSS_MAX_SIZE);
    }
    dCount.Download(out_counts, CACHE_SLOTS), dDim.Download(out_push_dim, N);
    return 0;
    LMC_CATCH(-1)
}

int lmc_reloc_plan_probe(int N, const unsigned char *step_kind, const int *c, const int *l, const int *flags, const unsigned *placed_key, int without_gaussian_only,
                         int capacity, int skipped_before, int *out_count, int *out_members, int *out_sorted) {
    LMC_TRY
    Require(N >= 1 && step_kind && c && l && flags && placed_key && capacity >= 0 && out_count && out_members && out_sorted, "lmc_reloc_plan_probe: bad arguments");
    std::vector<float> contrib((size_t)2 * N);  // words 0 and 1 of A.curContrib: camera and light depth, as integers
    memcpy(contrib.data(), c, (size_t)N * 4), memcpy(contrib.data() + N, l, (size_t)N * 4);
    const int count0[2] = {kSentinel, skipped_before};
    Stream st;
    Buf<unsigned char> sk;
    Buf<float> con;
    Buf<int> fl, tileCount, tileHist, members, sorted, count;
    Buf<unsigned> placed;
    sk.Upload(step_kind, N), con.Upload(contrib), fl.Upload(flags, N), placed.Upload(placed_key, N);
    tileCount.Fill(RelocTiles(N) + 1, kSentinel), tileHist.Fill(RelocTiles(N) * 64, kSentinel);  // the sizes host/context.cpp allocates
    members.Fill(N, kSentinel), sorted.Fill(N, kSentinel), count.Upload(count0, 2);
    ChainArrays A;
    memset(&A, 0, sizeof(A));
    A.N = N, A.stepKind = sk.p, A.curContrib = con.p, A.flags = fl.p;
    const RelocBuffers B{placed.p, tileCount.p, tileHist.p, members.p, sorted.p, count.p, nullptr, capacity, false};
    LaunchRelocPlan(A, 6, B, without_gaussian_only != 0, st.s);
    st.Finish();
    count.Download(out_count, 2), members.Download(out_members, N), sorted.Download(out_sorted, N);
    return 0;
    LMC_CATCH(-1)
}

}  // extern "C"

// ---- the wave-cooperative derivative launches on a caller-given work list (device/dh2coop.h: bins, task table, grid-stride loop over the tasks)
namespace {

float Untouched() {
    const uint32_t bits = 0x7fc0beefu;
    float f;
    memcpy(&f, &bits, 4);
    return f;
}

// What the kernels trust: they index the records and the output rows by items[], and a task's LDS by the bin's technique.  fits(chain, technique):
// the chain's state is one of that technique; techArg names the arrays that say so.  Host only: runs before the first device call.
template <class Fits>
void RequireWorkList(const std::string &who, int N, int n_list, const int *items, const int *count, const int *start, int grid_blocks, Fits fits, const char *techArg) {
    auto fail = [&](const std::string &what) { throw std::runtime_error(who + ": " + what); };
    if (n_list < 1) fail("n_list = " + std::to_string(n_list) + ": a list needs at least one entry (n = 0 is not a call)");
    if (N < n_list) fail("N = " + std::to_string(N) + " is smaller than n_list = " + std::to_string(n_list));
    if (!items || !count || !start) fail("items, count and start are required");
    if (grid_blocks < 1 || grid_blocks > 4096) fail("grid_blocks = " + std::to_string(grid_blocks) + " is outside [1, 4096]");
    std::vector<char> listed(N, 0);
    for (int j = 0; j < n_list; j++) {
        if (items[j] < 0 || items[j] >= N) fail("items[" + std::to_string(j) + "] = " + std::to_string(items[j]) + " is outside [0, N)");
        if (listed[items[j]]) fail("items[" + std::to_string(j) + "] = " + std::to_string(items[j]) + " is listed twice");
        listed[items[j]] = 1;
    }
    std::vector<std::pair<long long, int>> ranges;  // (start, bin) of the bins that hold something
    for (int b = 0; b < H2_NBINS; b++) {
        if (count[b] < 0) fail("count[" + std::to_string(b) + "] = " + std::to_string(count[b]) + " is negative");
        if (count[b] == 0) continue;
        if (start[b] < 0 || (long long)start[b] + count[b] > n_list)
            fail("start[" + std::to_string(b) + "] = " + std::to_string(start[b]) + " with count " + std::to_string(count[b]) + " leaves [0, n_list)");
        ranges.emplace_back(start[b], b);
        for (int j = start[b]; j < start[b] + count[b]; j++)
            if (!fits(items[j], b / H2_NSIG))
                fail(std::string(techArg) + " of chain " + std::to_string(items[j]) + " (items[" + std::to_string(j) + "]) is not the technique of its bin " + std::to_string(b));
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t r = 1; r < ranges.size(); r++)
        if (ranges[r - 1].first + count[ranges[r - 1].second] > ranges[r].first)
            fail("start[" + std::to_string(ranges[r].second) + "] = " + std::to_string(start[ranges[r].second]) + " lies inside bin " + std::to_string(ranges[r - 1].second) + ": the bins overlap");
}

struct DeviceWorkList {  // items | count | start on the device, the two tables padded as the renderer's (H2_COUNT_WORDS)
    Buf<int> items, count, start;
    void Upload(int n_list, const int *it, const int *cnt, const int *st) {
        std::vector<int> c(H2_COUNT_WORDS, 0), s(H2_COUNT_WORDS, 0);
        std::copy(cnt, cnt + H2_NBINS, c.begin()), std::copy(st, st + H2_NBINS, s.begin());
        items.Upload(it, n_list), count.Upload(c), start.Upload(s);
    }
    H2Bins Bins() const { return H2Bins{items.p, count.p, start.p, nullptr, nullptr}; }
};

// N serialised states (dh2coop.h `rec`): [0, 2 L + 1) primary | c | l | vertParams, the rest zero
std::vector<float> PackRecords(int N, const float *primary, const int *c, const int *l, const float *vert) {
    std::vector<float> rec((size_t)N * H2_REC_WORDS, 0.f);
    for (int i = 0; i < N; i++) {
        float *r = rec.data() + (size_t)i * H2_REC_WORDS;
        memcpy(r + H2_REC_C, &c[i], 4), memcpy(r + H2_REC_L, &l[i], 4);
        if (H2TechIndex(c[i], l[i]) < 0) continue;  // (cannot be listed)
        const int L = std::max(c[i] + l[i] - 1, 2), V = 238 + 59 * (c[i] + l[i] - 3);
        memcpy(r, primary + (size_t)i * 17, (size_t)(2 * L + 1) * sizeof(float));
        memcpy(r + H2_REC_VP, vert + (size_t)i * LMC_PROBE_VERT_WORDS, (size_t)V * sizeof(float));
    }
    return rec;
}

// the body the gradient and the Hessian probe share: the launch takes (records, bins, N, scene, rows, grid, stream)
template <class Launch>
void RunRecordProbe(const char *who, int rowWords, Launch launch, int N, const float *primary, const int *c, const int *l, const float *vert, const float *scene38,
                    int n_list, const int *items, const int *count, const int *start, int grid_blocks, float *out) {
    Require(primary && c && l && vert && scene38 && out, (std::string(who) + ": primary, c, l, vert, scene38 and out are required").c_str());
    RequireWorkList(who, N, n_list, items, count, start, grid_blocks, [&](int i, int t) { return H2TechIndex(c[i], l[i]) == t; }, "(c, l)");
    Stream st;
    Buf<float> dRec, dOut;
    DeviceWorkList W;
    dRec.Upload(PackRecords(N, primary, c, l, vert)), dOut.Fill((size_t)N * rowWords, Untouched()), W.Upload(n_list, items, count, start);
    launch(dRec.p, W.Bins(), N, scene38, dOut.p, grid_blocks, st.s);
    st.Finish();
    dOut.Download(out, (size_t)N * rowWords);
}

}  // namespace

static_assert(LMC_PROBE_VERT_WORDS == 238 + 59 * 6 && H2_REC_VP + LMC_PROBE_VERT_WORDS <= H2_REC_WORDS, "include/lmc_abi.h: LMC_PROBE_VERT_WORDS is the longest vertParams (dh2coop.h)");
static_assert(MAXPSS >= 16, "the Gaussian probe lays out 16 offset words per chain");

extern "C" {

int lmc_mala_grad_list_probe(int N, const float *primary, const int *c, const int *l, const float *vert, const float *scene38, int n_list, const int *items,
                             const int *count, const int *start, int grid_blocks, float *out) {
    LMC_TRY
    RunRecordProbe("lmc_mala_grad_list_probe", MG_OUT_WORDS, LaunchMalaGrad, N, primary, c, l, vert, scene38, n_list, items, count, start, grid_blocks, out);
    return 0;
    LMC_CATCH(-1)
}

int lmc_h2_hess_list_probe(int N, const float *primary, const int *c, const int *l, const float *vert, const float *scene38, int n_list, const int *items,
                           const int *count, const int *start, int grid_blocks, float *out) {
    LMC_TRY
    RunRecordProbe("lmc_h2_hess_list_probe", H2_OUT_WORDS, LaunchH2Hess, N, primary, c, l, vert, scene38, n_list, items, count, start, grid_blocks, out);
    return 0;
    LMC_CATCH(-1)
}

int lmc_h2_gauss_list_probe(int N, const int *dim, const float *grad, const float *hess, const int *flags, const float *offset, int stage, float sigma, int n_list,
                            const int *items, const int *count, const int *start, int grid_blocks, float *gauss, float *px) {
    LMC_TRY
    const std::string who = "lmc_h2_gauss_list_probe";
    Require(dim && grad && hess && flags && offset && gauss && px, "lmc_h2_gauss_list_probe: dim, grad, hess, flags, offset, gauss and px are required");
    Require(stage == 0 || stage == 1, "lmc_h2_gauss_list_probe: stage must be 0 or 1");
    Require(sigma > 0.0f, "lmc_h2_gauss_list_probe: sigma must be positive");
    for (int i = 0; i < N; i++)
        if (dim[i] < 4 || dim[i] > 16 || (dim[i] & 1)) throw std::runtime_error(who + ": dim[" + std::to_string(i) + "] = " + std::to_string(dim[i]) + " is not even, 4 .. 16");
    RequireWorkList(who, N, n_list, items, count, start, grid_blocks, [&](int i, int t) { return H2TechDim(t) == dim[i]; }, "dim");  // (the launch reads a technique's dim alone)
    std::vector<float> hout((size_t)N * H2_OUT_WORDS, 0.f), off((size_t)MAXPSS * N, 0.f);
    for (int i = 0; i < N; i++) {
        memcpy(hout.data() + (size_t)i * H2_OUT_WORDS, grad + (size_t)i * 16, 16 * sizeof(float));
        memcpy(hout.data() + (size_t)i * H2_OUT_WORDS + H2_OUT_HESS, hess + (size_t)i * 256, (size_t)dim[i] * dim[i] * sizeof(float));
        for (int k = 0; k < dim[i]; k++) off[(size_t)k * N + i] = offset[(size_t)i * 16 + k];
    }
    Stream st;
    Buf<float> dHout, dOff, dGauss, dPx;
    Buf<int> dFlags;
    DeviceWorkList W;
    dHout.Upload(hout), dOff.Upload(off), dFlags.Upload(flags, N), W.Upload(n_list, items, count, start);
    dGauss.Fill(2 * (size_t)N * H2_GAUSS_AOS, Untouched()), dPx.Fill(N, Untouched());
    LaunchH2Gauss(W.Bins(), N, dHout.p, MakeH2MCParam(sigma), 0, dFlags.p, stage, dGauss.p, dOff.p, dPx.p, grid_blocks, st.s);
    st.Finish();
    dGauss.Download(gauss, 2 * (size_t)N * H2_GAUSS_AOS), dPx.Download(px, N);
    return 0;
    LMC_CATCH(-1)
}

int lmc_coop_plan_probe(int kernel, int tech, int *states_per_task, int *rec_words) {
    LMC_TRY
    Require(kernel >= 0 && kernel <= 2, "lmc_coop_plan_probe: kernel must be 0 (k_mala_grad), 1 (k_h2_hess) or 2 (k_h2_gauss)");
    Require(tech >= 0 && tech < H2_NTECH, "lmc_coop_plan_probe: tech is outside [0, 42)");
    Require(states_per_task && rec_words, "lmc_coop_plan_probe: both outputs are required");
    *states_per_task = kernel == 0 ? MalaGradStatesPerTask(tech) : kernel == 1 ? H2HessStatesPerTask(tech) : H2_GAUSS_STATES_PER_TASK;
    *rec_words = kernel == 2 ? H2_OUT_WORDS : H2RecWordsOfTech(tech);
    return 0;
    LMC_CATCH(-1)
}

}  // extern "C"
