// Test probes of the bookkeeping launches (include/lmc_abi.h "probes used by the parity tests"): the inclusive scan, the 24-bit radix sort, the work
// lists and their counting sorts, the cache-push pack and the plan of a relocation, each on caller-given arrays.  Host code only: every probe
// allocates device buffers, copies the arrays in, calls the launch function of device/kernels.hip / device/relocate.hip that the renderer calls,
// unchanged, on a stream of its own, waits and copies the results back.  The stand-in ChainArrays hold only the fields the launch reads.
// What a launch would write out of bounds on inconsistent arguments (a list entry beyond N, a bin count that disagrees with the list) is refused here.
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
