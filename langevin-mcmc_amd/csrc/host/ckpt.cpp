// Checkpoint and resume (include/lmc_abi.h: lmc_checkpoint_*, lmc_group_checkpoint_*, lmc_checkpoint_info).  Host logic only: the records are packed
// and unpacked by device/checkpoint.hip, the chains set up and the next step's lists built by context.cpp (context.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/lmc_abi.h"
#include "../device/kernels.h"
#include "accel.h"
#include "context.h"
#include "hostutil.h"
#include "scene.h"

// One little-endian file (INTEGRATION.md "Checkpoint and resume"): header (magic, version, the fingerprint of what the states depend on, the job's
// shape, steps and seconds so far) | job-wide state, once (init results, the gradient caches' rows, counters, film) | one fixed-size record per
// chain of the JOB, in chain order (device/checkpoint.hip).  Nothing in it depends on the slots the chains lived in, on the schedule that ran
// them or on how many members of an in-process group held them, so it loads into one context or into a group of any size.
namespace {
constexpr char kCkptMagic[8] = {'L', 'M', 'C', 'C', 'K', 'P', 'T', '\n'};
// version 1: the film section is W*H*3 floats (byte for byte what every earlier build wrote); version 2: the header's filmFormat is 1 and the film
// section is W*H*3 signed 64-bit fixed-point words (exact mode, INTEGRATION.md "Exact film").  Float-mode renders keep writing version 1.
constexpr uint32_t kCkptVersion = 1, kCkptVersionExact = 2;
constexpr int32_t kFilmFloat32 = 0, kFilmFixed64 = 1;
const char *FilmFormatName(int32_t f) { return f == kFilmFixed64 ? "fixed-point int64 (film_exact=1)" : "float32 (film_exact=0)"; }
// Chains per chunk of the record stream (device staging -> pinned host -> file): as many as fit kCkptChunkBytes.  Neither side ever holds a second
// copy of the population; 64 MiB is where the per-chunk costs (a launch, a copy, a stream wait) have vanished against the copy itself
// (DESIGN.md "Checkpoint": the file is the bound, by an order of magnitude).
constexpr size_t kCkptChunkBytes = (size_t)64 << 20;
struct CkptHeader {
    char magic[8];
    uint32_t version, headerBytes;
    // fingerprint
    uint64_t sceneHash;
    int32_t forceDiffuse, width, height, maxDepth, minDepth, seedOffset, useGradient, maxDervDepth;
    int32_t mala, h2mc, sampleCache, useLightCoord, largeStepMultiplexed, filmFormat;  // filmFormat: kFilmFloat32 / kFilmFixed64 (the word was reserved and zero in version 1)
    float largeStepProb, largeStepScale, malaStepsize, malaGN, perturbStdDev, uniformMixProb;
    // the job's shape, progress
    int32_t nChainsTotal, initThreads;
    int64_t samplesPerChain, chainsNeedExtra, numInitSamples, stepsDone;
    double wallSeconds;
    // sizes
    uint32_t recordWords, filmWords;
    uint64_t jobBytes, totalBytes;
};
static_assert(sizeof(CkptHeader) == 176, "the checkpoint header is written as it lies in memory");
}  // namespace

uint64_t lmc_host::HashSceneFiles(const lmc::Scene &sc) {  // FNV-1a, 64 bit, over the bytes of the XML and of every file it pulled in, in parse order
    uint64_t h = 1469598103934665603ull;
    std::vector<unsigned char> buf(1 << 20);
    for (const std::string &fn : sc.sourceFiles) {
        FILE *f = fopen(fn.c_str(), "rb");
        if (!f) throw std::runtime_error("checkpoint: cannot read the scene file " + fn + " for its content hash");
        for (size_t n; (n = fread(buf.data(), 1, buf.size(), f)) > 0;)
            for (size_t k = 0; k < n; k++) h = (h ^ buf[k]) * 1099511628211ull;
        fclose(f);
        h = (h ^ 0xffu) * 1099511628211ull;  // file boundary
    }
    return h;
}
namespace {
CkptHeader MakeCkptHeader(lmc_ctx *c) {
    CkptHeader H;
    memset(&H, 0, sizeof(H));
    memcpy(H.magic, kCkptMagic, 8);
    H.version = c->filmExact ? kCkptVersionExact : kCkptVersion, H.headerBytes = sizeof(CkptHeader);
    H.filmFormat = c->filmExact ? kFilmFixed64 : kFilmFloat32;
    if (!c->sceneHash) c->sceneHash = HashSceneFiles(*c->scene);
    const lmc::DptOptions &o = c->scene->options;
    H.sceneHash = c->sceneHash;
    H.forceDiffuse = c->forceDiffuse, H.width = c->S.cam.width, H.height = c->S.cam.height, H.maxDepth = o.maxDepth, H.minDepth = o.minDepth, H.seedOffset = o.seedOffset;
    H.useGradient = c->useGradient, H.maxDervDepth = c->maxDervDepth;
    H.mala = o.mala, H.h2mc = o.h2mc, H.sampleCache = o.sampleFromGlobalCache, H.useLightCoord = o.useLightCoordinateSampling, H.largeStepMultiplexed = o.largeStepMultiplexed;
    H.largeStepProb = o.largeStepProbability, H.largeStepScale = o.largeStepProbScale, H.malaStepsize = o.malaStepsize, H.malaGN = o.malaGN;
    H.perturbStdDev = o.perturbStdDev, H.uniformMixProb = o.uniformMixingProbability;
    H.recordWords = (uint32_t)CkptRecordWords(o.maxDepth, c->S.opt.sampleCache != 0, o.h2mc);
    H.filmWords = (uint32_t)c->film.n;
    return H;
}
// the first fingerprint field in which the file differs from what the context would write; nullptr: none
const char *CkptMismatch(const CkptHeader &f, const CkptHeader &c) {
#define LMC_CK_FIELD(field, name) \
    if (memcmp(&f.field, &c.field, sizeof(f.field)) != 0) return name;
    LMC_CK_FIELD(sceneHash, "scene (the content hash of the scene XML and the files it pulls in)")
    LMC_CK_FIELD(forceDiffuse, "force_diffuse")
    LMC_CK_FIELD(width, "width")
    LMC_CK_FIELD(height, "height")
    LMC_CK_FIELD(maxDepth, "maxdepth")
    LMC_CK_FIELD(minDepth, "mindepth")
    LMC_CK_FIELD(seedOffset, "seedoffset")
    LMC_CK_FIELD(useGradient, "use_gradient")
    LMC_CK_FIELD(maxDervDepth, "max-derivatives-depth")
    LMC_CK_FIELD(mala, "mala")
    LMC_CK_FIELD(h2mc, "h2mc")
    LMC_CK_FIELD(sampleCache, "samplecache")
    LMC_CK_FIELD(useLightCoord, "uselightcoordinatesampling")
    LMC_CK_FIELD(largeStepMultiplexed, "largestepmultiplexed")
    LMC_CK_FIELD(largeStepProb, "largestepprob")
    LMC_CK_FIELD(largeStepScale, "largestepscale")
    LMC_CK_FIELD(malaStepsize, "mala-stepsize")
    LMC_CK_FIELD(malaGN, "mala-gn")
    LMC_CK_FIELD(perturbStdDev, "perturbstddev")
    LMC_CK_FIELD(uniformMixProb, "uniformmixprob")
    LMC_CK_FIELD(recordWords, "record size")
    LMC_CK_FIELD(filmWords, "film size")
#undef LMC_CK_FIELD
    return nullptr;
}
struct CkptFile {
    FILE *f = nullptr;
    std::string path;
    ~CkptFile() {
        if (f) fclose(f);
    }
    void Open(const std::string &p, const char *mode) {
        path = p;
        f = fopen(p.c_str(), mode);
        if (!f) throw std::runtime_error("checkpoint: cannot open " + p);
    }
    void Write(const void *p, size_t bytes) {
        if (bytes && fwrite(p, 1, bytes, f) != bytes) throw std::runtime_error("checkpoint: short write to " + path);
    }
    void Read(void *p, size_t bytes) {
        if (bytes && fread(p, 1, bytes, f) != bytes) throw std::runtime_error("checkpoint: " + path + " ends before its header says it does");
    }
    template <class T>
    void WriteVec(const std::vector<T> &v) { Write(v.data(), v.size() * sizeof(T)); }
    template <class T>
    std::vector<T> ReadVec(size_t n) {
        std::vector<T> v(n);
        Read(v.data(), n * sizeof(T));
        return v;
    }
};
// header of `path`, checked as far as a file alone can be: magic, version, header size, and a length of at least what the header says
CkptHeader ReadCkptHeader(CkptFile &F) {
    CkptHeader H;
    memset(&H, 0, sizeof(H));
    if (fread(&H, 1, sizeof(H), F.f) != sizeof(H)) throw std::runtime_error("checkpoint: " + F.path + " is shorter than a checkpoint header");
    if (memcmp(H.magic, kCkptMagic, 8) != 0) throw std::runtime_error("checkpoint: " + F.path + " is not a checkpoint file (wrong magic)");
    if ((H.version != kCkptVersion && H.version != kCkptVersionExact) || H.headerBytes != sizeof(CkptHeader))
        throw std::runtime_error("checkpoint: " + F.path + " has format version " + std::to_string(H.version) + ", this library reads version " + std::to_string(kCkptVersion) + " (and " +
                                 std::to_string(kCkptVersionExact) + ", the exact film)");
    if (H.filmFormat != (H.version == kCkptVersionExact ? kFilmFixed64 : kFilmFloat32)) throw std::runtime_error("checkpoint: " + F.path + " has an inconsistent header (film format)");
    if (fseek(F.f, 0, SEEK_END) != 0) throw std::runtime_error("checkpoint: cannot seek in " + F.path);
    const long long len = ftell(F.f);
    if (H.nChainsTotal <= 0 || H.totalBytes != sizeof(CkptHeader) + H.jobBytes + (uint64_t)H.nChainsTotal * H.recordWords * sizeof(float))
        throw std::runtime_error("checkpoint: " + F.path + " has an inconsistent header");
    if (len < 0 || (uint64_t)len < H.totalBytes)
        throw std::runtime_error("checkpoint: " + F.path + " is truncated: " + std::to_string(len) + " bytes, its header says " + std::to_string(H.totalBytes));
    if (fseek(F.f, (long)sizeof(CkptHeader), SEEK_SET) != 0) throw std::runtime_error("checkpoint: cannot seek in " + F.path);
    return H;
}
void CkptDrain(lmc_ctx *c) {  // the tail of the last step: cache pushes, the fill counts on their way to the host, a kd-tree going up on the cache stream
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    for (hipStream_t st : c->sideStream)
        if (st) HIP_CHECK(hipStreamSynchronize(st));
    for (hipStream_t st : c->partStream)
        if (st) HIP_CHECK(hipStreamSynchronize(st));
    if (c->cacheStream) HIP_CHECK(hipStreamSynchronize(c->cacheStream));
}
void CkptCheckMembers(const std::vector<lmc_ctx *> &g, const char *what, bool needChains) {
    for (lmc_ctx *c : g) {
        if (!c) throw std::runtime_error(std::string(what) + ": null context");
        if (c->comm && c->world > 1) throw std::runtime_error(std::string(what) + ": this context is a rank of an RCCL job (lmc_comm_init); checkpoints serve single contexts and in-process groups only");
        if (needChains && c->N <= 0) throw std::runtime_error(std::string(what) + " before lmc_chains_init");
    }
    if (needChains) {
        if (g.size() == 1 && g[0]->group.size() > 1) throw std::runtime_error(std::string(what) + ": this context is a member of an in-process group, use the lmc_group_checkpoint_ call");
        if (g.size() > 1)
            for (lmc_ctx *c : g)
                if (c->group != g) throw std::runtime_error(std::string(what) + ": not the group lmc_group_chains_init / lmc_group_checkpoint_load set up");
    }
}
struct CkptTiming {
    double packMs = 0, copyMs = 0, fileMs = 0;
};
bool CkptLog() {
    static const bool on = getenv("LMC_CKPT_LOG") != nullptr;  // measurement: the parts of a save / load, one line on stderr
    return on;
}

void CkptSave(const std::vector<lmc_ctx *> &g, const char *path, const char *what) {
    if (!path || !*path) throw std::runtime_error(std::string(what) + ": no path");
    CkptCheckMembers(g, what, true);
    for (lmc_ctx *c : g) RefuseLayered(c, what, "in this version a checkpoint holds an unlayered film only (nothing was written)");
    for (lmc_ctx *c : g)
        if (c->filmReduced) throw std::runtime_error(std::string(what) + ": the film already holds the sum over the ranks; a checkpoint of it would count the other ranks' share again");
    const auto t0 = std::chrono::steady_clock::now();
    for (lmc_ctx *c : g) CkptDrain(c);
    lmc_ctx *c0 = g[0];
    CkptHeader H = MakeCkptHeader(c0);
    int next = 0;
    for (lmc_ctx *c : g) {
        if (c->chainBegin != next || c->numChainsTotal != c0->numChainsTotal) throw std::runtime_error(std::string(what) + ": the contexts do not hold one job's chains in order");
        if (CkptMismatch(MakeCkptHeader(c), H)) throw std::runtime_error(std::string(what) + ": the members differ in " + CkptMismatch(MakeCkptHeader(c), H));
        if (c->filmExact != c0->filmExact) throw std::runtime_error(std::string(what) + ": the members differ in film_exact");
        next += c->N;
    }
    if (next != c0->numChainsTotal) throw std::runtime_error(std::string(what) + ": the contexts hold " + std::to_string(next) + " of the job's " + std::to_string(c0->numChainsTotal) + " chains");
    H.nChainsTotal = c0->numChainsTotal, H.initThreads = c0->initThreads;
    H.samplesPerChain = c0->perChain, H.chainsNeedExtra = c0->chainsNeedExtra, H.numInitSamples = c0->numInitSamples, H.stepsDone = c0->stepsDone;
    H.wallSeconds = c0->secondsBefore + std::chrono::duration<double>(std::chrono::steady_clock::now() - c0->chainsSince).count();
    // ---- job-wide state, from member 0 (identical on all members) except what the members hold a share of: counters, weight sum, film
    HIP_CHECK(hipSetDevice(c0->device));
    std::vector<char> job;
    auto put = [&](const void *p, size_t bytes) { job.insert(job.end(), (const char *)p, (const char *)p + bytes); };
    const int32_t lengthCount = (int32_t)c0->lengthFunc.size();
    const int64_t numInitContribs = c0->numInitContribs;
    put(&c0->normalization, 4), put(&c0->lengthFuncInt, 4), put(&numInitContribs, 8), put(&lengthCount, 4), put(&lengthCount, 4);
    put(c0->lengthFunc.data(), c0->lengthFunc.size() * 4), put(c0->lengthCdf.data(), c0->lengthCdf.size() * 4);
    {
        const std::vector<float> ls = c0->initLsAll.Download();
        std::vector<unsigned char> cl = c0->initCLAll.Download();
        cl.resize((cl.size() + 3) / 4 * 4, 0);
        put(ls.data(), ls.size() * 4), put(cl.data(), cl.size());
    }
    const std::vector<int> counts = c0->cacheCounts.Download();
    for (int sl = 0; sl < CACHE_SLOTS; sl++) {
        const CacheDimHost &cd = c0->cacheDims[6 + 2 * sl];
        const int32_t head[4] = {cd.relevant ? 1 : 0, cd.relevant ? counts[sl] : 0, cd.ready ? 1 : 0, 6 + 2 * sl};
        put(head, sizeof(head));
        if (!cd.relevant) continue;
        for (const DevBuf<float> *b : {&cd.pss, &cd.v1, &cd.v2, &cd.weight, &cd.extra}) {
            const std::vector<float> v = b->Download();
            put(v.data(), v.size() * 4);
        }
    }
    {
        std::vector<unsigned long long> counters(8, 0);
        double weightSum = 0;
        std::vector<float> film(c0->filmExact ? 0 : c0->film.n, 0.f);
        std::vector<long long> filmFx(c0->filmExact ? c0->film.n + 1 : 0, 0);  // exact mode: summed in int64; the film_overflow counter is the word behind the film, as on the device
        for (lmc_ctx *c : g) {  // rank order, like the film merge
            HIP_CHECK(hipSetDevice(c->device));
            const std::vector<unsigned long long> cc = c->counters.Download();
            for (int k = 0; k < 8; k++) counters[k] += cc[k];
            weightSum += c->weightSum.Download()[0];
            if (c0->filmExact) {
                const std::vector<long long> f = c->filmFx.Download();
                if (f.size() != filmFx.size()) throw std::runtime_error(std::string(what) + ": the members' films differ in size");
                for (size_t k = 0; k < filmFx.size(); k++) filmFx[k] += f[k];
                continue;
            }
            const std::vector<float> f = c->film.Download();
            if (f.size() != film.size()) throw std::runtime_error(std::string(what) + ": the members' films differ in size");
            for (size_t k = 0; k < f.size(); k++) film[k] += f[k];
        }
        put(counters.data(), 64), put(&weightSum, 8), put(film.data(), film.size() * 4), put(filmFx.data(), filmFx.size() * 8);
    }
    H.jobBytes = job.size();
    H.totalBytes = sizeof(CkptHeader) + H.jobBytes + (uint64_t)H.nChainsTotal * H.recordWords * sizeof(float);
    const std::string tmp = std::string(path) + ".tmp";
    CkptTiming T;
    {
        CkptFile F;
        F.Open(tmp, "wb");
        auto tf = std::chrono::steady_clock::now();
        F.Write(&H, sizeof(H)), F.Write(job.data(), job.size());
        T.fileMs += MsSince(tf);
        // ---- the records, member by member = in chain order, a chunk at a time
        const size_t recBytes = (size_t)H.recordWords * sizeof(float);
        for (lmc_ctx *c : g) {
            HIP_CHECK(hipSetDevice(c->device));
            const int chunk = (int)std::min<size_t>((size_t)c->N, std::max<size_t>(1024, kCkptChunkBytes / recBytes));
            DevBuf<float> staging;
            staging.Alloc((size_t)chunk * H.recordWords, false);
            float *pinned = nullptr;
            HIP_CHECK(hipHostMalloc((void **)&pinned, (size_t)chunk * recBytes, hipHostMallocDefault));
            try {
                for (int first = 0; first < c->N; first += chunk) {
                    const int n = std::min(chunk, c->N - first);
                    auto tp = std::chrono::steady_clock::now();
                    LaunchCkptPack(c->A, c->S.opt.maxDepth, c->S.opt.sampleCache != 0, c->S.opt.h2mc ? c->h2Gauss.p : nullptr, first, n, staging.p, c->stream);
                    HIP_CHECK(hipGetLastError());
                    if (CkptLog()) HIP_CHECK(hipStreamSynchronize(c->stream));
                    T.packMs += MsSince(tp);
                    tp = std::chrono::steady_clock::now();
                    HIP_CHECK(hipMemcpyAsync(pinned, staging.p, (size_t)n * recBytes, hipMemcpyDeviceToHost, c->stream));
                    HIP_CHECK(hipStreamSynchronize(c->stream));
                    T.copyMs += MsSince(tp);
                    tp = std::chrono::steady_clock::now();
                    F.Write(pinned, (size_t)n * recBytes);
                    T.fileMs += MsSince(tp);
                }
            } catch (...) {
                (void)hipHostFree(pinned);
                throw;
            }
            (void)hipHostFree(pinned);
        }
        auto tp = std::chrono::steady_clock::now();
        if (fflush(F.f) != 0) throw std::runtime_error(std::string(what) + ": cannot flush " + tmp);
        T.fileMs += MsSince(tp);
    }
    if (rename(tmp.c_str(), path) != 0) throw std::runtime_error(std::string(what) + ": cannot rename " + tmp + " to " + path);
    if (CkptLog())
        fprintf(stderr, "[lmc] checkpoint save: %d chains, %llu bytes, %u bytes per chain record: pack %.3f ms, copies %.3f ms, file %.3f ms, total %.3f ms\n", H.nChainsTotal,
                (unsigned long long)H.totalBytes, H.recordWords * 4u, T.packMs, T.copyMs, T.fileMs, MsSince(t0));
}

void CkptLoad(const std::vector<lmc_ctx *> &g, const char *path, const char *what) {
    if (!path || !*path) throw std::runtime_error(std::string(what) + ": no path");
    if (g.empty()) throw std::runtime_error(std::string(what) + ": empty group");
    CkptCheckMembers(g, what, false);
    for (lmc_ctx *c : g) RefuseLayered(c, what, "in this version a checkpoint holds an unlayered film only (the context is unchanged)");
    const auto t0 = std::chrono::steady_clock::now();
    CkptFile F;
    F.Open(path, "rb");
    const CkptHeader H = ReadCkptHeader(F);
    for (lmc_ctx *c : g) {
        if (const char *field = CkptMismatch(H, MakeCkptHeader(c))) throw std::runtime_error(std::string(what) + ": " + path + " was written for another render: '" + field + "' differs");
        if (H.filmFormat != (c->filmExact ? kFilmFixed64 : kFilmFloat32))
            throw std::runtime_error(std::string(what) + ": " + path + " holds a " + FilmFormatName(H.filmFormat) + " film, this context's film is " + FilmFormatName(c->filmExact ? kFilmFixed64 : kFilmFloat32) +
                                     "; set the film_exact option to the file's mode before loading");
    }
    if ((size_t)H.nChainsTotal < g.size()) throw std::runtime_error(std::string(what) + ": fewer chains than members");
    // ---- the job-wide state, on the host (a few MB); everything up to here has left the contexts as they were
    std::vector<char> job(H.jobBytes);
    F.Read(job.data(), job.size());
    size_t at = 0;
    auto get = [&](void *p, size_t bytes) {
        if (at + bytes > job.size()) throw std::runtime_error(std::string(what) + ": " + path + " has a job-wide section shorter than its contents");
        memcpy(p, job.data() + at, bytes);
        at += bytes;
    };
    float normalization = 0, lengthFuncInt = 0;
    int64_t numInitContribs = 0;
    int32_t lengthCount = 0, lengthCount2 = 0;
    get(&normalization, 4), get(&lengthFuncInt, 4), get(&numInitContribs, 8), get(&lengthCount, 4), get(&lengthCount2, 4);
    if (lengthCount < 0 || lengthCount > LENGTH_DIST_MAX) throw std::runtime_error(std::string(what) + ": bad length distribution in " + path);
    std::vector<float> lengthFunc(lengthCount), lengthCdf(lengthCount + 1), seedLs(H.nChainsTotal);
    std::vector<unsigned char> seedCL(((size_t)H.nChainsTotal + 3) / 4 * 4);
    get(lengthFunc.data(), lengthFunc.size() * 4), get(lengthCdf.data(), lengthCdf.size() * 4), get(seedLs.data(), seedLs.size() * 4), get(seedCL.data(), seedCL.size());
    seedCL.resize(H.nChainsTotal);
    struct DimRows {
        int32_t head[4] = {0, 0, 0, 0};  // relevant, rows filled, ready, dim
        std::vector<float> rows[5];      // pss, v1, v2, weight, extra
    } dims[CACHE_SLOTS];
    const bool sampleCache = g[0]->S.opt.sampleCache != 0;
    for (int sl = 0; sl < CACHE_SLOTS; sl++) {
        const int d = 6 + 2 * sl;
        get(dims[sl].head, sizeof(dims[sl].head));
        if (dims[sl].head[3] != d) throw std::runtime_error(std::string(what) + ": bad cache section in " + path);
        if (!dims[sl].head[0]) continue;
        const size_t n[5] = {(size_t)PSS_MAX_SIZE * d, (size_t)PSS_MAX_SIZE * d, (size_t)PSS_MAX_SIZE * d, (size_t)PSS_MAX_SIZE, sampleCache ? (size_t)PSS_MAX_SIZE * CACHE_ROW_EXTRA : 0};
        for (int k = 0; k < 5; k++) dims[sl].rows[k].resize(n[k]), get(dims[sl].rows[k].data(), n[k] * 4);
    }
    std::vector<unsigned long long> counters(8);
    double weightSum = 0;
    const bool exact = H.filmFormat == kFilmFixed64;
    std::vector<float> film(exact ? 0 : H.filmWords);
    std::vector<long long> filmFx(exact ? (size_t)H.filmWords + 1 : 0);
    get(counters.data(), 64), get(&weightSum, 8), get(film.data(), film.size() * 4);
    if (exact) get(filmFx.data(), filmFx.size() * 8);  // the words, then the film_overflow counter
    // the kd-trees of the dims the file holds ready: rebuilt from the rows by the code that built them (deterministic), once for all members
    lmc::KdTreeResult trees[CACHE_SLOTS];
    for (int sl = 0; sl < CACHE_SLOTS; sl++)
        if (dims[sl].head[0] && dims[sl].head[2]) trees[sl] = lmc::BuildKdTree(dims[sl].rows[0].data(), PSS_MAX_SIZE, 6 + 2 * sl);
    // ---- from here on the contexts change
    const size_t n = g.size();
    const size_t recBytes = (size_t)H.recordWords * sizeof(float);
    const uint64_t recordsAt = sizeof(CkptHeader) + H.jobBytes;
    CkptTiming T;
    try {
        if (n > 1 || g[0]->group.size() > 1)
            for (size_t r = 0; r < n; r++) {
                for (lmc_ctx *peer : g[r]->group)  // leaving an earlier group (lmc_group_chains_init does the same)
                    if (peer != g[r]) peer->group.clear(), peer->world = 1, peer->rank = 0;
                g[r]->world = (int)n, g[r]->rank = (int)r, g[r]->group = n > 1 ? g : std::vector<lmc_ctx *>();
            }
        for (size_t r = 0; r < n; r++) {
            lmc_ctx *c = g[r];
            ChainSetUp U;
            U.numChainsTotal = H.nChainsTotal, U.chainBegin = (int)((long long)H.nChainsTotal * (long long)r / (long long)n), U.chainEnd = (int)((long long)H.nChainsTotal * (long long)(r + 1) / (long long)n);
            U.perChain = H.samplesPerChain, U.chainsNeedExtra = H.chainsNeedExtra, U.seedLs = &seedLs, U.seedCL = &seedCL, U.fromCheckpoint = true;
            // before the set-up: its warm launches take their parameters (MakeStepParams: the length distribution) from the context
            c->normalization = normalization, c->lengthFuncInt = lengthFuncInt, c->numInitContribs = numInitContribs, c->lengthFunc = lengthFunc, c->lengthCdf = lengthCdf;
            SetUpChains(c, U);
            hipStream_t s = c->stream;
            c->initCL.clear(), c->initLs.clear(), c->initOffsets.clear();  // the per-contribution lists of MLTInit (lmc_init_contribs) are not part of a checkpoint
            c->numInitSamples = H.numInitSamples, c->initThreads = H.initThreads;
            // the caches: rows and fill counts as they were; a ready dim's existence grid built on the device, its tree uploaded, the struct published
            int cnt[CACHE_SLOTS] = {0, 0, 0, 0};
            bool anyReady = false;
            for (int sl = 0; sl < CACHE_SLOTS; sl++) {
                const int d = 6 + 2 * sl;
                CacheDimHost &cd = c->cacheDims[d];
                if ((dims[sl].head[0] != 0) != cd.relevant) throw std::runtime_error(std::string(what) + ": the file's cache dims are not this render's");
                if (!cd.relevant) continue;
                DevBuf<float> *dst[5] = {&cd.pss, &cd.v1, &cd.v2, &cd.weight, &cd.extra};
                for (int k = 0; k < 5; k++)
                    if (!dims[sl].rows[k].empty()) HIP_CHECK(hipMemcpy(dst[k]->p, dims[sl].rows[k].data(), dims[sl].rows[k].size() * 4, hipMemcpyHostToDevice));
                cnt[sl] = dims[sl].head[1], c->lastCounts[sl] = cnt[sl];
                if (!dims[sl].head[2]) continue;
                const lmc::KdTreeResult &t = trees[sl];
                if (t.nodes.size() > KD_MAX_NODES || t.vind.size() > (size_t)PSS_MAX_SIZE) throw std::runtime_error("kd-tree larger than its preallocated buffers");
                lmc::ChooseGridCoords(dims[sl].rows[0].data(), PSS_MAX_SIZE, d, cd.gridM, cd.gridCoord);
                LaunchBuildCacheGrid(cd.pss.p, PSS_MAX_SIZE, d, cd.gridG, cd.gridM, cd.gridCoord, c->gridScratchStart.p, c->gridScratchCursor.p, c->gridScratchWordCount.p, c->gridTileSums.p,
                                     cd.gridWords.p, cd.gridCellStart.p, cd.gridIdx.p, s);
                HIP_CHECK(hipMemcpyAsync(cd.nodes.p, t.nodes.data(), t.nodes.size() * sizeof(KdNode), hipMemcpyHostToDevice, s));
                HIP_CHECK(hipMemcpyAsync(cd.vind.p, t.vind.data(), t.vind.size() * sizeof(int), hipMemcpyHostToDevice, s));
                HIP_CHECK(hipStreamSynchronize(s));
                PublishCacheDim(c, d, t, s);
                cd.ready = true, anyReady = true;
            }
            HIP_CHECK(hipMemcpy(c->cacheCounts.p, cnt, sizeof(cnt), hipMemcpyHostToDevice));
            if (anyReady) UploadCacheStruct(c);
            if (r == 0) {  // the film, the counters and the weight sum go to member 0 alone: the film merge stays a sum
                HIP_CHECK(hipMemcpy(c->counters.p, counters.data(), 64, hipMemcpyHostToDevice));
                HIP_CHECK(hipMemcpy(c->weightSum.p, &weightSum, 8, hipMemcpyHostToDevice));
                if (exact) HIP_CHECK(hipMemcpy(c->filmFx.p, filmFx.data(), filmFx.size() * 8, hipMemcpyHostToDevice));
                else
                    HIP_CHECK(hipMemcpy(c->film.p, film.data(), film.size() * 4, hipMemcpyHostToDevice));
            }
            // the records of this member's chains
            const int chunk = (int)std::min<size_t>((size_t)c->N, std::max<size_t>(1024, kCkptChunkBytes / recBytes));
            DevBuf<float> staging;
            staging.Alloc((size_t)chunk * H.recordWords, false);
            float *pinned = nullptr;
            HIP_CHECK(hipHostMalloc((void **)&pinned, (size_t)chunk * recBytes, hipHostMallocDefault));
            try {
                if (fseeko(F.f, (off_t)(recordsAt + (uint64_t)c->chainBegin * recBytes), SEEK_SET) != 0) throw std::runtime_error(std::string(what) + ": cannot seek in " + path);
                for (int first = 0; first < c->N; first += chunk) {
                    const int m = std::min(chunk, c->N - first);
                    auto tp = std::chrono::steady_clock::now();
                    F.Read(pinned, (size_t)m * recBytes);
                    T.fileMs += MsSince(tp);
                    tp = std::chrono::steady_clock::now();
                    HIP_CHECK(hipMemcpyAsync(staging.p, pinned, (size_t)m * recBytes, hipMemcpyHostToDevice, s));
                    if (CkptLog()) HIP_CHECK(hipStreamSynchronize(s));
                    T.copyMs += MsSince(tp);
                    tp = std::chrono::steady_clock::now();
                    LaunchCkptUnpack(c->A, c->S.opt.maxDepth, sampleCache, c->S.opt.h2mc ? c->h2Gauss.p : nullptr, first, m, staging.p, s);
                    HIP_CHECK(hipGetLastError());
                    HIP_CHECK(hipStreamSynchronize(s));
                    T.packMs += MsSince(tp);
                }
            } catch (...) {
                (void)hipHostFree(pinned);
                throw;
            }
            (void)hipHostFree(pinned);
            // the work lists of the step that runs next, from the chains' nextKind and the caches as they are now (what the step before the save built)
            HIP_CHECK(hipMemsetAsync(c->listCounts[0].p, 0, 4 * sizeof(int), s));
            if (!c->allCachesReady) CachePending(c);  // allCachesReady / needGeneric as the head of the next step would find them
            BuildNextLists(c, 0);
            c->parity = 0;
            HIP_CHECK(hipStreamSynchronize(s));
            HIP_CHECK(hipGetLastError());
            c->stepsDone = H.stepsDone, c->secondsBefore = H.wallSeconds, c->chainsSince = std::chrono::steady_clock::now();
        }
        if (n > 1) GroupSetUpMerge(g);
    } catch (...) {  // a load that failed half way leaves no chains behind
        for (lmc_ctx *c : g) c->group.clear(), c->world = 1, c->rank = 0, c->N = 0;
        throw;
    }
    if (CkptLog())
        fprintf(stderr, "[lmc] checkpoint load: %d chains, %llu bytes: file %.3f ms, copies %.3f ms, unpack %.3f ms, total %.3f ms (set-up, cache trees and lists included)\n", H.nChainsTotal,
                (unsigned long long)H.totalBytes, T.fileMs, T.copyMs, T.packMs, MsSince(t0));
}
}  // namespace

extern "C" {

int lmc_checkpoint_save(lmc_ctx *c, const char *path) {
    LMC_TRY
    CkptSave({c}, path, "lmc_checkpoint_save");
    return 0;
    LMC_CATCH(-1)
}
int lmc_checkpoint_load(lmc_ctx *c, const char *path) {
    LMC_TRY
    if (c && c->group.size() > 1) throw std::runtime_error("lmc_checkpoint_load: this context is a member of an in-process group, use lmc_group_checkpoint_load");
    CkptLoad({c}, path, "lmc_checkpoint_load");
    return 0;
    LMC_CATCH(-1)
}
int lmc_group_checkpoint_save(lmc_ctx **ctxs, int n, const char *path) {
    LMC_TRY
    if (n < 1) throw std::runtime_error("lmc_group_checkpoint_save: empty group");
    CkptSave(std::vector<lmc_ctx *>(ctxs, ctxs + n), path, "lmc_group_checkpoint_save");
    return 0;
    LMC_CATCH(-1)
}
int lmc_group_checkpoint_load(lmc_ctx **ctxs, int n, const char *path) {
    LMC_TRY
    if (n < 1) throw std::runtime_error("lmc_group_checkpoint_load: empty group");
    CkptLoad(std::vector<lmc_ctx *>(ctxs, ctxs + n), path, "lmc_group_checkpoint_load");
    return 0;
    LMC_CATCH(-1)
}
// host only: the header of a checkpoint file as one JSON document (lmc_scene_dump's convention: at most cap - 1 characters + NUL, returns the full length, -1 on error)
long long lmc_checkpoint_info(const char *path, char *out, long long cap) {
    LMC_TRY
    if (!path) throw std::runtime_error("lmc_checkpoint_info: no path");
    CkptFile F;
    F.Open(path, "rb");
    const CkptHeader H = ReadCkptHeader(F);
    char buf[2048];
    snprintf(buf, sizeof(buf),
             "{\"version\":%u,\"film_format\":\"%s\",\"scene_hash\":\"%016llx\",\"force_diffuse\":%d,\"width\":%d,\"height\":%d,\"maxdepth\":%d,\"mindepth\":%d,\"seedoffset\":%d,\"use_gradient\":%d,"
             "\"max-derivatives-depth\":%d,\"mala\":%d,\"h2mc\":%d,\"samplecache\":%d,\"uselightcoordinatesampling\":%d,\"largestepmultiplexed\":%d,\"largestepprob\":%.9g,"
             "\"largestepscale\":%.9g,\"mala-stepsize\":%.9g,\"mala-gn\":%.9g,\"perturbstddev\":%.9g,\"uniformmixprob\":%.9g,\"n_chains_total\":%d,\"samples_per_chain\":%lld,"
             "\"chains_need_extra\":%lld,\"num_init_samples\":%lld,\"init_threads\":%d,\"steps_done\":%lld,\"wall_seconds\":%.9g,\"record_bytes\":%u,\"job_bytes\":%llu,\"total_bytes\":%llu}",
             H.version, H.filmFormat == kFilmFixed64 ? "fixed64" : "float32", (unsigned long long)H.sceneHash, H.forceDiffuse, H.width, H.height, H.maxDepth, H.minDepth, H.seedOffset, H.useGradient, H.maxDervDepth, H.mala, H.h2mc, H.sampleCache,
             H.useLightCoord, H.largeStepMultiplexed, H.largeStepProb, H.largeStepScale, H.malaStepsize, H.malaGN, H.perturbStdDev, H.uniformMixProb, H.nChainsTotal, (long long)H.samplesPerChain,
             (long long)H.chainsNeedExtra, (long long)H.numInitSamples, H.initThreads, (long long)H.stepsDone, H.wallSeconds, H.recordWords * 4u, (unsigned long long)H.jobBytes,
             (unsigned long long)H.totalBytes);
    const std::string j(buf);
    if (out && cap > 0) {
        const size_t n = std::min<size_t>(j.size(), (size_t)cap - 1);
        memcpy(out, j.data(), n);
        out[n] = 0;
    }
    return (long long)j.size();
    LMC_CATCH(-1)
}

}  // extern "C"
