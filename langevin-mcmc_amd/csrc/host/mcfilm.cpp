// Host-side bookkeeping of the exact mc film: coverage arithmetic, launch chunks, the state file (mcfilm.h).
#include "mcfilm.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace lmc {

bool McCoverage::Overlaps(long long begin, long long end) const {
    if (begin >= end) return false;
    for (const McRange &r : ranges)
        if (begin < r.second && r.first < end) return true;
    return false;
}

bool McCoverage::Add(long long begin, long long end) {
    if (begin < 0 || begin > end || Overlaps(begin, end)) return false;
    if (begin == end) return true;
    std::vector<McRange> out;
    McRange add(begin, end);
    for (const McRange &r : ranges) {  // nothing overlaps, so at most one range touches from below and one from above
        if (r.second == add.first) add.first = r.first;
        else if (r.first == add.second) add.second = r.second;
        else
            out.push_back(r);
    }
    out.push_back(add);
    std::sort(out.begin(), out.end());
    ranges.swap(out);
    return true;
}

std::vector<McRange> McCoverage::Complement(long long total) const {
    std::vector<McRange> out;
    long long at = 0;
    for (const McRange &r : ranges) {
        if (at >= total) break;
        if (r.first > at) out.push_back(McRange(at, std::min(r.first, total)));
        at = std::max(at, r.second);
    }
    if (at < total) out.push_back(McRange(at, total));
    return out;
}

long long McCoverage::Count() const {
    long long n = 0;
    for (const McRange &r : ranges) n += r.second - r.first;
    return n;
}

std::vector<McRange> McChunks(long long begin, long long end, long long nTiles, long long cap) {
    std::vector<McRange> out;
    if (cap < 1) cap = 1;
    if (nTiles < 1) nTiles = 1;
    for (long long at = begin; at < end;) {
        long long e = std::min(end, at + cap);
        if (e < end) {
            const long long aligned = e / nTiles * nTiles;
            if (aligned > at) e = aligned;
        }
        out.push_back(McRange(at, e));
        at = e;
    }
    return out;
}

namespace {

constexpr char kMcMagic[8] = {'L', 'M', 'C', 'M', 'C', 'F', 'X', '\n'};

void Put(std::vector<unsigned char> &b, uint64_t v, int bytes) {
    for (int k = 0; k < bytes; k++) b.push_back((unsigned char)(v >> (8 * k)));
}
uint64_t Get(const unsigned char *p, int bytes) {
    uint64_t v = 0;
    for (int k = 0; k < bytes; k++) v |= (uint64_t)p[k] << (8 * k);
    return v;
}

struct FileCloser {
    FILE *f;
    ~FileCloser() {
        if (f) fclose(f);
    }
};

}  // namespace

void McFileWrite(const std::string &path, const McFileHeader &H, const long long *words) {
    std::vector<unsigned char> b;
    b.insert(b.end(), kMcMagic, kMcMagic + 8);
    Put(b, H.version, 4), Put(b, (uint32_t)H.coverage.ranges.size(), 4);
    Put(b, H.sceneHash, 8);
    const int32_t i32[8] = {H.forceDiffuse, H.width, H.height, H.minDepth, H.maxDepth, H.seedOffset, H.bidirectional, 0};
    for (int32_t v : i32) Put(b, (uint32_t)v, 4);
    const int64_t i64[5] = {H.nTiles, H.spp, H.paths, H.contributions, H.overflow};
    for (int64_t v : i64) Put(b, (uint64_t)v, 8);
    for (const McRange &r : H.coverage.ranges) Put(b, (uint64_t)r.first, 8), Put(b, (uint64_t)r.second, 8);
    const size_t nWords = H.Words();
    b.reserve(b.size() + nWords * 8);
    for (size_t i = 0; i < nWords; i++) Put(b, (uint64_t)words[i], 8);
    const std::string tmp = path + ".tmp";
    FileCloser F{fopen(tmp.c_str(), "wb")};
    if (!F.f) throw std::runtime_error("mc state file: cannot open " + tmp + " for writing");
    const bool ok = fwrite(b.data(), 1, b.size(), F.f) == b.size() && fflush(F.f) == 0;
    fclose(F.f);
    F.f = nullptr;
    if (!ok) {
        remove(tmp.c_str());
        throw std::runtime_error("mc state file: short write to " + tmp);
    }
    if (rename(tmp.c_str(), path.c_str()) != 0) throw std::runtime_error("mc state file: cannot rename " + tmp + " to " + path);
}

McFileHeader McFileRead(const std::string &path, std::vector<long long> *words) {
    FileCloser F{fopen(path.c_str(), "rb")};
    if (!F.f) throw std::runtime_error("mc state file: cannot open " + path);
    unsigned char fixed[kMcFileFixedBytes];
    const size_t got = fread(fixed, 1, sizeof(fixed), F.f);
    if (got >= 8 && memcmp(fixed, kMcMagic, 8) != 0) throw std::runtime_error("mc state file: " + path + " has a wrong magic (not an mc film state file)");
    if (got >= 12 && Get(fixed + 8, 4) != kMcFileVersion)
        throw std::runtime_error("mc state file: " + path + " has a wrong version (" + std::to_string(Get(fixed + 8, 4)) + ", this build reads " + std::to_string(kMcFileVersion) + ")");
    if (got < sizeof(fixed)) throw std::runtime_error("mc state file: " + path + " is a short file (" + std::to_string(got) + " bytes, the header alone has " + std::to_string(sizeof(fixed)) + ")");
    McFileHeader H;
    H.version = (uint32_t)Get(fixed + 8, 4);
    const uint64_t nRanges = Get(fixed + 12, 4);
    H.sceneHash = Get(fixed + 16, 8);
    int32_t *i32[7] = {&H.forceDiffuse, &H.width, &H.height, &H.minDepth, &H.maxDepth, &H.seedOffset, &H.bidirectional};
    for (int k = 0; k < 7; k++) *i32[k] = (int32_t)Get(fixed + 24 + 4 * k, 4);
    int64_t *i64[5] = {&H.nTiles, &H.spp, &H.paths, &H.contributions, &H.overflow};
    for (int k = 0; k < 5; k++) *i64[k] = (int64_t)Get(fixed + 56 + 8 * k, 8);
    if (H.width < 1 || H.height < 1 || H.width > 65536 || H.height > 65536 || H.spp < 0 || H.nTiles != (int64_t)((H.width + 15) / 16) * ((H.height + 15) / 16))
        throw std::runtime_error("mc state file: " + path + " has an inconsistent header (film size / tiles)");
    if (fseek(F.f, 0, SEEK_END) != 0) throw std::runtime_error("mc state file: cannot seek in " + path);
    const long long size = ftell(F.f);
    const unsigned long long want = kMcFileFixedBytes + nRanges * 16 + (unsigned long long)H.Words() * 8;
    if (size < 0 || (unsigned long long)size < want)
        throw std::runtime_error("mc state file: " + path + " is a short file (" + std::to_string(size) + " bytes, its header asks for " + std::to_string(want) + ")");
    if ((unsigned long long)size != want) throw std::runtime_error("mc state file: " + path + " has an inconsistent header (" + std::to_string(size) + " bytes, its header asks for " + std::to_string(want) + ")");
    fseek(F.f, (long)kMcFileFixedBytes, SEEK_SET);
    std::vector<unsigned char> rb((size_t)nRanges * 16);
    if (!rb.empty() && fread(rb.data(), 1, rb.size(), F.f) != rb.size()) throw std::runtime_error("mc state file: " + path + " is a short file (coverage)");
    for (uint64_t k = 0; k < nRanges; k++) {
        const long long b = (long long)Get(rb.data() + 16 * k, 8), e = (long long)Get(rb.data() + 16 * k + 8, 8);
        if (b >= e || b < H.coverage.End() + (H.coverage.ranges.empty() ? 0 : 1) || !H.coverage.Add(b, e))
            throw std::runtime_error("mc state file: " + path + " has an inconsistent header (coverage ranges not disjoint, merged and ascending)");
    }
    if (words) {
        std::vector<unsigned char> wb(H.Words() * 8);
        if (fread(wb.data(), 1, wb.size(), F.f) != wb.size()) throw std::runtime_error("mc state file: " + path + " is a short file (film words)");
        words->resize(H.Words());
        for (size_t i = 0; i < words->size(); i++) (*words)[i] = (long long)Get(wb.data() + 8 * i, 8);
    }
    return H;
}

const char *McFileMismatch(const McFileHeader &f, const McFileHeader &c) {
    if (f.sceneHash != c.sceneHash) return "scene (the content hash of the scene XML and the files it pulls in)";
    if (f.forceDiffuse != c.forceDiffuse) return "force_diffuse";
    if (f.width != c.width) return "width";
    if (f.height != c.height) return "height";
    if (f.minDepth != c.minDepth) return "mindepth";
    if (f.maxDepth != c.maxDepth) return "maxdepth";
    if (f.seedOffset != c.seedOffset) return "seedoffset";
    if (f.bidirectional != c.bidirectional) return "bidirectional";
    if (f.nTiles != c.nTiles) return "n_tiles";
    return nullptr;
}

std::string McFileJson(const McFileHeader &H) {
    char buf[1024];
    snprintf(buf, sizeof(buf),
             "{\"version\":%u,\"film_format\":\"fixed64\",\"scene_hash\":\"%016llx\",\"force_diffuse\":%d,\"width\":%d,\"height\":%d,\"mindepth\":%d,\"maxdepth\":%d,\"seedoffset\":%d,"
             "\"bidirectional\":%d,\"n_tiles\":%lld,\"spp\":%lld,\"paths\":%lld,\"contributions\":%lld,\"overflow\":%lld,\"streams_held\":%lld,\"film_words\":%llu,\"words_offset\":%llu,"
             "\"total_bytes\":%llu,\"coverage\":[",
             H.version, (unsigned long long)H.sceneHash, H.forceDiffuse, H.width, H.height, H.minDepth, H.maxDepth, H.seedOffset, H.bidirectional, (long long)H.nTiles, (long long)H.spp,
             (long long)H.paths, (long long)H.contributions, (long long)H.overflow, H.coverage.Count(), (unsigned long long)H.Words(), (unsigned long long)H.WordsOffset(),
             (unsigned long long)(H.WordsOffset() + H.Words() * 8));
    std::string j(buf);
    for (size_t k = 0; k < H.coverage.ranges.size(); k++)
        j += (k ? ",[" : "[") + std::to_string(H.coverage.ranges[k].first) + "," + std::to_string(H.coverage.ranges[k].second) + "]";
    return j + "]}";
}

}  // namespace lmc

// ---- C-ABI test hooks (include/lmc_abi.h): host only
// adds[2 i], adds[2 i + 1] are added in turn to an empty coverage; accepted[i] = 1 / 0.  Then cov receives the ranges held (at most covCap pairs, *nCov
// the number held) and comp the complement within [0, total) (likewise).
extern "C" int lmc_mc_coverage_probe(const long long *adds, int nAdds, long long total, int *accepted, long long *cov, int covCap, int *nCov, long long *comp, int compCap,
                                     int *nComp) {
    lmc::McCoverage C;
    for (int i = 0; i < nAdds; i++) {
        const std::vector<lmc::McRange> before = C.ranges;
        const bool ok = C.Add(adds[2 * i], adds[2 * i + 1]);
        if (!ok && C.ranges != before) return -1;
        if (accepted) accepted[i] = ok ? 1 : 0;
    }
    const std::vector<lmc::McRange> m = C.Complement(total);
    for (int k = 0; k < (int)C.ranges.size() && k < covCap; k++) cov[2 * k] = C.ranges[k].first, cov[2 * k + 1] = C.ranges[k].second;
    for (int k = 0; k < (int)m.size() && k < compCap; k++) comp[2 * k] = m[k].first, comp[2 * k + 1] = m[k].second;
    if (nCov) *nCov = (int)C.ranges.size();
    if (nComp) *nComp = (int)m.size();
    return 0;
}
// the launches [begin, end) is cut into (mcfilm.h McChunks): returns their number, writes at most cap pairs
extern "C" int lmc_mc_chunks_probe(long long begin, long long end, long long nTiles, long long launchStreams, long long *out, int cap) {
    const std::vector<lmc::McRange> c = lmc::McChunks(begin, end, nTiles, launchStreams);
    for (int k = 0; k < (int)c.size() && k < cap; k++) out[2 * k] = c[k].first, out[2 * k + 1] = c[k].second;
    return (int)c.size();
}
