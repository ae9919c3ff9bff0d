// Host-side bookkeeping of the exact mc film (lmc_mc_accumulate / lmc_mc_coverage / lmc_mc_save / lmc_mc_load; INTEGRATION.md "Exact mc film"):
// which stream ids of [0, nTiles * spp) a film holds, how a call's range is cut into launches, and the state file.
// Pure C++ (no HIP): mcrender.cpp calls these around its launches, and the CPU tier reaches them through lmc_mc_file_info and the
// lmc_mc_coverage_probe / lmc_mc_chunks_probe hooks (tests/test_mc_exact_abi.py, tests/helpers/mcfilm_main.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace lmc {

typedef std::pair<long long, long long> McRange;  // [begin, end) of stream ids

// the stream ids a film holds: disjoint, merged (no two ranges touch), ascending
struct McCoverage {
    std::vector<McRange> ranges;
    bool Overlaps(long long begin, long long end) const;  // an empty range overlaps nothing
    // adds [begin, end), merging with the ranges it touches; false, and nothing changed, if it overlaps what is there or begin > end or begin < 0
    bool Add(long long begin, long long end);
    // what [0, total) lacks, ascending
    std::vector<McRange> Complement(long long total) const;
    long long Count() const;
    long long End() const { return ranges.empty() ? 0 : ranges.back().second; }
    void Clear() { ranges.clear(); }
};

// [begin, end) cut into launches of at most `cap` stream ids; a cut falls on a multiple of nTiles wherever one lies inside the launch it ends
// (the samples of a tile then stay side by side in a wave, device/mc.hip "Lanes")
std::vector<McRange> McChunks(long long begin, long long end, long long nTiles, long long cap);

// The state file.  Little-endian, in this order:
//   magic "LMCMCFX\n" (8 bytes), uint32 version (1), uint32 number of coverage ranges R,
//   uint64 scene hash, int32 force_diffuse, width, height, mindepth, maxdepth, seedoffset, bidirectional, 0,
//   int64 nTiles, spp (the read divisor), paths, contributions, overflow,
//   R x (int64 begin, int64 end), width * height * 3 x int64 film words.
constexpr uint32_t kMcFileVersion = 1;
constexpr size_t kMcFileFixedBytes = 96;
struct McFileHeader {
    uint32_t version = kMcFileVersion;
    uint64_t sceneHash = 0;
    int32_t forceDiffuse = 0, width = 0, height = 0, minDepth = 0, maxDepth = 0, seedOffset = 0, bidirectional = 0;
    int64_t nTiles = 0, spp = 0, paths = 0, contributions = 0, overflow = 0;
    McCoverage coverage;
    size_t Words() const { return (size_t)width * (size_t)height * 3; }
    size_t WordsOffset() const { return kMcFileFixedBytes + coverage.ranges.size() * 16; }
};
// writes path + ".tmp" and renames it; throws std::runtime_error
void McFileWrite(const std::string &path, const McFileHeader &H, const long long *words);
// throws naming a wrong magic, a wrong version, a short file or an inconsistent header; words may be nullptr (header only)
McFileHeader McFileRead(const std::string &path, std::vector<long long> *words);
// the first field in which the file differs from what the context would write (divisor, counters and coverage are state, not compared); nullptr: none
const char *McFileMismatch(const McFileHeader &file, const McFileHeader &ctx);
std::string McFileJson(const McFileHeader &H);

}  // namespace lmc
