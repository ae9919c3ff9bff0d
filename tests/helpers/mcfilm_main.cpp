// Stand-alone driver of host/mcfilm.cpp for the sanitizer build of tests/test_mc_exact_abi.py (g++ -fsanitize=address,undefined, no HIP, no Python).
// Reads one case per line from stdin and checks it:
//   coverage <total> <nAdds> <b e>.. | <accepted>.. | <nHeld> <b e>.. | <nComp> <b e>..
//   chunks <begin> <end> <nTiles> <cap> | <n> <b e>..
//   file <path>      a write / read round trip of the state file at <path>, then its refusals (truncated, wrong magic, wrong version)
// Prints "ok <n> cases" and returns 0, or the first failing line and returns 1.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>

#include "mcfilm.h"

using lmc::McRange;

static std::vector<McRange> ReadRanges(std::istream &in, int n) {
    std::vector<McRange> r(n);
    for (McRange &p : r) in >> p.first >> p.second;
    return r;
}
static void Bar(std::istream &in) {
    std::string s;
    in >> s;
    if (s != "|") throw std::runtime_error("malformed case");
}

static bool Coverage(std::istream &in) {
    long long total;
    int nAdds, n;
    in >> total >> nAdds;
    const std::vector<McRange> adds = ReadRanges(in, nAdds);
    Bar(in);
    std::vector<int> accepted(nAdds);
    for (int &a : accepted) in >> a;
    Bar(in);
    in >> n;
    const std::vector<McRange> held = ReadRanges(in, n);
    Bar(in);
    in >> n;
    const std::vector<McRange> comp = ReadRanges(in, n);
    lmc::McCoverage C;
    for (int i = 0; i < nAdds; i++) {
        const std::vector<McRange> before = C.ranges;
        const bool ok = C.Add(adds[i].first, adds[i].second);
        if (ok != (accepted[i] != 0)) return false;
        if (!ok && C.ranges != before) return false;  // a refused range leaves the coverage as it was
    }
    long long count = 0;
    for (const McRange &r : held) count += r.second - r.first;
    return C.ranges == held && C.Complement(total) == comp && C.Count() == count;
}

static bool Chunks(std::istream &in) {
    long long b, e, nTiles, cap;
    int n;
    in >> b >> e >> nTiles >> cap;
    Bar(in);
    in >> n;
    return lmc::McChunks(b, e, nTiles, cap) == ReadRanges(in, n);
}

static bool Refused(const std::string &path, const char *reason) {
    try {
        lmc::McFileRead(path, nullptr);
    } catch (const std::exception &e) {
        return std::string(e.what()).find(reason) != std::string::npos;
    }
    return false;
}
static std::string Slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}
static void Spit(const std::string &path, const std::string &bytes) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    f << bytes;
}

static bool File(std::istream &in) {
    std::string path;
    in >> path;
    lmc::McFileHeader H;
    H.sceneHash = 0xfedcba9876543210ull, H.forceDiffuse = 1, H.width = 21, H.height = 17, H.minDepth = -1, H.maxDepth = 8, H.seedOffset = 7, H.bidirectional = 1;
    H.nTiles = 4, H.spp = 3, H.paths = 1071, H.contributions = 998, H.overflow = 1;
    H.coverage.Add(0, 5), H.coverage.Add(8, 12);
    std::vector<long long> words(H.Words());
    for (size_t i = 0; i < words.size(); i++) words[i] = ((long long)i - 100) * 0x100000003ll;
    lmc::McFileWrite(path, H, words.data());
    std::vector<long long> back;
    const lmc::McFileHeader G = lmc::McFileRead(path, &back);
    if (back != words || lmc::McFileMismatch(G, H) || G.spp != 3 || G.paths != 1071 || G.contributions != 998 || G.overflow != 1 || G.coverage.ranges != H.coverage.ranges) return false;
    if (std::ifstream(path + ".tmp").good()) return false;  // renamed, not copied
    lmc::McFileHeader other = H;
    other.width = 22;
    if (std::string(lmc::McFileMismatch(G, other)) != "width") return false;
    other = H, other.seedOffset = 0;
    if (std::string(lmc::McFileMismatch(G, other)) != "seedoffset") return false;
    if (lmc::McFileJson(G).find("\"coverage\":[[0,5],[8,12]]") == std::string::npos) return false;
    const std::string bytes = Slurp(path);
    if (bytes.size() != G.WordsOffset() + G.Words() * 8) return false;
    for (size_t cut : {bytes.size() - 1, G.WordsOffset() - 3, (size_t)50, (size_t)10, (size_t)0}) {
        Spit(path, bytes.substr(0, cut));
        if (!Refused(path, "short file")) return false;
    }
    std::string bad = bytes;
    bad[3] = 'X';
    Spit(path, bad);
    if (!Refused(path, "wrong magic")) return false;
    bad = bytes, bad[8] = 9;
    Spit(path, bad);
    if (!Refused(path, "wrong version")) return false;
    Spit(path, bytes + "x");
    if (!Refused(path, "inconsistent header")) return false;
    return Refused(path + ".absent", "cannot open");
}

int main() {
    std::string line;
    int n = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        bool ok = false;
        try {
            ok = kind == "coverage" ? Coverage(in) : kind == "chunks" ? Chunks(in) : kind == "file" ? File(in) : false;
            if (in.fail()) ok = false;
        } catch (const std::exception &e) {
            printf("exception: %s\n", e.what());
        }
        if (!ok) {
            printf("FAILED: %s\n", line.c_str());
            return 1;
        }
        n++;
    }
    printf("ok %d cases\n", n);
    return 0;
}
