// tools/bz_check.cpp -- the bzip2 block decoder (csrc/bz_block.h, bz_host.h)
// under AddressSanitizer and UBSan, as a stand-alone host program.  The
// kernels compile the same header, so this run is the gate for the corrupt
// inputs before they go to a device once.  tools/bz_check.py writes the case
// files, builds this file with -fsanitize=address,undefined and runs it:
//
//   bz_check DIR     DIR/manifest.txt: one "<kind> <name> <reason>" per line
//                    valid   name.bz2 decodes to name.out
//                    corrupt name.bz2 fails with <reason> (-1: any reason)
//                    fuzz    name.bz2: every single-bit flip and every
//                            truncation either decodes or fails, cleanly,
//                            and the two routes below agree on which
//                    chain   name.bz2 (several blocks): an injected false
//                            candidate is dropped, a missing one is an error
//
// Every input runs through two routes: up_bz_decode_host (serial along the
// chain) and the device path's host side with the kernels' work done by the
// same header's routines (scan, entropy stage per candidate at the device's
// capacity, bz_chain, inverse BWT, run-length stage, bz_check_crcs).  Output
// buffers are heap blocks of the exact size, so one byte too many is caught.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../unipeak_amd/csrc/bz_host.h"

extern "C" int up_bz_decode_host(const void *src, uint64_t n, void *dst, uint64_t cap, uint64_t *n_out,
                                 up_bz_info_t *info) {
    return upk::bz_decode_host_capi(src, n, dst, cap, n_out, info);
}

namespace {

using Bytes = std::vector<uint8_t>;
int g_failures = 0;

void fail(const std::string &what) {
    std::fprintf(stderr, "FAIL: %s\n", what.c_str());
    ++g_failures;
}

bool read_file(const std::string &path, Bytes &out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

// a copy in a heap block of exactly n bytes: a read past the input is caught
std::unique_ptr<uint8_t[]> exact(const Bytes &v) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[v.size() ? v.size() : 1]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), v.size());
    return p;
}

// route 1: the twin, sized first, then into an exact block
int twin(const Bytes &z, Bytes &out, up_bz_info_t &info) {
    auto src = exact(z);
    uint64_t n = 0;
    int rc = up_bz_decode_host(src.get(), z.size(), nullptr, 0, &n, &info);
    if (rc != UP_OK && info.reason != UP_BZ_NOSPACE) return info.reason;
    std::unique_ptr<uint8_t[]> dst(new uint8_t[n ? n : 1]);
    uint64_t n2 = 0;
    rc = up_bz_decode_host(src.get(), z.size(), dst.get(), n, &n2, &info);
    if (rc != UP_OK) return info.reason ? info.reason : -100;
    if (n2 != n) return -101;
    out.assign(dst.get(), dst.get() + n);
    return UP_BZ_OK;
}

struct Staged {
    std::vector<upk::BzCand> cands;
    std::vector<upk::BzRec> recs;
    std::vector<Bytes> tt;
    std::vector<std::vector<uint32_t>> hist;
};

void stage(const uint8_t *src, uint64_t n, Staged &S) {
    S.cands = upk::bz_scan_host(src, n);
    S.recs.assign(S.cands.size(), upk::BzRec{0, 0, 0, 0, UP_BZ_OK});
    S.tt.assign(S.cands.size(), Bytes());
    S.hist.assign(S.cands.size(), std::vector<uint32_t>(256));
    std::unique_ptr<upk::BzTables> T(new upk::BzTables);
    std::unique_ptr<uint8_t[]> tt(new uint8_t[upk::kBzMaxCap]);
    for (size_t i = 0; i < S.cands.size(); ++i) {
        if (S.cands[i].kind) continue;
        upk::bz_entropy_host(src, n, S.cands[i].bit, upk::kBzMaxCap, *T, tt.get(), S.hist[i].data(), S.recs[i]);
        if (!S.recs[i].err) S.tt[i].assign(tt.get(), tt.get() + S.recs[i].n_block);
    }
}

// route 2 from the chain on
int finish(const uint8_t *src, uint64_t n, const Staged &S, Bytes &out, up_bz_info_t &info) {
    upk::BzChain C;
    if (upk::bz_chain(src, n, S.cands, S.recs, C, info) != UP_BZ_OK) return info.reason;
    std::vector<uint32_t> crcs(C.blocks.size()), work;
    out.clear();
    for (size_t b = 0; b < C.blocks.size(); ++b) {
        const uint32_t ci = C.blocks[b].cand;
        const upk::BzRec &R = S.recs[ci];
        std::unique_ptr<uint8_t[]> txt(new uint8_t[R.n_block]);
        upk::bz_unbwt_host(S.tt[ci].data(), R.n_block, S.hist[ci].data(), R.orig_ptr, work, txt.get());
        const uint64_t size = upk::bz_rle_expand(txt.get(), R.n_block, nullptr, 0, nullptr, nullptr);
        std::unique_ptr<uint8_t[]> dst(new uint8_t[size ? size : 1]);
        upk::bz_rle_expand(txt.get(), R.n_block, dst.get(), size, upk::bz_crc_table(), &crcs[b]);
        out.insert(out.end(), dst.get(), dst.get() + size);
    }
    if (upk::bz_check_crcs(C, S.cands, S.recs, crcs.data(), info) != UP_BZ_OK) return info.reason;
    return UP_BZ_OK;
}

int staged(const Bytes &z, Bytes &out, up_bz_info_t &info) {
    auto src = exact(z);
    Staged S;
    stage(src.get(), z.size(), S);
    return finish(src.get(), z.size(), S, out, info);
}

// both routes; they must agree on success and bytes.  Returns the twin's reason.
int both(const std::string &name, const Bytes &z, Bytes &out) {
    up_bz_info_t i1, i2;
    Bytes o2;
    const int r1 = twin(z, out, i1), r2 = staged(z, o2, i2);
    if (r1 < 0 || r2 < 0) fail(name + ": internal inconsistency");
    if ((r1 == UP_BZ_OK) != (r2 == UP_BZ_OK)) fail(name + ": the twin and the staged route disagree");
    if (r1 == UP_BZ_OK && r2 == UP_BZ_OK && (out != o2 || i1.blocks != i2.blocks || i1.streams != i2.streams))
        fail(name + ": the two routes decode differently");
    return r1;
}

void run_valid(const std::string &dir, const std::string &name) {
    Bytes z, want, got;
    if (!read_file(dir + "/" + name + ".bz2", z) || !read_file(dir + "/" + name + ".out", want))
        return fail(name + ": case files missing");
    const int r = both(name, z, got);
    if (r != UP_BZ_OK) return fail(name + ": valid file refused, reason " + std::to_string(r));
    if (got != want) fail(name + ": wrong bytes");
}

void run_corrupt(const std::string &dir, const std::string &name, int reason) {
    Bytes z, got;
    if (!read_file(dir + "/" + name + ".bz2", z)) return fail(name + ": case file missing");
    const int r = both(name, z, got);
    if (r == UP_BZ_OK) return fail(name + ": corrupt file accepted");
    if (reason >= 0 && r != reason)
        fail(name + ": reason " + std::to_string(r) + ", expected " + std::to_string(reason));
    up_bz_info_t info;
    const int r2 = staged(z, got, info);
    if (reason >= 0 && r2 != reason)
        fail(name + ": the staged route gives reason " + std::to_string(r2) + ", expected " + std::to_string(reason));
}

void run_fuzz(const std::string &dir, const std::string &name) {
    Bytes z, got;
    if (!read_file(dir + "/" + name + ".bz2", z)) return fail(name + ": case file missing");
    size_t ok = 0, bad = 0;
    for (size_t bit = 0; bit < z.size() * 8; ++bit) {
        Bytes m = z;
        m[bit >> 3] ^= (uint8_t)(0x80u >> (bit & 7));
        (both(name + " flip " + std::to_string(bit), m, got) == UP_BZ_OK ? ok : bad)++;
    }
    for (size_t len = 0; len < z.size(); ++len) {
        Bytes m(z.begin(), z.begin() + len);
        // a cut at a stream's end leaves a valid file; every other one must be refused, and the
        // two routes agreeing with each other is the check
        (both(name + " cut " + std::to_string(len), m, got) == UP_BZ_OK ? ok : bad)++;
    }
    std::printf("fuzz %s: %zu inputs, %zu decoded, %zu refused\n", name.c_str(), ok + bad, ok, bad);
}

void run_chain(const std::string &dir, const std::string &name) {
    Bytes z, want, got;
    if (!read_file(dir + "/" + name + ".bz2", z) || !read_file(dir + "/" + name + ".out", want))
        return fail(name + ": case files missing");
    auto src = exact(z);
    Staged S;
    stage(src.get(), z.size(), S);
    size_t blocks = 0;
    for (const auto &c : S.cands) blocks += c.kind == 0;
    if (blocks < 3) return fail(name + ": needs three blocks or more");
    up_bz_info_t info;
    // a false block candidate (as the entropy stage leaves it: an error) and a false end
    // candidate, both between the second and the third candidate
    Staged F = S;
    const uint64_t at = S.cands[1].bit + 1001;
    auto ins = [&](uint64_t bit, uint8_t kind, int err) {
        size_t k = 0;
        while (k < F.cands.size() && F.cands[k].bit < bit) ++k;
        F.cands.insert(F.cands.begin() + k, upk::BzCand{bit, kind});
        F.recs.insert(F.recs.begin() + k, upk::BzRec{0, 0, 0, 0, err});
        F.tt.insert(F.tt.begin() + k, Bytes());
        F.hist.insert(F.hist.begin() + k, std::vector<uint32_t>(256));
    };
    ins(at, 0, UP_BZ_BAD_CODE);
    ins(at + 77, 1, UP_BZ_OK);
    // a false candidate that "decodes": it must still be dropped, nothing ends at it
    ins(at + 150, 0, UP_BZ_OK);
    F.recs[std::find_if(F.cands.begin(), F.cands.end(), [&](const upk::BzCand &c) { return c.bit == at + 150; }) -
           F.cands.begin()] = upk::BzRec{at + 5000, 10, 0, 0, UP_BZ_OK};
    if (finish(src.get(), z.size(), F, got, info) != UP_BZ_OK || got != want)
        fail(name + ": false candidates changed the result");
    else if (info.dropped != 3)
        fail(name + ": dropped " + std::to_string(info.dropped) + " candidates, expected 3");
    // the second block's candidate missing: the chain breaks there
    Staged M = S;
    size_t second = 0, seen = 0;
    for (size_t k = 0; k < S.cands.size(); ++k)
        if (S.cands[k].kind == 0 && ++seen == 2) second = k;
    M.cands.erase(M.cands.begin() + second);
    M.recs.erase(M.recs.begin() + second);
    M.tt.erase(M.tt.begin() + second);
    M.hist.erase(M.hist.begin() + second);
    if (finish(src.get(), z.size(), M, got, info) != UP_BZ_BAD_MAGIC || info.fail_bit != S.cands[second].bit)
        fail(name + ": a missing candidate was not reported as a broken chain");
    std::printf("chain %s: %zu candidates, false ones dropped, missing one reported\n", name.c_str(),
                S.cands.size());
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: bz_check DIR\n");
        return 2;
    }
    const std::string dir = argv[1];
    std::ifstream mf(dir + "/manifest.txt");
    if (!mf) {
        std::fprintf(stderr, "bz_check: no manifest in %s\n", dir.c_str());
        return 2;
    }
    std::string line;
    size_t cases = 0;
    while (std::getline(mf, line)) {
        std::istringstream ss(line);
        std::string kind, name;
        int reason = -1;
        if (!(ss >> kind >> name >> reason)) continue;
        ++cases;
        if (kind == "valid") run_valid(dir, name);
        else if (kind == "corrupt") run_corrupt(dir, name, reason);
        else if (kind == "fuzz") run_fuzz(dir, name);
        else if (kind == "chain") run_chain(dir, name);
        else fail("unknown case kind " + kind);
    }
    std::printf("bz_check: %zu cases, %d failures\n", cases, g_failures);
    return g_failures ? 1 : 0;
}
