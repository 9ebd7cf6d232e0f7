// tools/gzdev_check.cpp -- a host-only check of the batching gzip writer
// (host/gzdev.cpp) and of the code-length routine (csrc/dfl_codes.h), meant
// to be built with sanitizers:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include -o gzdev_check tools/gzdev_check.cpp unipeak_amd/host/gzdev.cpp -lz
//   ./gzdev_check /tmp/gzdev_check_dir
//
// The compressor is a stub that writes stored blocks, so no device is needed:
// what is checked is the batching (writes that straddle batches, whole
// batches from the caller's memory, the small-file path) and the framing
// (every file must read back through zlib's gzread as the bytes written).
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../unipeak_amd/csrc/dfl_codes.h"
#include "../unipeak_amd/host/gzdev.hpp"

using namespace unipeak;

namespace {

int g_streams = 0;

struct StoredStub : GzCompressor {
    std::vector<unsigned char> out_;
    bool stream(const void *src, uint64_t n, const void **out, uint64_t *n_out, uint32_t *crc) override {
        ++g_streams;
        out_.clear();
        const unsigned char *p = (const unsigned char *)src;
        for (uint64_t at = 0; at < n; at += 65535) {
            const uint32_t len = (uint32_t)std::min<uint64_t>(65535, n - at);
            const unsigned char h[5] = {0, (unsigned char)len, (unsigned char)(len >> 8), (unsigned char)~len,
                                        (unsigned char)(~len >> 8)};
            out_.insert(out_.end(), h, h + 5);
            out_.insert(out_.end(), p + at, p + at + len);
        }
        *out = out_.data();
        *n_out = out_.size();
        *crc = (uint32_t)crc32(0, p, (uInt)n);
        return true;
    }
    double device_ms() const override { return 0; }
    std::string error() const override { return ""; }
};

std::string read_back(const std::string &path) {
    gzFile g = gzopen(path.c_str(), "rb");
    if (!g) return "<unreadable>";
    std::string out;
    char buf[1 << 16];
    int r;
    while ((r = gzread(g, buf, sizeof buf)) > 0) out.append(buf, (size_t)r);
    if (r < 0) out = "<corrupt>";
    gzclose(g);
    return out;
}

int fails = 0;
void expect(bool ok, const char *what) {
    if (!ok) {
        std::fprintf(stderr, "FAIL: %s\n", what);
        ++fails;
    }
}

void one_file(const std::string &path, size_t total, size_t batch, size_t max_write, unsigned seed,
              int want_streams) {
    std::mt19937 rng(seed);
    std::string data(total, '\0');
    for (char &c : data) c = (char)('0' + rng() % 12);
    g_streams = 0;
    GzBatchWriter w(path, batch, [](std::string *) { return std::unique_ptr<GzCompressor>(new StoredStub); },
                    false);
    expect(w.open(), "open");
    for (size_t at = 0; at < total;) {
        const size_t n = std::min<size_t>(total - at, 1 + rng() % max_write);
        expect(w.write(data.data() + at, n), "write");
        at += n;
    }
    expect(w.close(), "close");
    expect(read_back(path) == data, path.c_str());
    if (want_streams >= 0) expect(g_streams == want_streams, "number of members");
}

void code_lengths() {
    std::mt19937 rng(7);
    for (int round = 0; round < 2000; ++round) {
        const uint32_t n = 1 + rng() % 288, max_len = 1 + rng() % 15;
        uint32_t freq[288];
        uint8_t len[288];
        uint32_t used = 0;
        for (uint32_t s = 0; s < n; ++s) {
            freq[s] = (rng() % 3 == 0) ? 0 : 1 + (rng() % (1u << (rng() % 20)));
            used += freq[s] != 0;
        }
        const bool ok = upk::dfl_code_lengths_host(freq, n, max_len, len);
        expect(ok == (used <= (1u << max_len)), "refusal exactly when the symbols do not fit");
        if (!ok) continue;
        uint64_t kraft = 0;
        for (uint32_t s = 0; s < n; ++s) {
            expect((len[s] == 0) == (freq[s] == 0) && len[s] <= max_len, "length range");
            if (len[s]) kraft += 1ull << (max_len - len[s]);
        }
        if (used >= 2) expect(kraft == (1ull << max_len), "Kraft sum");
    }
}

}  // namespace

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    one_file(dir + "/empty.gz", 0, 65536, 1, 1, 0);
    one_file(dir + "/small.gz", 70000, 1u << 20, 5000, 2, 0);           // zlib path
    one_file(dir + "/exact.gz", 3 * 65536, 65536, 65536 * 2, 3, 3);     // whole batches, none left over
    one_file(dir + "/straddle.gz", 500000, 65536, 300000, 4, 8);        // writes larger than a batch
    one_file(dir + "/tiny_writes.gz", 200001, 65536, 7, 5, 4);
    one_file(dir + "/one_batch_big.gz", (1u << 20) + 5, 4u << 20, 100000, 6, 1);  // >= 1 MiB: one member at close
    one_file(dir + "/below_small.gz", (1u << 20) - 1, 4u << 20, 100000, 7, 0);
    code_lengths();
    std::printf("%s\n", fails ? "FAILED" : "ok");
    return fails ? 1 : 0;
}
