// unipeak_amd/host/gzio.cpp -- see gzio.hpp.  gzip streams are wrapped as
// stdio FILEs (fopencookie over zlib's gzFile), so every reader and writer of
// the CLIs keeps its FILE* code path.  A ".bz2" input is decoded whole
// (up_bz_decode_host, or up_bz_decode on the device with UNIPEAK_BZ_DEVICE=1) and read
// from memory.
#include "gzio.hpp"

#include <sys/stat.h>
#include <zlib.h>

#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../include/unipeak_hip.h"
#include "cli.hpp"
#include "gzdev.hpp"
#include "wigio.hpp"

namespace unipeak {

static bool ends_with(const std::string &s, const char *suf) {
    const size_t n = std::strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

bool is_gz(const std::string &fname) { return ends_with(fname, ".gz"); }
bool is_bz2(const std::string &fname) { return ends_with(fname, ".bz2"); }

[[noreturn]] static void no_bz2_output(const std::string &fname) {
    fatal("could not write " + fname + ": bzip2 (.bz2) output is not supported (input is read, output is not written)");
}

[[noreturn]] static void gz_fail(gzFile g, const std::string &what) {
    int code = 0;
    const char *m = gzerror(g, &code);
    fatal(what + ": " + (m && *m ? m : "gzip stream error"));
}

namespace {
struct GzCookie {
    gzFile g;
    std::string name;
    uint64_t in = 0;      // bytes written through it
    bool timing = false;  // UNIPEAK_TIMING: a "gz" line at close
};

bool env_on(const char *name) {
    const char *e = std::getenv(name);
    return e && *e && *e != '0';
}

ssize_t gz_read(void *c, char *buf, size_t n) {
    GzCookie *k = (GzCookie *)c;
    const int r = gzread(k->g, buf, (unsigned)std::min<size_t>(n, 1u << 30));
    if (r < 0) gz_fail(k->g, "could not read " + k->name);
    return r;
}

ssize_t gz_write(void *c, const char *buf, size_t n) {
    GzCookie *k = (GzCookie *)c;
    size_t done = 0;
    while (done < n) {
        const int w = gzwrite(k->g, buf + done, (unsigned)std::min<size_t>(n - done, 1u << 30));
        if (w <= 0) return done ? (ssize_t)done : -1;
        done += (size_t)w;
    }
    k->in += done;
    return (ssize_t)done;
}

int gz_close(void *c) {
    GzCookie *k = (GzCookie *)c;
    const int r = gzclose(k->g);
    if (k->timing && r == Z_OK) {
        struct stat sb;
        const unsigned long long out = stat(k->name.c_str(), &sb) == 0 ? (unsigned long long)sb.st_size : 0;
        std::fprintf(stderr, "[timing] gz %s in %llu B out %llu B members 1 device 0.000 ms path zlib\n",
                     k->name.c_str(), (unsigned long long)k->in, out);
    }
    delete k;
    return r == Z_OK ? 0 : EOF;
}

// the device's DEFLATE encoder (up_dfl_stream) as the batch writer's compressor
class DeviceCompressor : public GzCompressor {
public:
    explicit DeviceCompressor(up_dfl *h) : h_(h) {}
    ~DeviceCompressor() override { up_dfl_close(h_); }
    bool stream(const void *src, uint64_t n, const void **out, uint64_t *n_out, uint32_t *crc32) override {
        rc_ = up_dfl_stream(h_, src, n, out, n_out, crc32);
        return rc_ == UP_OK;
    }
    double device_ms() const override {
        double v[1] = {0};
        up_dfl_timings(h_, v, 1);
        return v[0];
    }
    std::string error() const override { return up_strerror(rc_); }

private:
    up_dfl *h_;
    int rc_ = UP_OK;
};

std::unique_ptr<GzCompressor> make_device_compressor(std::string *err) {
    up_dfl *h = nullptr;
    const int rc = up_dfl_open(cli_physical_device(0), &h);
    if (rc != UP_OK) {
        *err = up_strerror(rc);
        return nullptr;
    }
    return std::unique_ptr<GzCompressor>(new DeviceCompressor(h));
}

ssize_t gzb_write(void *c, const char *buf, size_t n) {
    GzBatchWriter *w = (GzBatchWriter *)c;
    if (!w->write(buf, n)) fatal("could not write gzip output: " + w->error());
    return (ssize_t)n;
}

int gzb_close(void *c) {
    GzBatchWriter *w = (GzBatchWriter *)c;
    const bool ok = w->close();
    const std::string err = w->error();
    delete w;
    if (!ok) fatal("could not write gzip output: " + err);
    return 0;
}
// the reference's gzip filter (boost gzip_decompressor, misc/filterstream.cpp:
// 30-50) throws on a file without a gzip header; zlib would read it as plain
// bytes ("transparent" mode), so refuse it the same way
void not_gzip_check(gzFile g, const std::string &fname) {
    char c;
    const int r = gzread(g, &c, 1);  // reading decides direct vs gzip
    if (r < 0) gz_fail(g, "could not read " + fname);
    if (r == 1 && gzdirect(g)) {
        gzclose(g);
        fatal("could not read " + fname + ": not in gzip format");
    }
    if (r == 1) gzungetc((unsigned char)c, g);
}

// ISIZE of a gzip file (its last four bytes, little-endian), 0 if unreadable
size_t gz_isize_hint(const std::string &fname) {
    FILE *f = std::fopen(fname.c_str(), "rb");
    if (!f) return 0;
    unsigned char b[4] = {0, 0, 0, 0};
    size_t v = 0;
    if (std::fseek(f, -4, SEEK_END) == 0 && std::fread(b, 1, 4, f) == 4)
        v = (size_t)b[0] | ((size_t)b[1] << 8) | ((size_t)b[2] << 16) | ((size_t)b[3] << 24);
    std::fclose(f);
    return v;
}
}  // namespace

namespace {
// a decoded ".bz2" file behind a FILE*
struct MemCookie {
    std::string data;
    size_t at = 0;
};

ssize_t mem_read(void *c, char *buf, size_t n) {
    MemCookie *k = (MemCookie *)c;
    const size_t take = std::min(n, k->data.size() - k->at);
    std::memcpy(buf, k->data.data() + k->at, take);
    k->at += take;
    return (ssize_t)take;
}

int mem_close(void *c) {
    delete (MemCookie *)c;
    return 0;
}

bool read_whole(const std::string &fname, std::string &out) {
    FILE *f = std::fopen(fname.c_str(), "rb");
    if (!f) return false;
    out.clear();
    struct stat sb;
    if (fstat(fileno(f), &sb) == 0 && sb.st_size > 0) out.reserve((size_t)sb.st_size);
    char buf[1 << 16];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, k);
    std::fclose(f);
    return true;
}

[[noreturn]] void bz_fail(const std::string &fname, const up_bz_info_t &info) {
    fatal("could not read " + fname + ": " + up_bz_reason(info.reason) + " (bit " +
          std::to_string((unsigned long long)info.fail_bit) + ")");
}
}  // namespace

bool bunzip_file(const std::string &fname, std::string &out) {
    std::string z;
    if (!read_whole(fname, z)) return false;
    // the host twin unless UNIPEAK_BZ_DEVICE=1 asks for the device: on the samples measured so far
    // (9 and 24 blocks) the device path is the slower one
    const char *e = std::getenv("UNIPEAK_BZ_DEVICE");
    const bool device = e && *e && std::atoi(e) != 0;
    up_bz_info_t info{};
    double ms = 0;
    out.clear();
    if (device) {
        up_bz *h = nullptr;
        int rc = up_bz_open(cli_physical_device(0), &h);
        if (rc != UP_OK) fatal("could not read " + fname + ": bzip2 decoder: " + up_strerror(rc));
        const void *p = nullptr;
        uint64_t n = 0;
        rc = up_bz_decode(h, z.data(), z.size(), &p, &n, &info);
        if (rc == UP_OK) {
            out.assign((const char *)p, (size_t)n);
            double v[5] = {0, 0, 0, 0, 0};
            up_bz_timings(h, v, 5);
            ms = v[0] + v[1] + v[2] + v[3] + v[4];
        }
        up_bz_close(h);
        if (rc != UP_OK && info.reason != UP_BZ_OK) bz_fail(fname, info);
        if (rc != UP_OK) fatal("could not read " + fname + ": bzip2 decoder: " + up_strerror(rc));
    } else {
        out.resize(std::max<size_t>(z.size() * 8, 1u << 16));
        for (int pass = 0;; ++pass) {
            uint64_t n = 0;
            const int rc = up_bz_decode_host(z.data(), z.size(), &out[0], out.size(), &n, &info);
            if (rc != UP_OK && info.reason == UP_BZ_NOSPACE && pass == 0) {
                out.resize((size_t)n);  // the full size: the second pass fits
                continue;
            }
            if (rc != UP_OK) bz_fail(fname, info);
            out.resize((size_t)n);
            break;
        }
    }
    if (env_on("UNIPEAK_TIMING"))
        std::fprintf(stderr, "[timing] bz2 %s in %llu B out %llu B blocks %u device %.3f ms path %s\n", fname.c_str(),
                     (unsigned long long)z.size(), (unsigned long long)out.size(), info.blocks, ms,
                     device ? "device" : "host");
    return true;
}

FILE *open_input(const std::string &fname) {
    if (is_bz2(fname)) {
        std::unique_ptr<MemCookie> k(new MemCookie);
        if (!bunzip_file(fname, k->data)) return nullptr;
        cookie_io_functions_t io{mem_read, nullptr, nullptr, mem_close};
        FILE *f = fopencookie(k.get(), "r", io);
        if (f) (void)k.release();  // mem_close deletes it
        return f;
    }
    if (!is_gz(fname)) return std::fopen(fname.c_str(), "rb");
    gzFile g = gzopen(fname.c_str(), "rb");
    if (!g) return nullptr;
    gzbuffer(g, 1u << 20);
    not_gzip_check(g, fname);
    cookie_io_functions_t io{gz_read, nullptr, nullptr, gz_close};
    GzCookie *k = new GzCookie{g, fname};
    FILE *f = fopencookie(k, "r", io);
    if (!f) {
        gzclose(g);
        delete k;
    }
    return f;
}

FILE *open_output(const std::string &fname) {
    if (is_bz2(fname)) no_bz2_output(fname);
    if (!is_gz(fname)) return std::fopen(fname.c_str(), "wb");
    const bool timing = env_on("UNIPEAK_TIMING");
    const char *dev = std::getenv("UNIPEAK_GZ_DEVICE");
    if (!dev || std::atoi(dev) != 0) {  // batches through the device's encoder (gzdev.hpp)
        size_t batch = kGzBatchDefault;
        if (const char *e = std::getenv("UNIPEAK_GZ_BATCH")) batch = (size_t)std::strtoull(e, nullptr, 10);
        batch = std::max<size_t>(batch, up_dfl_block());
        GzBatchWriter *w = new GzBatchWriter(fname, batch, make_device_compressor, timing);
        cookie_io_functions_t io{nullptr, gzb_write, nullptr, gzb_close};
        FILE *f = w->open() ? fopencookie(w, "w", io) : nullptr;
        if (!f) delete w;
        return f;
    }
    gzFile g = gzopen(fname.c_str(), "wb");
    if (!g) return nullptr;
    gzbuffer(g, 1u << 20);
    cookie_io_functions_t io{nullptr, gz_write, nullptr, gz_close};
    GzCookie *k = new GzCookie{g, fname, 0, timing};
    FILE *f = fopencookie(k, "w", io);
    if (!f) {
        gzclose(g);
        delete k;
    }
    return f;
}

bool inflate_file(const std::string &fname, std::string &out) {
    gzFile g = gzopen(fname.c_str(), "rb");
    if (!g) return false;
    gzbuffer(g, 1u << 20);
    not_gzip_check(g, fname);
    out.clear();
    // sized from the gzip trailer's ISIZE (the uncompressed length mod 2^32
    // of the last member): one allocation for files below 4 GiB instead of
    // doubling to up to twice the inflated size
    out.resize(gz_isize_hint(fname) + (1u << 16));
    size_t n = 0;
    for (;;) {
        if (out.size() - n < (1u << 16)) out.resize(out.size() + std::max<size_t>(out.size() / 4, 1u << 22));
        const int r = gzread(g, &out[n], (unsigned)std::min<size_t>(out.size() - n, 1u << 30));
        if (r < 0) gz_fail(g, "could not read " + fname);
        if (r == 0) break;
        n += (size_t)r;
    }
    out.resize(n);
    gzclose(g);
    return true;
}

}  // namespace unipeak
