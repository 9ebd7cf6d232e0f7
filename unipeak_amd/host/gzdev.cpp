// unipeak_amd/host/gzdev.cpp -- see gzdev.hpp.
#include "gzdev.hpp"

#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cstring>

namespace unipeak {

GzBatchWriter::GzBatchWriter(std::string name, size_t batch, GzCompressorFactory make, bool timing)
    : name_(std::move(name)), batch_(std::max<size_t>(batch, 1)), make_(std::move(make)), timing_(timing) {}

GzBatchWriter::~GzBatchWriter() {
    if (raw_) std::fclose(raw_);
}

bool GzBatchWriter::open() {
    raw_ = std::fopen(name_.c_str(), "wb");
    return raw_ != nullptr;
}

bool GzBatchWriter::write(const char *p, size_t n) {
    if (!err_.empty()) return false;
    in_ += n;
    while (n) {
        if (buf_.empty() && n >= batch_) {  // a whole batch straight from the caller's memory
            if (!flush_member(p, batch_)) return false;
            p += batch_;
            n -= batch_;
            continue;
        }
        const size_t take = std::min(n, batch_ - buf_.size());
        buf_.insert(buf_.end(), p, p + take);
        p += take;
        n -= take;
        if (buf_.size() == batch_) {
            if (!flush_member(buf_.data(), buf_.size())) return false;
            buf_.clear();
        }
    }
    return true;
}

bool GzBatchWriter::flush_member(const char *p, size_t n) {
    if (!comp_) {
        comp_ = make_(&err_);
        if (!comp_) {
            if (err_.empty()) err_ = "no DEFLATE device";
            return false;
        }
    }
    const void *out = nullptr;
    uint64_t n_out = 0;
    uint32_t crc = 0;
    if (!comp_->stream(p, n, &out, &n_out, &crc)) {
        err_ = comp_->error();
        if (err_.empty()) err_ = "device DEFLATE failed";
        return false;
    }
    const unsigned char head[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};  // deflate, no flags, no mtime, Unix
    unsigned char tail[10] = {0x03, 0x00};                                // the empty final block
    const uint32_t isize = (uint32_t)n;
    for (int k = 0; k < 4; ++k) {
        tail[2 + k] = (unsigned char)(crc >> (8 * k));
        tail[6 + k] = (unsigned char)(isize >> (8 * k));
    }
    if (std::fwrite(head, 1, 10, raw_) != 10 || (n_out && std::fwrite(out, 1, n_out, raw_) != n_out) ||
        std::fwrite(tail, 1, 10, raw_) != 10) {
        err_ = "write failed";
        return false;
    }
    out_ += 20 + n_out;
    ++members_;
    return true;
}

// the file as gzopen / gzwrite / gzclose leave it (one deflate call at close)
bool GzBatchWriter::finish_zlib() {
    std::fflush(raw_);
    const int fd = dup(fileno(raw_));
    gzFile g = fd >= 0 ? gzdopen(fd, "wb") : nullptr;
    if (!g) {
        if (fd >= 0) ::close(fd);
        err_ = "gzdopen failed";
        return false;
    }
    gzbuffer(g, 1u << 20);
    bool ok = buf_.empty() || gzwrite(g, buf_.data(), (unsigned)buf_.size()) == (int)buf_.size();
    ok = gzclose(g) == Z_OK && ok;
    if (!ok) err_ = "gzip stream error";
    return ok;
}

bool GzBatchWriter::close() {
    bool ok = err_.empty();
    const bool small = members_ == 0 && buf_.size() < kGzSmall;
    if (ok) ok = small ? finish_zlib() : (buf_.empty() || flush_member(buf_.data(), buf_.size()));
    if (raw_) {
        if (ok && small) {
            std::fseek(raw_, 0, SEEK_END);
            const long at = std::ftell(raw_);
            out_ = at > 0 ? (uint64_t)at : 0;
        }
        if (std::fclose(raw_) != 0 && ok) {
            err_ = "close failed";
            ok = false;
        }
        raw_ = nullptr;
    }
    if (timing_ && ok)
        std::fprintf(stderr, "[timing] gz %s in %llu B out %llu B members %llu device %.3f ms path %s\n",
                     name_.c_str(), (unsigned long long)in_, (unsigned long long)out_,
                     (unsigned long long)(small ? 1 : members_), comp_ ? comp_->device_ms() : 0.0,
                     small ? "zlib" : "device");
    return ok;
}

}  // namespace unipeak
