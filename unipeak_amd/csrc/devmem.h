// unipeak_amd/csrc/devmem.h -- owners of device memory, pinned host memory,
// events, streams and graph executables for the host layer (api.hip, tir.hip,
// countmap.hip).  Host-only: the kernel sources do not include it.  Every
// owner frees its resource in its destructor and is move-only, so a context
// needs no list of what to free and an early return leaks nothing.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <memory>
#include <utility>
#include <vector>

namespace upk {

// device memory: p points at n elements
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            n = std::exchange(o.n, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    // at least `want` elements, with a quarter of slack when it has to grow
    // (scratch that follows the data: contents are not kept)
    hipError_t ensure(size_t want) {
        if (want <= n && p) return hipSuccess;
        // growth is rare (first passes); a pipelined pass may still read p
        if (p) (void)hipDeviceSynchronize();
        return alloc_exact(want < 16 ? 16 : want + want / 4);
    }
    // at least `want` elements without slack or a device-wide wait: for
    // buffers sized by the data whose reader the caller has already drained
    hipError_t ensure_exact(size_t want) {
        if (want <= n && p) return hipSuccess;
        return alloc_exact(want < 16 ? 16 : want);
    }
    // a fresh allocation of exactly `count` elements (the old one is freed)
    hipError_t alloc_exact(size_t count) {
        release();
        hipError_t e = hipMalloc(&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

// pinned, device-mapped host memory: kernels write results straight into it
// (coherent, so the writes are visible to the host once the stream syncs)
template <typename T>
struct HostBuf {
    T *p = nullptr;    // host address
    T *dev = nullptr;  // device address of the same memory
    size_t n = 0;
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    HostBuf(HostBuf &&o) noexcept
        : p(std::exchange(o.p, nullptr)), dev(std::exchange(o.dev, nullptr)), n(std::exchange(o.n, 0)) {}
    HostBuf &operator=(HostBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            dev = std::exchange(o.dev, nullptr);
            n = std::exchange(o.n, 0);
        }
        return *this;
    }
    ~HostBuf() { release(); }
    hipError_t ensure(size_t want) {
        if (want <= n && p) return hipSuccess;
        if (p) (void)hipDeviceSynchronize();
        release();
        size_t cap = want < 16 ? 16 : want + want / 4;
        hipError_t e = hipHostMalloc((void **)&p, cap * sizeof(T), hipHostMallocMapped | hipHostMallocCoherent);
        if (e != hipSuccess) return e;
        e = hipHostGetDevicePointer((void **)&dev, p, 0);
        if (e == hipSuccess) n = cap;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = dev = nullptr;
        n = 0;
    }
};

// device scratch of one call: freed on every return path, an early error
// return included, after the stream whose work reads it has drained
class StreamScratch {
public:
    explicit StreamScratch(hipStream_t s) : s_(s) {}
    StreamScratch(const StreamScratch &) = delete;
    StreamScratch &operator=(const StreamScratch &) = delete;
    ~StreamScratch() {
        if (!p_.empty()) (void)hipStreamSynchronize(s_);
        for (void *q : p_) (void)hipFree(q);
    }
    // exactly `bytes` of device memory that lives until the call returns
    template <typename T>
    hipError_t alloc(T **out, size_t bytes) {
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, bytes);
        if (e == hipSuccess && q) p_.push_back(q);
        *out = (T *)q;
        return e;
    }

private:
    hipStream_t s_;
    std::vector<void *> p_;
};

// move-only owner of a HIP handle that converts to the raw handle, so it is
// passed to the runtime like one; create into it with &owner
template <typename H, hipError_t (*Destroy)(H)>
class Handle {
public:
    Handle() = default;
    Handle(const Handle &) = delete;
    Handle &operator=(const Handle &) = delete;
    Handle(Handle &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Handle &operator=(Handle &&o) noexcept {
        if (this != std::addressof(o)) {
            reset();
            h_ = std::exchange(o.h_, nullptr);
        }
        return *this;
    }
    ~Handle() { reset(); }
    operator H() const { return h_; }
    H *operator&() { return &h_; }  // for hipEventCreate(&e), hipStreamCreate...(&s, ...)
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }

private:
    H h_ = nullptr;
};

using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using GraphExec = Handle<hipGraphExec_t, hipGraphExecDestroy>;

}  // namespace upk
