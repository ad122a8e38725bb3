// devmem.hpp -- the owners of the host side's device and pinned memory (engine.cpp, engine_plan.cpp, engine_dag.cpp): DevBuf, one allocation with its
// capacity, and StagedUpload, a pinned-to-device upload with its event.  Move-only; no HIP call except where a comment says
// so (tests/integration/devmem_selftest.cpp counts them against stand-ins of the runtime).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace bce {

// One hipMalloc (Pinned: hipHostMalloc) allocation of capacity() elements, freed by reset() and the destructor.
template <class T, bool Pinned = false>
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {   // what this held goes to o, and is freed with it
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
        return *this;
    }
    ~DevBuf() { reset(); }

    T* get() const { return p_; }
    size_t capacity() const { return cap_; }

    // exactly n elements; the buffer must be empty
    hipError_t alloc(size_t n) {
        void* p = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p);
        cap_ = n;
        return hipSuccess;
    }
    // Nothing when need <= capacity().  Otherwise: waits for `sync` if given (work in flight may use the old buffer), frees,
    // allocates `cap` >= need elements (the policy is the caller's; contents are not kept).  Empty after a failure.
    hipError_t grow(size_t need, size_t cap, hipStream_t sync) {
        if (need <= cap_) return hipSuccess;
        const hipError_t e = sync ? hipStreamSynchronize(sync) : hipSuccess;
        reset();
        return e != hipSuccess ? e : alloc(cap);
    }
    void reset() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }

  private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// A device buffer, a pinned buffer of the same capacity (bytes) and the event that tells when the device is done with
// what was staged last: reserve(), fill host(), send() -- or copy(), launch the kernel that reads device(), mark().
class StagedUpload {
  public:
    StagedUpload() = default;
    StagedUpload(StagedUpload&& o) noexcept
        : dev_(std::move(o.dev_)), host_(std::move(o.host_)), ev_(std::exchange(o.ev_, nullptr)), busy_(std::exchange(o.busy_, false)) {}
    StagedUpload& operator=(StagedUpload&& o) noexcept {   // as DevBuf's: a swap
        std::swap(dev_, o.dev_); std::swap(host_, o.host_); std::swap(ev_, o.ev_); std::swap(busy_, o.busy_);
        return *this;
    }
    ~StagedUpload() { reset(); }

    void* host() const { return host_.get(); }
    const void* device() const { return dev_.get(); }
    size_t capacity() const { return dev_.capacity(); }

    // Waits for the event if the last send() / mark() may not have passed yet; grows both buffers to cap_bytes if they hold
    // less than `bytes` (DevBuf::grow, after `sync`); creates the event if there is none.  Large enough and not busy: no HIP
    // call, nothing moves.  After a failed growth both buffers are empty.
    hipError_t reserve(size_t bytes, size_t cap_bytes, hipStream_t sync) {
        if (busy_) {
            const hipError_t e = hipEventSynchronize(ev_);
            if (e != hipSuccess) return e;
            busy_ = false;
        }
        hipError_t e = dev_.grow(bytes, cap_bytes, sync);
        if (e == hipSuccess) e = host_.grow(bytes, cap_bytes, nullptr);
        if (e == hipSuccess && !ev_) e = hipEventCreateWithFlags(&ev_, hipEventDisableTiming);
        if (e != hipSuccess) { dev_.reset(); host_.reset(); }
        return e;
    }
    // host() -> device() on stream s, and nothing else
    hipError_t copy(size_t bytes, hipStream_t s) { return hipMemcpyAsync(dev_.get(), host_.get(), bytes, hipMemcpyHostToDevice, s); }
    // the event follows what s holds now: the copy alone (send), or the kernel that reads device() as well
    hipError_t mark(hipStream_t s) {
        const hipError_t e = hipEventRecord(ev_, s);
        busy_ = e == hipSuccess;
        return e;
    }
    hipError_t send(size_t bytes, hipStream_t s) {
        const hipError_t e = copy(bytes, s);
        return e != hipSuccess ? e : mark(s);
    }
    void reset() {
        dev_.reset();
        host_.reset();
        if (ev_) (void)hipEventDestroy(ev_);
        ev_ = nullptr;
        busy_ = false;
    }

  private:
    DevBuf<char> dev_;
    DevBuf<char, true> host_;
    hipEvent_t ev_ = nullptr;
    bool busy_ = false;
};

}  // namespace bce
