// vf_device_buf.hpp -- the owner of a block of memory made after creation: on first use, or grown on demand.  Device memory
// (DeviceBuf) or pinned host memory (PinnedBuf).  Move-only; the destructor frees.  The four HIP calls below are all it uses
// (tests/native/device_buf.cpp stubs them and checks it on the CPU).  Event owns an event likewise (tests/native/upload_channel.cpp).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace vf {

inline size_t exact(size_t bytes) { return bytes; }
inline size_t twice(size_t bytes) { return 2 * bytes; }

template <typename T, bool PINNED>
class LateBuf {
  public:
    LateBuf() = default;
    LateBuf(LateBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    LateBuf& operator=(LateBuf&& o) noexcept {
        if (this != &o) release(), p_ = std::exchange(o.p_, nullptr), bytes_ = std::exchange(o.bytes_, 0);
        return *this;
    }
    ~LateBuf() { release(); }
    // The block as it is if it holds `bytes`; else it is freed and one of headroom(bytes) allocated (the contents are not
    // carried over).  A failure leaves the owner empty.  Work in flight that uses the old block is the caller's to wait for.
    hipError_t ensure(size_t bytes, size_t (*headroom)(size_t) = exact) {
        if (bytes <= bytes_) return hipSuccess;
        release();
        void* q = nullptr;
        const hipError_t err = PINNED ? hipHostMalloc(&q, headroom(bytes), hipHostMallocDefault) : hipMalloc(&q, headroom(bytes));
        if (err == hipSuccess) p_ = (T*)q, bytes_ = headroom(bytes);
        return err;
    }
    void release() {
        if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr, bytes_ = 0;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    size_t bytes() const { return bytes_; }

  private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
};
template <typename T> using DeviceBuf = LateBuf<T, false>;
template <typename T> using PinnedBuf = LateBuf<T, true>;

class Event {
  public:
    Event() = default;
    Event(Event&& o) noexcept : ev_(std::exchange(o.ev_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) release(), ev_ = std::exchange(o.ev_, nullptr);
        return *this;
    }
    ~Event() { release(); }
    // The event as it is if there is one (whatever its flags); else one made with `flags`
    hipError_t ensure(unsigned flags = hipEventDefault) { return ev_ ? hipSuccess : hipEventCreateWithFlags(&ev_, flags); }
    void release() { if (ev_) (void)hipEventDestroy(std::exchange(ev_, nullptr)); }
    operator hipEvent_t() const { return ev_; }

  private:
    hipEvent_t ev_ = nullptr;
};

}  // namespace vf
