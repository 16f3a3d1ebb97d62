// vf_upload_channel.hpp -- how a per-call block of arguments reaches the device without the host waiting for it: a pinned host
// block, its device twin, three events and what is known of the last send.  The protocol, once:
//   open(bytes)    the pinned block to fill.  If either block is too small, both are regrown (vf::twice) -- behind the last event of
//                  an outstanding send (its kernel's; its copy's if no launched() followed): a kernel may still read the device
//                  block about to go.  Then the outstanding send's copy is waited for (long done): it reads the pinned block.
//   send(...)      the copy on the caller's stream, between ev0 and ev1 (timed) or in front of ev1 alone (untimed)
//   launched(s)    ev2 behind what the caller has launched on the block: the send is complete
//   timings(...)   of a send that is timed and complete: waits for ev2; copy = ev0 -> ev1, kernel = ev1 -> ev2.  Of any other: zeros.
// A channel serves one call at a time; calls that may be in flight beside each other take a channel each.  Like vf_device_buf.hpp
// this needs <hip/hip_runtime_api.h> alone: tests/native/upload_channel.cpp stubs the calls made here and checks their order on the CPU.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "vf_device_buf.hpp"

namespace vf {

// One account of a packed block: add(bytes) is where the next segment starts, always a multiple of 8
struct Packed {
    size_t bytes = 0;
    size_t add(size_t n) { return std::exchange(bytes, (bytes + n + 7) & ~(size_t)7); }
};

class UploadChannel {
  public:
    hipError_t open(size_t bytes, char** host) {
        hipError_t err;
        for (Event& ev : ev_)
            if ((err = ev.ensure()) != hipSuccess) return err;
        if (bytes > host_.bytes() || bytes > dev_.bytes()) {
            if (sent_ && (err = hipEventSynchronize(ev_[complete_ ? 2 : 1])) != hipSuccess) return err;
            if ((err = host_.ensure(bytes, twice)) != hipSuccess || (err = dev_.ensure(bytes, twice)) != hipSuccess) return err;
        }
        if (sent_ && (err = hipEventSynchronize(ev_[1])) != hipSuccess) return err;
        *host = host_;
        return hipSuccess;
    }
    hipError_t send(size_t bytes, hipStream_t stream, bool timed) {
        hipError_t err;
        if (timed && (err = hipEventRecord(ev_[0], stream)) != hipSuccess) return err;
        if ((err = hipMemcpyAsync(dev_, host_, bytes, hipMemcpyHostToDevice, stream)) != hipSuccess) return err;
        sent_ = true, timed_ = timed, complete_ = false;
        return hipEventRecord(ev_[1], stream);
    }
    hipError_t launched(hipStream_t stream) {
        const hipError_t err = hipEventRecord(ev_[2], stream);
        complete_ = err == hipSuccess;
        return err;
    }
    hipError_t timings(float* h2d_ms, float* kernel_ms) {
        if (h2d_ms) *h2d_ms = 0.f;
        if (kernel_ms) *kernel_ms = 0.f;
        if (!(timed_ && complete_)) return hipSuccess;
        hipError_t err = hipEventSynchronize(ev_[2]);
        if (err == hipSuccess && h2d_ms) err = hipEventElapsedTime(h2d_ms, ev_[0], ev_[1]);
        if (err == hipSuccess && kernel_ms) err = hipEventElapsedTime(kernel_ms, ev_[1], ev_[2]);
        return err;
    }
    char* device() const { return dev_; }       // the twin of what open() handed out
    bool outstanding() const { return sent_; }  // something has been sent (and may have reported: the ingest's status word)

  private:
    PinnedBuf<char> host_;
    DeviceBuf<char> dev_;
    Event ev_[3];
    bool sent_ = false, timed_ = false, complete_ = false;   // the last send: there is one / ev0 is its own / launched() followed it
};

}  // namespace vf
