// Owners of the HIP handles a call creates and a guard for the engine state it sets: the engine reports
// errors by throwing, and a throw anywhere must leave nothing allocated, captured or half-set behind.
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>

namespace dsocr {

#define HIP_CHECK(x)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (x);                                                                           \
        if (_e != hipSuccess)                                                                          \
            throw std::runtime_error(std::string("EDEVICE: ") + #x + ": " + hipGetErrorString(_e));    \
    } while (0)

class HipEvent {
  public:
    explicit HipEvent(unsigned flags = 0) { HIP_CHECK(flags ? hipEventCreateWithFlags(&e_, flags) : hipEventCreate(&e_)); }
    ~HipEvent() { if (e_) (void)hipEventDestroy(e_); }
    HipEvent(HipEvent&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    HipEvent& operator=(HipEvent&& o) noexcept { std::swap(e_, o.e_); return *this; }
    operator hipEvent_t() const { return e_; }

  private:
    hipEvent_t e_ = nullptr;
};

// an instantiated graph with the hipGraph_t it came from (empty until it is given one)
class HipGraphExec {
  public:
    HipGraphExec() = default;
    explicit HipGraphExec(hipGraph_t g) : HipGraphExec() {  // (delegating: a failed instantiate still destroys g)
        g_ = g;
        HIP_CHECK(hipGraphInstantiate(&x_, g_, nullptr, nullptr, 0));
    }
    ~HipGraphExec() {
        if (x_) (void)hipGraphExecDestroy(x_);
        if (g_) (void)hipGraphDestroy(g_);
    }
    HipGraphExec(HipGraphExec&& o) noexcept : g_(std::exchange(o.g_, nullptr)), x_(std::exchange(o.x_, nullptr)) {}
    HipGraphExec& operator=(HipGraphExec&& o) noexcept { std::swap(g_, o.g_); std::swap(x_, o.x_); return *this; }
    explicit operator bool() const { return x_ != nullptr; }
    void launch(hipStream_t st) const { HIP_CHECK(hipGraphLaunch(x_, st)); }

  private:
    hipGraph_t g_ = nullptr;
    hipGraphExec_t x_ = nullptr;
};

// A thread-local capture on a stream; `capturing` (Engine::capturing_) is true exactly while it is open.
// Unwinding past an open capture ends it and drops the graph, so the stream stays usable.
class StreamCapture {
  public:
    StreamCapture(hipStream_t st, bool& capturing) : st_(st), capturing_(capturing) {
        HIP_CHECK(hipStreamBeginCapture(st_, hipStreamCaptureModeThreadLocal));
        capturing_ = true;
    }
    StreamCapture(const StreamCapture&) = delete;
    StreamCapture& operator=(const StreamCapture&) = delete;
    ~StreamCapture() {
        if (!capturing_) return;
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(st_, &g);  // (an invalidated capture reports an error here: nothing to do about it)
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        capturing_ = false;
    }
    HipGraphExec finish() {
        hipGraph_t g = nullptr;
        capturing_ = false;
        HIP_CHECK(hipStreamEndCapture(st_, &g));
        return HipGraphExec(g);
    }

  private:
    hipStream_t st_;
    bool& capturing_;
};

template <typename T>
class PinnedBuffer {
  public:
    PinnedBuffer() = default;
    explicit PinnedBuffer(size_t n) { HIP_CHECK(hipHostMalloc((void**)&p_, sizeof(T) * n)); }
    ~PinnedBuffer() { if (p_) (void)hipHostFree(p_); }
    PinnedBuffer(PinnedBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    PinnedBuffer& operator=(PinnedBuffer&& o) noexcept { std::swap(p_, o.p_); return *this; }
    operator T*() const { return p_; }

  private:
    T* p_ = nullptr;
};

// a device allocation of its own (beside the engine's named workspaces); throws ENOMEM when hipMalloc fails
class DeviceBuffer {
  public:
    DeviceBuffer() = default;
    explicit DeviceBuffer(size_t bytes) : bytes_(bytes) {
        if (hipMalloc(&p_, bytes ? bytes : 16) != hipSuccess) {
            (void)hipGetLastError();
            p_ = nullptr;
            throw std::runtime_error("ENOMEM: hipMalloc(" + std::to_string(bytes) + ") failed");
        }
    }
    ~DeviceBuffer() { if (p_) (void)hipFree(p_); }
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); return *this; }
    void* get() const { return p_; }
    size_t bytes() const { return bytes_; }

  private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
};

// sets `ref` for the scope and puts the old value back on every exit
template <typename T>
class ScopedSet {
  public:
    ScopedSet(T& ref, std::common_type_t<T> value) : ref_(ref), old_(std::exchange(ref, std::move(value))) {}
    ScopedSet(const ScopedSet&) = delete;
    ScopedSet& operator=(const ScopedSet&) = delete;
    ~ScopedSet() { ref_ = std::move(old_); }

  private:
    T& ref_;
    T old_;
};

}  // namespace dsocr
