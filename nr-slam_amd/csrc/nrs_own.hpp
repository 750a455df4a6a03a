// Owners of the GPU resources the library holds: device buffers, pinned host memory, streams, events.  Each is move-only and gives its
// resource back in its destructor, through one of four functions that nrs_ctx.hip defines with the HIP calls (host/ctx_check.cpp defines
// counting ones: the header includes no HIP header).  No owner may have static or thread-local storage: its destructor would call into a
// HIP runtime that is already gone at process exit.  Structs passed to kernels by value hold plain pointers, never an owner.
#pragma once
#include <cstddef>
#include <memory>
#include <utility>

struct ihipStream_t;   // hipStream_t and hipEvent_t are pointers to these
struct ihipEvent_t;

namespace nrs {

// all four ignore null
void dev_free(void* p) noexcept;
void pin_free(void* p) noexcept;
void stream_destroy(ihipStream_t* s) noexcept;
void event_destroy(ihipEvent_t* e) noexcept;

// what nrs_ctx::ensure allocates for a request of `bytes`: a quarter of headroom, so that a slowly growing frame does not reallocate each time
inline size_t grown_bytes(size_t bytes) { return bytes + bytes / 4 + 256; }

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); } return *this; }
    ~DevBuf() { reset(); }
    void reset() noexcept { dev_free(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct PinBuf {
    void* p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(PinBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    PinBuf& operator=(PinBuf&& o) noexcept { if (this != &o) { reset(); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); } return *this; }
    ~PinBuf() { reset(); }
    void reset() noexcept { pin_free(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct StreamDestroy { void operator()(ihipStream_t* s) const noexcept { stream_destroy(s); } };
struct EventDestroy { void operator()(ihipEvent_t* e) const noexcept { event_destroy(e); } };
using Stream = std::unique_ptr<ihipStream_t, StreamDestroy>;
using Event = std::unique_ptr<ihipEvent_t, EventDestroy>;

}  // namespace nrs
