// device_mem.hpp — move-only owners of what the host layer (sixdof_capi.cpp) holds of the runtime: device buffers, streams,
// events, dlopen handles and page-locked host ranges.  The only place that calls hipFree / hipStreamDestroy /
// hipEventDestroy / hipHostUnregister / dlclose: a member of one of these types is released when it is reset, replaced
// or destroyed, so an early return can neither leak it nor leave a freed pointer behind.  Nothing virtual: get() is the
// stored value.
#pragma once
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace sixdof {

// One runtime object of type T (a pointer; null: none), released by Free.  out() is where a creation call stores it.
template <class T, class Free>
class Owner {
    T v_{};
  public:
    Owner() = default;
    Owner(Owner&& o) noexcept : v_(std::exchange(o.v_, T{})) {}
    Owner& operator=(Owner&& o) noexcept {
        if (this != &o) reset(), v_ = std::exchange(o.v_, T{});
        return *this;
    }
    ~Owner() { reset(); }
    T get() const { return v_; }
    explicit operator bool() const { return v_ != T{}; }
    T* out() { return reset(), &v_; }
    void reset() {
        if (v_) Free{}(v_);
        v_ = T{};
    }
};
struct StreamFree { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
struct EventFree { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct DlFree { void operator()(void* dl) const { dlclose(dl); } };
using Stream = Owner<hipStream_t, StreamFree>;
using Event = Owner<hipEvent_t, EventFree>;
using DlHandle = Owner<void*, DlFree>;

// A device allocation and its size: empty (null, 0 bytes) or alloc()'s, never in between.
class DeviceBuffer {
    void* p_ = nullptr;
    size_t bytes_ = 0;
  public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        if (this != &o) reset(), p_ = std::exchange(o.p_, nullptr), bytes_ = std::exchange(o.bytes_, 0);
        return *this;
    }
    ~DeviceBuffer() { reset(); }
    // frees what it held first; on failure it is empty
    hipError_t alloc(size_t bytes) {
        reset();
        const hipError_t e = hipMalloc(&p_, bytes);
        if (e == hipSuccess) bytes_ = bytes;
        else p_ = nullptr;
        return e;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        release();
    }
    // gives the allocation up without freeing it (something may still read it)
    void* release() { return bytes_ = 0, std::exchange(p_, nullptr); }
    template <class T = void> T* get() const { return static_cast<T*>(p_); }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }
};

// A host range this library page-locked.  A range that cannot be locked stays pageable (copies are then staged): no error.
struct PinnedFree { void operator()(void* p) const { (void)hipHostUnregister(p); } };
class PinnedRange : public Owner<void*, PinnedFree> {
    size_t bytes_ = 0;   // of the range while it is locked
  public:
    bool lock(void* p, size_t bytes) {
        reset();
        if (hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess) return *out() = p, bytes_ = bytes, true;
        return (void)hipGetLastError(), false;
    }
    // how [p, p + bytes) lies to the locked range
    bool contains(const void* p, size_t bytes) const {
        const char *lo = static_cast<const char*>(get()), *q = static_cast<const char*>(p);
        return lo && lo <= q && q + bytes <= lo + bytes_;
    }
    bool intersects(const void* p, size_t bytes) const {
        const char *lo = static_cast<const char*>(get()), *q = static_cast<const char*>(p);
        return lo && lo < q + bytes && q < lo + bytes_;
    }
};

}  // namespace sixdof
