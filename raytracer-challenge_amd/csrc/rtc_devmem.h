// rtc_devmem.h — how the host code owns device memory: DevBuf, one grow-only hipMalloc'd array. Every device buffer of
// librtc.so is one. Not part of the ABI.
#ifndef RTC_DEVMEM_H
#define RTC_DEVMEM_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rtc.h"

// RTC_ERR_NOMEM when HIP is out of memory, RTC_ERR_DEVICE for any other failure.
inline rtc_status rtc_status_of(hipError_t e) {
    return e == hipSuccess ? RTC_OK : e == hipErrorOutOfMemory ? RTC_ERR_NOMEM : RTC_ERR_DEVICE;
}

// At most one device array of T. It is freed with whatever device is current: its owner makes its own device current
// before it lets go, and frees nothing that a stream may still use.
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_;
            cap_ = o.cap_;
            o.p_ = nullptr;
            o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    T *get() const { return p_; }
    size_t capacity() const { return cap_; } // elements

    // Room for n elements. Nothing happens when there is room already; otherwise the old array is freed first (hipFree
    // waits for the device), then n elements are allocated. On failure HIP's sticky error is cleared and the buffer is
    // empty. `allocs`, when given, counts the hipMalloc call.
    rtc_status reserve(size_t n, unsigned long long *allocs = nullptr) {
        if (n <= cap_) return RTC_OK;
        reset();
        if (allocs) ++*allocs;
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p_), n * sizeof(T));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            p_ = nullptr;
            return rtc_status_of(e);
        }
        cap_ = n;
        return RTC_OK;
    }
    // reserve(n), then n elements from the host
    rtc_status upload(const T *src, size_t n) {
        const rtc_status st = reserve(n);
        return st != RTC_OK ? st : rtc_status_of(hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice));
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }

private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};

// One page-locked 32-bit word of host memory, the landing place of a count that the host reads after a stream wait.
// Allocated on first use, freed with its owner.
class PinnedWord {
public:
    PinnedWord() = default;
    PinnedWord(const PinnedWord &) = delete;
    PinnedWord &operator=(const PinnedWord &) = delete;
    ~PinnedWord() {
        if (p_) (void)hipHostFree(p_);
    }
    rtc_status ready() {
        if (p_) return RTC_OK;
        const hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p_), sizeof(uint32_t), hipHostMallocDefault);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            p_ = nullptr;
        }
        return rtc_status_of(e);
    }
    uint32_t *get() const { return p_; }

private:
    uint32_t *p_ = nullptr;
};

#endif
