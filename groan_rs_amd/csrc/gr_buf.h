// gr_buf.h -- the grow-only buffers of a context and its plans.  No HIP header in here: include it behind hip/hip_runtime.h, or (as
// tests/test_buf_host.py does) behind stand-ins for hipMalloc / hipFree / hipHostMalloc / hipHostFree.
//
// reserve(need, headroom) does nothing while need <= cap(); else it frees the block (its contents are NOT kept; the caller has made
// sure that nobody reads it any more), allocates headroom(need) elements and records that as the capacity.  After a failed allocation
// pointer and capacity are null and 0: the next call tries again.  The destructor frees: destroy the owner with its device set, streams idle.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstring>

namespace grbuf {

// headroom policies: elements to allocate when `need` no longer fits
inline size_t exact(size_t need) { return need; }
inline size_t quarter(size_t need) { return need + need / 4; }
inline size_t quarter_aligned256(size_t need) { return (need + need / 4 + 255) & ~(size_t)255; }
inline size_t eighth_plus_64(size_t need) { return need + need / 8 + 64; }

template <class T, bool Host>
class Buf {
    T *p_ = nullptr;
    size_t cap_ = 0;
    static hipError_t alloc(T **p, size_t n) {
        return Host ? hipHostMalloc((void **)p, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)p, n * sizeof(T));
    }
public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { release(); }
    T *get() const { return p_; }
    size_t cap() const { return cap_; }
    void release() {
        if (p_) { if (Host) (void)hipHostFree(p_); else (void)hipFree(p_); }
        p_ = nullptr; cap_ = 0;
    }
    // *grew (when given): a new block was allocated (its contents are undefined)
    template <class Headroom>
    hipError_t reserve(size_t need, Headroom headroom, bool *grew = nullptr) {
        if (grew) *grew = false;
        if (need <= cap_) return hipSuccess;
        release();
        const size_t n = headroom(need);
        const hipError_t e = alloc(&p_, n);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        cap_ = n;
        if (grew) *grew = true;
        return hipSuccess;
    }
    // ... the same, but the first keep_bytes bytes of the old block (when there was one; no more than it or the new one holds) are in
    // the new one: the host copies them
    template <class Headroom>
    hipError_t reserve_keep(size_t need, Headroom headroom, size_t keep_bytes) {
        static_assert(Host, "pinned blocks only");
        if (need <= cap_) return hipSuccess;
        const size_t n = headroom(need);
        T *bigger = nullptr;
        const hipError_t e = alloc(&bigger, n);
        if (e == hipSuccess && p_) memcpy(bigger, p_, std::min(keep_bytes, std::min(cap_, n) * sizeof(T)));
        release();
        if (e != hipSuccess) return e;
        p_ = bigger; cap_ = n;
        return hipSuccess;
    }
};

template <class T> using Dev = Buf<T, false>;        // device memory
template <class T> using Pinned = Buf<T, true>;      // pinned host memory

}  // namespace grbuf
