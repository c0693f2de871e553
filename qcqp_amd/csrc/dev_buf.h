// Owning buffers of the host side of the C ABI: DevBuf<T> (device memory) and PinBuf<T> (pinned host memory).  Host code only,
// no kernel; the ONE place of the library that allocates and frees through the HIP runtime.  A buffer frees what it holds when it
// goes out of scope; reserve() is the grow-only rule every site used to write out by hand.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

// Busy-wait for the stream.  hipStreamSynchronize and the implicit wait of a pageable copy go to sleep in slices once a kernel
// has run for a few milliseconds and wake up 10-30 ms late in about one call of four on this stack (measured round 6 with the 34 ms
// lifecycle launch: tools/timed_region_probe.py, profiles/r06_timed_region.md); the long launches of the coordinate-descent paths
// are therefore awaited by polling hipStreamQuery -- one host core spins for the length of the launch.
inline hipError_t spin_sync(hipStream_t st) {
    for (;;) {
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e;
    }
}

template <class T, bool Pinned = false>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;      // elements behind p

    DevBuf() = default;
    DevBuf(T *q, size_t count) : p(q), cap(count) {}      // adopts what take() gave away
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    ~DevBuf() { release(); }

    operator T *() const { return p; }

    // At least `count` elements afterwards (an empty buffer allocates even for count == 0: one element, so that p is a valid
    // address).  Growth waits for `st` (work in flight may still read the old block), drops what the buffer held and allocates
    // afresh; zero: the new block is cleared on `st`.  A failed growth leaves {nullptr, 0}.
    hipError_t reserve(hipStream_t st, size_t count, bool zero = true) {
        if (p && count <= cap) return hipSuccess;
        if (p) {
            const hipError_t e = spin_sync(st);
            if (e != hipSuccess) return e;
            release();
        }
        const size_t bytes = (count > 0 ? count : 1) * sizeof(T);
        void *v = nullptr;
        hipError_t e = Pinned ? hipHostMalloc(&v, bytes, hipHostMallocDefault) : hipMalloc(&v, bytes);
        if (e != hipSuccess) return e;
        p = (T *)v;
        if (zero && (e = hipMemsetAsync(p, 0, bytes, st)) != hipSuccess) { release(); return e; }
        cap = count;
        return hipSuccess;
    }

    void release() {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr; cap = 0;
    }

    T *take() { T *q = p; p = nullptr; cap = 0; return q; }      // the caller owns the block now
};

template <class T>
using PinBuf = DevBuf<T, true>;
