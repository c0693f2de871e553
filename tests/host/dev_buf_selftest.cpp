// Stand-alone check of qcqp_amd/csrc/dev_buf.h on the CPU: built with the host compiler and the sanitizers, linked against the
// stand-in runtime below instead of libamdhip64.  The stand-ins count live blocks, abort on a free of a block that is not live
// and can make the next allocation fail.  Exit status 0 and "ok" on stdout: every check held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>

#include "../../qcqp_amd/csrc/dev_buf.h"

namespace {
std::set<void *> live_dev, live_pin;
int fail_next = 0;        // allocations to refuse from now on
int allocs = 0, frees = 0, memsets = 0, queries = 0;

hipError_t fake_alloc(std::set<void *> &live, void **ptr, size_t size) {
    if (fail_next > 0) { fail_next--; *ptr = nullptr; return hipErrorOutOfMemory; }
    if (size == 0) { fprintf(stderr, "allocation of 0 bytes\n"); abort(); }
    void *p = malloc(size);
    memset(p, 0xA5, size);
    live.insert(p);
    allocs++;
    *ptr = p;
    return hipSuccess;
}

hipError_t fake_free(std::set<void *> &live, void *p) {
    if (!p) return hipSuccess;
    if (!live.erase(p)) { fprintf(stderr, "free of a block that is not live (double free, or the wrong kind of memory)\n"); abort(); }
    free(p);
    frees++;
    return hipSuccess;
}

size_t live_total() { return live_dev.size() + live_pin.size(); }

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)
}  // namespace

extern "C" {
hipError_t hipMalloc(void **ptr, size_t size) { return fake_alloc(live_dev, ptr, size); }
hipError_t hipFree(void *p) { return fake_free(live_dev, p); }
hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int) { return fake_alloc(live_pin, ptr, size); }
hipError_t hipHostFree(void *p) { return fake_free(live_pin, p); }
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t) {
    if (!live_dev.count(dst) && !live_pin.count(dst)) { fprintf(stderr, "memset of a block that is not live\n"); abort(); }
    memset(dst, value, bytes);
    memsets++;
    return hipSuccess;
}
hipError_t hipStreamQuery(hipStream_t) { queries++; return hipSuccess; }
}

template <class Buf>
void checks() {
    const size_t before = live_total();
    {
        Buf b;
        CHECK(b.p == nullptr && b.cap == 0 && !b);
        // first reservation: allocates, zeroes, sets the capacity; no wait for the stream (there is nothing to free)
        const int q0 = queries;
        CHECK(b.reserve(nullptr, 100) == hipSuccess);
        CHECK(b.p && b.cap == 100 && live_total() == before + 1 && queries == q0);
        for (size_t i = 0; i < 100; i++) CHECK(b.p[i] == 0);
        // count <= cap: nothing happens
        auto *p0 = b.p;
        const int a0 = allocs, f0 = frees, m0 = memsets;
        CHECK(b.reserve(nullptr, 100) == hipSuccess && b.reserve(nullptr, 1) == hipSuccess && b.reserve(nullptr, 0) == hipSuccess);
        CHECK(b.p == p0 && b.cap == 100 && allocs == a0 && frees == f0 && memsets == m0 && queries == q0);
        // growth: waits for the stream, frees the old block, allocates the new one; zero = false leaves it as allocated
        CHECK(b.reserve(nullptr, 300, false) == hipSuccess);
        CHECK(b.cap == 300 && allocs == a0 + 1 && frees == f0 + 1 && memsets == m0 && queries == q0 + 1 && live_total() == before + 1);
        CHECK(((unsigned char *)b.p)[0] == 0xA5);
        // a failed growth leaves {nullptr, 0} (the old block is gone, no stale capacity) ...
        fail_next = 1;
        CHECK(b.reserve(nullptr, 1000) != hipSuccess);
        CHECK(b.p == nullptr && b.cap == 0 && live_total() == before);
        // ... and a later, smaller request allocates again
        CHECK(b.reserve(nullptr, 10) == hipSuccess);
        CHECK(b.p && b.cap == 10 && live_total() == before + 1);
        // the conversion the call sites rely on: pointer arithmetic, indexing, truth value
        auto *raw = b + 3;
        CHECK(raw == b.p + 3 && &b[2] == b.p + 2 && b);
        // take(): the block changes owner and is not freed
        const int f1 = frees;
        auto *mine = b.take();
        CHECK(mine && b.p == nullptr && b.cap == 0 && frees == f1 && live_total() == before + 1);
        Buf c(mine, 10);                 // adopted by another buffer ...
        Buf d(std::move(c));             // ... and moved: one owner at any time
        CHECK(c.p == nullptr && c.cap == 0 && d.p == mine && d.cap == 10);
        // an empty buffer asked for 0 elements still gets an address (one element)
        Buf e;
        CHECK(e.reserve(nullptr, 0, false) == hipSuccess && e.p && live_total() == before + 2);
        // release(): frees and resets; a second one is a no-op
        e.release();
        e.release();
        CHECK(e.p == nullptr && e.cap == 0 && live_total() == before + 1);
    }
    CHECK(live_total() == before);       // nothing is live after destruction
}

int main() {
    checks<DevBuf<double>>();
    CHECK(live_pin.empty());             // device buffers never touch pinned memory
    checks<PinBuf<int>>();
    CHECK(live_dev.empty() && live_pin.empty() && allocs == frees);
    printf("ok\n");
    return 0;
}
