// The host side of ONE small-problem batch launch, described once (capi_small.hip has the six drivers): the pieces of the call's work
// buffer, the ticket, the per-restart records, and the arithmetic the drivers and the launchers of small_batch.h share (tickets, the
// workgroup size of the wide kernels, kernel names).  Host code over the HIP runtime API and dev_buf.h only: no context, no kernel
// header, no messages -- a hipError_t comes back and the driver words the refusal.  tests/host/batch_call_selftest.cpp runs all of it
// on the CPU against a stand-in runtime.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "dev_buf.h"

namespace qcqpmi {

// A driver DECLARES its arrays in the order they lie in the work buffer, each with the slot of the kernel's argument struct that will
// point at it; reserve() lays them out (every piece 256-byte aligned, an empty one takes no room) and only then fills the slots;
// upload() and download() enqueue the copies.  Nothing waits: spin_sync is the driver's.
struct BatchCall {
    struct Piece { size_t off, bytes; const void *src; void *slot; };
    struct Fetch { int piece; void *dst; };
    std::vector<Piece> pieces;
    std::vector<Fetch> fetches;      // in the order they will be enqueued
    size_t total = 0;                // bytes asked of the buffer
    char *w = nullptr;               // the buffer, once reserved
    int iticket = -1;

    // `bytes` of the buffer; *slot (a T *, nulled here) gets its address at reserve(), or stays null for an empty piece
    template <class T>
    int room(size_t bytes, T **slot) {
        *slot = nullptr;
        pieces.push_back({total, bytes, nullptr, (void *)slot});
        total += (bytes + 255) / 256 * 256;
        return (int)pieces.size() - 1;
    }
    // an input: uploaded from src; a missing one (src == nullptr) takes no room
    template <class T>
    int in(const void *src, size_t bytes, T **slot) { const int i = room(src ? bytes : 0, slot); pieces[(size_t)i].src = src; return i; }
    // an output: downloaded to dst unless that is null.  fetch(): piece i comes down at THIS place of the order (an output that does
    // not lie where it is fetched: room() first, fetch() later)
    template <class T>
    int out(void *dst, size_t bytes, T **slot) { const int i = room(bytes, slot); fetch(i, dst); return i; }
    void fetch(int i, void *dst) { fetches.push_back({i, dst}); }
    // the two ints every batch kernel draws its work from: [0] the next ticket, [1] "a matrix is not symmetric"; zeroed by upload()
    void ticket(int **slot) { iticket = room(2 * sizeof(int), slot); }

    hipError_t reserve(DevBuf<char> &buf, hipStream_t st) {
        const hipError_t e = buf.reserve(st, total, false);
        if (e != hipSuccess) return e;
        w = buf.p;
        for (const Piece &p : pieces) {
            char *at = p.bytes ? w + p.off : nullptr;
            memcpy(p.slot, &at, sizeof(at));      // every slot is an object pointer
        }
        return hipSuccess;
    }

    hipError_t upload(hipStream_t st) const {
        for (const Piece &p : pieces)
            if (p.src && p.bytes) {
                const hipError_t e = hipMemcpyAsync(w + p.off, p.src, p.bytes, hipMemcpyHostToDevice, st);
                if (e != hipSuccess) return e;
            }
        return iticket < 0 ? hipSuccess : hipMemsetAsync(w + pieces[(size_t)iticket].off, 0, 2 * sizeof(int), st);
    }

    hipError_t download(hipStream_t st) const {
        for (const Fetch &f : fetches) {
            const Piece &p = pieces[(size_t)f.piece];
            if (!f.dst || !p.bytes) continue;
            const hipError_t e = hipMemcpyAsync(f.dst, w + p.off, p.bytes, hipMemcpyDeviceToHost, st);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
};

// ---- the per-restart records of the CD, ADMM and chain kernels: ONE block of the work buffer, array after array, `count` entries each.
// restart_records is the table: every array once, as (host destination, the kernel's pointer), widest entries first so that every
// array is aligned whatever the count.  A CD block holds the arrays marked REC_CD (4 x int64, 2 x double, 2 x int, 1 x uint8: 57
// bytes per restart), an ADMM block those marked REC_ADMM (2 x int64, 2 x double: 32), a chain's block all of them (73), every array
// [stages][restarts].  H: RecordsOut; K: the kernel's struct, which names its pointers alike (CdSmallArgs, AdmmSmallArgs, ChainStage).
enum { REC_CD = 1, REC_ADMM = 2 };

struct RecordsOut {      // where the caller wants them; any may be null
    int64_t *sweeps1, *sweeps2, *visits2, *accepted2, *iters1, *iters2;
    double *f0, *maxviol;
    int *status1, *status2;
    uint8_t *ran2;
};

template <int WHICH, class H, class K, class F>
inline void restart_records(const H &h, K &k, F &f) {
    if constexpr ((WHICH & REC_CD) != 0) { f(h.sweeps1, k.sweeps1); f(h.sweeps2, k.sweeps2); f(h.visits2, k.visits2); f(h.accepted2, k.accepted2); }
    if constexpr ((WHICH & REC_ADMM) != 0) { f(h.iters1, k.iters1); f(h.iters2, k.iters2); }
    f(h.f0, k.f0); f(h.maxviol, k.maxviol);
    if constexpr ((WHICH & REC_CD) != 0) { f(h.status1, k.status1); f(h.status2, k.status2); f(h.ran2, k.ran2); }
}

// What a walk over the table does with the entries [row, row + take) of every array: with `dev`, the kernel's pointers get their
// address in the block there; with `host`, the block's copy there, they go to the destinations that are not null.  `at` ends as the
// size of the block.  A chain's stage s is row = s restarts; the single kernels have row = 0, take = count.
struct RecordWalk {
    size_t count, row, take;
    char *dev;
    const char *host;
    size_t at = 0;
    template <class T>
    void operator()(T *dst, T *&k) {
        if (dev) k = (T *)(dev + at) + row;
        if (host && dst) memcpy(dst, (const T *)(host + at) + row, take * sizeof(T));
        at += count * sizeof(T);
    }
};

template <int WHICH>
inline size_t record_block_bytes(size_t count) {
    RecordsOut none{}, k{};
    RecordWalk size{count, 0, 0, nullptr, nullptr};
    restart_records<WHICH>(none, k, size);
    return size.at;
}

// k's pointers -> stage `stage` of the block at dev (arrays of stages x T entries)
template <int WHICH, class K>
inline void bind_records(K &k, char *dev, size_t T, size_t stages = 1, size_t stage = 0) {
    RecordWalk bind{stages * T, stage * T, T, dev, nullptr};
    restart_records<WHICH>(RecordsOut{}, k, bind);
}

// the downloaded block -> the caller's arrays: `take` entries from `row` on of every array of `count`
template <int WHICH>
inline void unpack_records(const RecordsOut &h, const char *host, size_t count, size_t row, size_t take) {
    RecordsOut k{};
    RecordWalk unpack{count, row, take, nullptr, host};
    restart_records<WHICH>(h, k, unpack);
}

// ---- Tickets of a launch over B problems with R restarts each on `wgs` resident workgroups of `waves` wavefronts: whole problems when
// there are enough of them to fill the device, else chunks of RC consecutive restarts, at least one restart per wave of a workgroup.
struct TicketPlan { int64_t RC, chunks; int wgs; };      // restarts per ticket, tickets per problem, workgroups (at most one per ticket)

inline TicketPlan ticket_partition(int64_t B, int64_t R, int wgs, int64_t waves) {
    int64_t chunks = B >= wgs ? 1 : (wgs + B - 1) / B;
    if (chunks > (R + waves - 1) / waves) chunks = (R + waves - 1) / waves;
    TicketPlan t;
    t.RC = (R + chunks - 1) / chunks;
    t.chunks = (R + t.RC - 1) / t.RC;
    t.wgs = wgs > B * t.chunks ? (int)(B * t.chunks) : wgs;
    return t;
}

// The workgroup of a wide ticket kernel, 256 threads or `large`: the one that puts more waves on a CU, given the workgroups per CU the
// occupancy query answers for each; a tie goes to the larger.  While three images fit a CU (n = 72: 41 KB each) four waves of each
// beat the eight of one workgroup; from n = 101 there is one image and eight waves beat four (measured: profiles/r12_wide_batch.md).
inline int batch_wide_threads(int per_small, int per_large, int large) { return per_large * large >= per_small * 256 ? large : 256; }

// "<base><MAXC[,pc][,w2]>", MAXC = 1 or 4: what qcqpmi_last_cd_kernel and its like hand out, so the text lives as long as the
// process.  Tag: one table of eight per kernel family (its argument struct).
template <class Tag>
inline const char *batch_kernel_name(const char *base, int maxc, bool pc, bool wide) {
    struct Table {
        char s[8][48];
        explicit Table(const char *b) { for (int v = 0; v < 8; v++) snprintf(s[v], 48, "%s<%d%s%s>", b, v & 4 ? 4 : 1, v & 2 ? ",pc" : "", v & 1 ? ",w2" : ""); }
    };
    static const Table t(base);
    return t.s[(maxc <= 1 ? 0 : 4) | (pc ? 2 : 0) | (wide ? 1 : 0)];
}

}  // namespace qcqpmi
