// Small-problem batch: what the batch kernels (cd_small.hip, admm_small.hip, chain_small.hip, sdr_small.hip) and their drivers
// (capi_small.hip) share.  chain_small.hip runs the chain frame at the end of this file, the ticket frame with stages.
//
// The ticket frame.  A persistent workgroup draws a ticket -- a problem b and a chunk [r_lo, r_hi) of its R restarts -- from a global
// counter (an ordinary atomic add), stages the problem's LDS image once
//        A_b [n][n] | q0_b [n] | per-problem coefficients [3][m] (p, then q, then r; PC only) | two control words
// and its waves take the chunk's restarts one by one from a counter in LDS: ONE WAVEFRONT PER (problem, restart).  After the barrier
// that follows the staging a wave never waits for another one: no flags, no spinning; the next barrier is the one before the image
// is replaced.  The restarts read column i of A_b as ROW i of the image, so a matrix that is not symmetric (or holds a NaN) sets
// ticket[1] and the call fails.  sdr_small_kernel, the spectral kernels and the ADMM setup kernels have a loop of their own (one wave
// per problem) and share the host helpers only: the launchers below (workgroups, launch), one pair for them and one for the ticket
// kernels.  What needs no device code -- the call frame of the drivers, ticket_partition, the workgroup-size rule, the kernel names
// -- is in batch_call.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>

#include "batch_call.h"      // batch_wide_threads, batch_kernel_name

namespace qcqpmi {

// bytes of the LDS image; pc_entries: 0, or the m list entries whose (p, q, r) the per-problem-constraint kernels stage
inline size_t small_image_bytes(int64_t n, int64_t pc_entries) { return (size_t)(n * n + n + 3 * pc_entries) * sizeof(double) + 2 * sizeof(int); }

// workgroups of a persistent launch: what the device holds at once (`per` workgroups on each CU: the occupancy query's answer, taken
// as at least one), at most one per ticket; or < 0: -hipError_t
inline int small_workgroup_cap(int device, int per, int64_t tickets) {
    int cus = 0;
    const hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return -(int)e;
    const int64_t cap = (int64_t)cus * (per < 1 ? 1 : per);
    return (int)(tickets < cap ? tickets : cap);
}

// the winners' points: out[b][0..n) = X[b][idx[2 b]][0..n)  (idx as select_best_kernel leaves it; < 0: row left as it is); cd_small.hip
int small_gather_launch(const double *X, int64_t n, int64_t R, int64_t B, const int64_t *idx, double *out, hipStream_t st);

// ---- the launchers of the persistent batch kernels: a unit keeps its LDS formula and its "which kernel for this n" and calls these
// with the kernel's address.  Workgroups: what the device holds at once, at most one per ticket, or < 0: -hipError_t.

// a ONE-WAVE-PER-PROBLEM kernel (sdr_small, spectral_small / _wide, admm_setup / _wide): 64 threads, dynamic LDS past 64 KB allowed
inline int small_wave_workgroups(const void *fn, size_t lds, int64_t B, int device) {
    int per = 0;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, fn, 64, lds);
    return e != hipSuccess ? -(int)e : small_workgroup_cap(device, per, B);
}

// a TICKET kernel (cd_small, admm_small) and *threads, the size of its workgroups: 256 -- or, for a wide kernel (large > 0: its
// largest workgroup; the image passes 64 KB from n = 91), what batch_wide_threads picks from two occupancy queries, or `asked`
inline int small_ticket_workgroups(const void *fn, size_t lds, int64_t tickets, int device, int large, int asked, int *threads) {
    int per = 0, per_large = 0;
    hipError_t e = large ? hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
    *threads = large && asked ? asked : 256;
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, fn, *threads, lds);
    if (e == hipSuccess && large && !asked) {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_large, fn, large, lds);
        if (e == hipSuccess && batch_wide_threads(per, per_large, large) == large) { per = per_large; *threads = large; }
    }
    return e != hipSuccess ? -(int)e : small_workgroup_cap(device, per, tickets);
}

// QCQPMI_CD_WIDE_THREADS / QCQPMI_ADMM_WIDE_THREADS = 64 .. large (a multiple of 64): that workgroup size for the wide kernels instead
// of the rule, for measuring the rule (tools/bench_small_batch.py, bench_admm_batch.py --wide-threads); results do not depend on it.
// 0: not set, or not such a number.  The units read theirs once.
inline int small_threads_asked(const char *variable, int large) {
    const char *v = getenv(variable);
    const int t = v ? atoi(v) : 0;
    return (t >= 64 && t <= large && t % 64 == 0) ? t : 0;
}

// the launch (a template: instantiated in the unit that owns the kernel); big_lds: more than 64 KB of dynamic LDS may be needed
template <class Args>
inline int small_launch(void (*fn)(Args), size_t lds, const Args &a, int wgs, int threads, bool big_lds, hipStream_t st) {
    const hipError_t e = big_lds ? hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(fn, dim3((unsigned)wgs), dim3((unsigned)threads), lds, st, a);
    return (int)hipGetLastError();
}

// ---- staging, by the nt threads of the workgroup (nn = n n entries; off: problem b's offset b n in q0s)
__device__ __attribute__((always_inline)) inline void small_stage_matrix(double *As, const double *Ag, int nn, int tid, int nt) {
    for (int e = tid; e < nn; e += nt) As[e] = Ag[e];
}

__device__ __attribute__((always_inline)) inline void small_stage_q(double *qs, const double *q0s, int64_t off, int n, int tid) {
    if (tid < n) qs[tid] = q0s[off + tid];
}

// entry e of the context's lists (cptr order) is constraint cidx[e] of cg [m][3] = (p, q, r) in CONSTRAINT order
__device__ __attribute__((always_inline)) inline void small_stage_cons(double *cs, const double *cg, const int *cidx, int m, int tid, int nt) {
    for (int e = tid; e < m; e += nt) {
        const double *ck = cg + (cidx[e] - 1) * 3;
        cs[e] = ck[0]; cs[m + e] = ck[1]; cs[2 * m + e] = ck[2];
    }
}

// does the staged image As -- or G, a second n x n matrix the restarts read from global memory (nullptr, the constant: none) -- differ
// from its transpose somewhere (a NaN differs from itself)?  This thread's share of the entries.
template <class Second>
__device__ __attribute__((always_inline)) inline bool small_asym_scan(const double *As, Second G, int n, int nn, int tid, int nt) {
    bool asym = false;
    for (int e = tid; e < nn; e += nt) {
        const int i = e / n, j = e - i * n;
        if constexpr (std::is_null_pointer_v<Second>) asym = asym || (j > i && !(As[e] == As[j * n + i]));
        else asym = asym || (j > i && (!(As[e] == As[j * n + i]) || !(G[e] == G[j * n + i])));
    }
    return asym;
}

// The frame.  a: the kernel's argument struct (P, B, R, RC, chunks, q0s, cons, ticket); lds: small_image_bytes of dynamic LDS; nt: threads.
//   stage(off, As, nn, tid, nt)    copies problem b's matrix into the image (off = b n n) and returns the G of small_asym_scan;
//   restart(As, qs, b, r, lane)    one restart, by one wave.
// Both are lambdas marked __attribute__((always_inline)): the kernel stays ONE function.  The frame hands down n n and the offsets
// so that the kernels keep the register counts of the frame written out (profiles/r15_small_batch_refactor.md).
// PC: problem b's (p, q, r) of every list entry are staged too and the restarts read them through a.P, the kernel's copy of the
// context's DevProblem, whose cp / cq / cr point at that image; cptr and crel stay the context's.
template <bool PC, class Args, class Stage, class Restart>
__device__ __attribute__((always_inline)) inline void small_ticket_frame(Args &a, double *lds, int nt, Stage stage, Restart restart) {
    const int n = (int)a.P.n, nn = n * n, m = PC ? (int)a.P.m : 0;
    double *As = lds, *qs = lds + nn;
    double *cs = qs + n;             // PC: [3][m] the staged coefficients, p then q then r
    int *ctl = (int *)(cs + 3 * m);  // [0] the workgroup's ticket, [1] next restart of its chunk
    const int *cidx = a.P.cidx;
    if constexpr (PC) { a.P.cp = cs; a.P.cq = cs + m; a.P.cr = cs + 2 * m; }      // the view
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t tickets = a.B * a.chunks;
    for (;;) {
        __syncthreads();             // every wave is done with the LDS image of the previous ticket
        if (tid == 0) {
            ctl[0] = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ctl[1] = 0;
        }
        __syncthreads();
        const int64_t tk = ctl[0];
        if (tk >= tickets) break;
        const int64_t b = tk / a.chunks, r_lo = (tk % a.chunks) * a.RC;
        const int64_t r_hi = r_lo + a.RC < a.R ? r_lo + a.RC : a.R;
        const int64_t bn = b * n;    // problem b's offset in q0s; bn n: in the [B][n][n] arrays
        const auto G = stage(bn * n, As, nn, tid, nt);
        small_stage_q(qs, a.q0s, bn, n, tid);
        if constexpr (PC) small_stage_cons(cs, a.cons + b * m * 3, cidx, m, tid, nt);
        __syncthreads();
        if (small_asym_scan(As, G, n, nn, tid, nt)) a.ticket[1] = 1;
        for (;;) {
            int k = 0;
            if (lane == 0) k = atomicAdd(&ctl[1], 1);
            k = __builtin_amdgcn_readfirstlane(k);
            if (r_lo + k >= r_hi) break;
            restart(As, qs, b, r_lo + k, lane);
        }
    }
}

// The chain frame (chain_small.hip): the ticket of small_ticket_frame, worked through a.nstages STAGES one after the other.  Every stage
// has an image of its own in the same LDS (its matrix, q0_b; the [3][m] coefficients are staged once per ticket) and runs every restart
// of the chunk once; restart o of stage s > 0 starts from the point restart o of stage s - 1 wrote to global memory, perhaps by another
// wave of this workgroup.  Per stage: barrier -- staging -- barrier -- scan -- the waves take the restarts from the LDS counter.  The
// barrier that opens stage s > 0 is the hand-over: every wave has waited for its own stores of stage s - 1 (s_waitcnt vmcnt(0)) before
// it arrives, and the loads of stage s are issued after it, by waves of the same workgroup through the same vector L1.
// No flags, no spinning: a wave waits for nothing but these barriers; a workgroup moves on to the next stage of ITS ticket whatever the
// other workgroups are doing.
//   stage(s, off, As, nn, tid, nt)            copies stage s's matrix of problem b into the image; returns the second matrix the restarts
//                                             read from global memory (a const double *, nullptr: none), which the scan covers too;
//   restart(s, As, qs, cs, b, r, lane)        one restart of stage s, by one wave; cs: the staged coefficients (PC), p then q then r.
// `a` is not written (the PC view of the lists is built by the caller from cs): its stage table stays in the kernel-argument segment.
template <bool PC, class Args, class Stage, class Restart>
__device__ __attribute__((always_inline)) inline void small_chain_frame(const Args &a, double *lds, int nt, Stage stage, Restart restart) {
    const int n = (int)a.P.n, nn = n * n, m = PC ? (int)a.P.m : 0;
    double *As = lds, *qs = lds + nn;
    double *cs = qs + n;             // PC: [3][m] the staged coefficients, p then q then r
    int *ctl = (int *)(cs + 3 * m);  // [0] the workgroup's ticket, [1] next restart of its chunk in the running stage
    const int *cidx = a.P.cidx;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t tickets = a.B * a.chunks;
    for (;;) {
        __syncthreads();             // every wave is done with the LDS image of the previous ticket
        if (tid == 0) ctl[0] = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const int64_t tk = ctl[0];
        if (tk >= tickets) break;
        const int64_t b = tk / a.chunks, r_lo = (tk % a.chunks) * a.RC;
        const int64_t r_hi = r_lo + a.RC < a.R ? r_lo + a.RC : a.R;
        const int64_t bn = b * n;    // problem b's offset in q0s; bn n: in the [B][n][n] arrays
        for (int s = 0; s < a.nstages; s++) {
            if (s > 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's points of stage s - 1 have left it
                __syncthreads();     // the hand-over; every wave is done with the image of stage s - 1
            }
            if (tid == 0) ctl[1] = 0;
            const double *G = stage(s, bn * n, As, nn, tid, nt);
            small_stage_q(qs, a.q0s, bn, n, tid);
            if constexpr (PC) { if (s == 0) small_stage_cons(cs, a.cons + b * m * 3, cidx, m, tid, nt); }
            __syncthreads();
            bool asym = small_asym_scan(As, nullptr, n, nn, tid, nt);
            if (G) asym = asym || small_asym_scan(G, nullptr, n, nn, tid, nt);
            if (asym) a.ticket[1] = 1;
            for (;;) {
                int k = 0;
                if (lane == 0) k = atomicAdd(&ctl[1], 1);
                k = __builtin_amdgcn_readfirstlane(k);
                if (r_lo + k >= r_hi) break;
                restart(s, As, qs, cs, b, r_lo + k, lane);
            }
        }
    }
}

}  // namespace qcqpmi
