// Building blocks of the role-split phase-2 kernels (cd_phase2_q.h, cd_queue.hip, cd_life.hip): the constants of the
// layout, the quad DPP helpers of the chain wave, the ownership of the contraction's blocks, the A-fragment / B-operand
// loads and the product of a multiplying wave, and the synchronisation words in LDS.  What the roles do and why:
// cd_phase2_q.h and DESIGN.md section 4.1.
#pragma once
#include <stdint.h>
#include "dev_util.h"
#include "mfma_block.h"
#include "cd_life_plan.h"      // RQ_NSIMD, RQ_MAXU, RQ_CSMAX: the constants the launch rules read too

namespace qcqpmi {

constexpr int RQ_NMW = 6;     // mfma waves: two per SIMD on three SIMDs, taking turns
constexpr int RQ_PFU = 5;     // A-fragment ring of an mfma wave: units (blocks of 16 coordinates) resident at a time
constexpr int RQ_RND = 4;     // passes over the ring per product
constexpr int RQ_PERS = 20;   // units whose B operands stay in registers; any others are re-read for every product

// LDS doubles besides the X tile
constexpr int RQ_LDS_COMMON = 2 * RQ_NSIMD * 256 + 256 + 2 * 256 + 2 * 16 + 2 * 16 + 2 * 16 + 16 + 4 * 16 + 8 + 8 + 8;

// the product loop's look-ahead loads reach unit RQ_MAXU - 1 of the X tile (at the start of the allocation) whatever n is
constexpr size_t RQ_LDS_MIN = (size_t)((RQ_NSIMD - 1) * 256 + (12 * (RQ_MAXU - 1) + 3) * 64 + 64) * 8;

template <int CTRL>
__device__ __attribute__((always_inline)) inline double rq_quad_bcast(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

__device__ __attribute__((always_inline)) inline double rq_quad_sum(double v) {
    const double a = __hiloint2double(__builtin_amdgcn_mov_dpp(__double2hiint(v), 0xB1, 0xf, 0xf, true),
                                      __builtin_amdgcn_mov_dpp(__double2loint(v), 0xB1, 0xf, 0xf, true));   // quad_perm [1,0,3,2]
    const double s = v + a;
    const double b = __hiloint2double(__builtin_amdgcn_mov_dpp(__double2hiint(s), 0x4E, 0xf, 0xf, true),
                                      __builtin_amdgcn_mov_dpp(__double2loint(s), 0x4E, 0xf, 0xf, true));   // quad_perm [2,3,0,1]
    return s + b;
}

__device__ __attribute__((always_inline)) inline unsigned rq_quad_or(unsigned v) {
    v |= (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, true);
    v |= (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, true);
    return v;
}

// Ownership of the contraction: the chain wave multiplies the last CS blocks of 16 coordinates itself, the others are
// dealt cyclically to the three multiplying SIMDs: block j < NB - CS belongs to SIMD j % 3, unit j / 3.
struct RqOwn {
    int first;    // first owned block
    int stride;   // distance between owned blocks
    int nu;       // number of owned blocks
    int NB;
};

__device__ __attribute__((always_inline)) inline RqOwn rq_own(int NB, int CS, int mw) {
    RqOwn o;
    const int cs = CS < NB ? CS : 0;
    const int rest = NB - cs;
    o.NB = NB;
    if (mw >= RQ_NSIMD) { o.first = rest; o.stride = 1; o.nu = cs; }
    else { o.first = mw; o.stride = RQ_NSIMD; o.nu = mw < rest ? (rest - mw + RQ_NSIMD - 1) / RQ_NSIMD : 0; }
    return o;
}

// block held by register slot U (clamped to a valid block: slots past the owned ones are loaded, never multiplied)
__device__ __attribute__((always_inline)) inline int rq_block(const RqOwn &o, int U) {
    const int bb = o.first + U * o.stride;
    return bb < o.NB ? bb : o.NB - 1;
}

// slot of block j, or -1 if the wave does not own it
__device__ __attribute__((always_inline)) inline int rq_slot(const RqOwn &o, int j) {
    const int d = j - o.first;
    if (d < 0 || d % o.stride != 0) return -1;
    const int U = d / o.stride;
    return U < o.nu ? U : -1;
}

// the pair-packed copy of P0 as 16-byte pairs, in the address space the caller holds it in (generic or global)
__device__ __attribute__((always_inline)) inline const v2d_ *rq_pairs(const double *p) { return reinterpret_cast<const v2d_ *>(p); }
__device__ __attribute__((always_inline)) inline GLB const v2d_ *rq_pairs(GLB const double *p) { return (GLB const v2d_ *)p; }

// A fragments (pair-packed copy: k-steps 2 kk2, 2 kk2 + 1 of block row bn at ((bn KS/2 + kk2) 64 + lane) 2) of the
// owned blocks for the product of block row bn -> registers
template <int NU, class APtr>
__device__ __attribute__((always_inline)) inline void rq_load_A(v2d_ (&ar)[2 * NU], APtr __restrict__ Apack2, int KS, const RqOwn &o, int lane, int bn) {
#pragma unroll
    for (int U = 0; U < NU; U++) {
        const auto ap = rq_pairs(Apack2) + ((int64_t)bn * (KS / 2) + 2 * rq_block(o, U)) * 64;
        ar[2 * U] = ap[(unsigned)lane];
        ar[2 * U + 1] = ap[64u + (unsigned)lane];
    }
}

// product of block row bn over the owned blocks except slots `hs`, `hs2` (the block the chain is rewriting and the one it
// rewrote just before: the chain supplies both itself; -1 = none); every
// fragment register is refilled right after the MFMAs that consumed it with the fragment of block row bn2
template <int NU, class APtr>
__device__ __attribute__((always_inline)) inline v4d_ rq_product(v2d_ (&ar)[2 * NU], const double (&bq)[4 * NU], APtr __restrict__ Apack2, int KS,
                                  const RqOwn &o, int lane, int hs, int hs2, int bn2, v4d_ acc0) {
    v4d_ acc = acc0, acc1 = {0.0, 0.0, 0.0, 0.0}, acc2 = acc1, acc3 = acc1;
#pragma unroll
    for (int U = 0; U < NU; U++) {
        if (U < o.nu && U != hs && U != hs2) {   // wave-uniform
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[2 * U][0], bq[4 * U], acc, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[2 * U][1], bq[4 * U + 1], acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[2 * U + 1][0], bq[4 * U + 2], acc2, 0, 0, 0);
            acc3 = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[2 * U + 1][1], bq[4 * U + 3], acc3, 0, 0, 0);
        }
        {   // unconditional refill: s_waitcnt can count the loads
            const auto ap = rq_pairs(Apack2) + ((int64_t)bn2 * (KS / 2) + 2 * rq_block(o, U)) * 64;
            ar[2 * U] = ap[(unsigned)lane];
            ar[2 * U + 1] = ap[64u + (unsigned)lane];
        }
    }
    return (acc + acc1) + (acc2 + acc3);
}

// B operands of the owned blocks from the X tile in LDS (MFMA B layout: lane l <- X[4 kk + (l >> 4)][l & 15])
template <int NU>
__device__ __attribute__((always_inline)) inline void rq_load_B(double (&bq)[4 * NU], const double *Xs, const RqOwn &o, int lane) {
    const int xoff = (lane >> 4) * 16 + (lane & 15);
#pragma unroll
    for (int U = 0; U < NU; U++) {
        const int bb = rq_block(o, U);
#pragma unroll
        for (int q = 0; q < 4; q++) bq[4 * U + q] = Xs[(4 * bb + q) * 64 + xoff];
    }
}

// the block in slot `us` has been rewritten by the chain: refresh those 4 operands
template <int NU>
__device__ __attribute__((always_inline)) inline void rq_refresh_B(double (&bq)[4 * NU], const double *Xs, const RqOwn &o, int lane, int us) {
    const int xoff = (lane >> 4) * 16 + (lane & 15);
    const int bb = rq_block(o, us < 0 ? 0 : us);
    const double n0 = Xs[(4 * bb + 0) * 64 + xoff], n1 = Xs[(4 * bb + 1) * 64 + xoff];
    const double n2 = Xs[(4 * bb + 2) * 64 + xoff], n3 = Xs[(4 * bb + 3) * 64 + xoff];
#pragma unroll
    for (int U = 0; U < NU; U++) {
        const bool hit = (U == us);      // wave-uniform
        bq[4 * U + 0] = hit ? n0 : bq[4 * U + 0];
        bq[4 * U + 1] = hit ? n1 : bq[4 * U + 1];
        bq[4 * U + 2] = hit ? n2 : bq[4 * U + 2];
        bq[4 * U + 3] = hit ? n3 : bq[4 * U + 3];
    }
}

// ---- synchronisation words in LDS (no s_barrier inside the block loop: waves only wait for what they consume)
//   [0] cons    = g + 1 once the chain has read the partial tiles of interval g
//   [1] commit  = g + 1 once the chain has committed the block of interval g to the X tile (and is done with its staged operands)
//   [2] stop    != 0: leave the loop
//   [4 + w]     iterations published by producer w: the six mfma waves (partial tiles), w = 6: the staging wave (small
//               operands of the block); one word PER WAVE: a shared counter would let a wave that runs ahead stand in for
//               one that lags
// LDS operations of one wave complete in program order, so "data, then flag" needs no wait on the producer side and
// "flag, then data" none on the consumer side.
enum { RQ_CONS = 0, RQ_COMMIT = 1, RQ_STOP = 2, RQ_PARTS = 4 };

typedef int rq_i4 __attribute__((ext_vector_type(4)));
// explicit LDS address space: a volatile access through a generic pointer becomes a FLAT instruction (vmcnt + lgkmcnt,
// not ordered with the wave's DS queue) -- the protocol needs plain ds_read / ds_write
typedef __attribute__((address_space(3))) int rq_lds_int;
typedef __attribute__((address_space(3))) rq_i4 rq_lds_i4;

__device__ __attribute__((always_inline)) inline rq_i4 rq_sync_read(rq_lds_int *sy) {
    rq_i4 v = *(volatile rq_lds_i4 *)sy;                     // one ds_read_b128
    asm volatile("" ::: "memory");                           // nothing that follows may be read before the flags
    v[0] = __builtin_amdgcn_readfirstlane(v[0]); v[1] = __builtin_amdgcn_readfirstlane(v[1]);
    v[2] = __builtin_amdgcn_readfirstlane(v[2]); v[3] = __builtin_amdgcn_readfirstlane(v[3]);
    return v;
}

__device__ __attribute__((always_inline)) inline void rq_sync_write(rq_lds_int *sy, int which, int value, int lane) {
    asm volatile("" ::: "memory");                           // data first, then the flag (DS queue is in order per wave)
    if (lane == 0) *(volatile rq_lds_int *)(sy + which) = value;
    asm volatile("" ::: "memory");
}

}  // namespace qcqpmi
