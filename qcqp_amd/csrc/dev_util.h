// Small device helpers shared by the kernel files: pointers typed as global memory with their relaxed agent-scope
// accesses, the order-preserving map between doubles and unsigned integers, the wave-wide maximum and sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qcqpmi {

// pointers typed as global memory: a generic pointer makes the compiler emit FLAT loads / stores / atomics, which count against
// the LDS counter as well -- and the roles of the pipelined kernels synchronise through LDS words (measured in round 3: 30 % slower)
#define GLB __attribute__((address_space(1)))
template <class T>
__device__ __attribute__((always_inline)) inline GLB T *glb(T *p) { return (GLB T *)p; }
__device__ __attribute__((always_inline)) inline int glb_load_int(GLB const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __attribute__((always_inline)) inline double glb_load_d(GLB const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __attribute__((always_inline)) inline int glb_add(GLB int *p, int v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// order-preserving map double -> u64 and back (reductions over the threads of a workgroup as integer LDS atomics: two
// instructions per wave instead of a DPP tree per wave plus a second level through LDS)
__device__ __attribute__((always_inline)) inline unsigned long long ordered_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __attribute__((always_inline)) inline double ordered_unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// maximum over the 64 lanes of a wave (butterfly: every lane ends with it)
__device__ __attribute__((always_inline)) inline double wave_max(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const double w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    return v;
}

// one value per lane from the lane a DPP control names (quad_perm / row_mirror / row_half_mirror: every lane has a partner)
template <int CTRL>
__device__ __attribute__((always_inline)) inline double dpp_partner(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// sum over the 64 lanes of a wave in ONE fixed order: the binary tree over adjacent lanes -- pairs, quads, eights (a lane and its
// mirror image in the group of eight hold the two quads' sums), sixteens (mirror image in the row), then lane ^ 16 and lane ^ 32.
// The two partners of a step add the same two numbers, so every lane ends with the same bits.
__device__ __attribute__((always_inline)) inline double wave_sum_tree(double v) {
    v += dpp_partner<0xB1>(v);       // quad_perm [1, 0, 3, 2]
    v += dpp_partner<0x4E>(v);       // quad_perm [2, 3, 0, 1]
    v += dpp_partner<0x141>(v);      // row_half_mirror
    v += dpp_partner<0x140>(v);      // row_mirror
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

}  // namespace qcqpmi
