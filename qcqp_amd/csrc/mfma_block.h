// The fp64 matrix-core building blocks every kernel of the coordinate-descent family shares: the vector types of the
// v_mfma_f64_16x16x4_f64 operands and the two loops that stream A fragments (Apack layout, kernels.h) against rows of a
// tile of 16 candidates.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qcqpmi {

typedef double v4d_ __attribute__((ext_vector_type(4)));
typedef double v2d_ __attribute__((ext_vector_type(2)));

// acc(16 rows of block b) x (16 candidates) += Apack[b][kk0..kk1) * Xt rows.  XT may point to LDS
// or global memory; rows are 16 doubles.
template <typename XPtr>
__device__ inline v4d_ block_rows_times_X(const double *__restrict__ Ab, XPtr Xs, int kk0, int kk1,
                                          int lane, v4d_ acc) {
    const int xoff = (lane >> 4) * 16 + (lane & 15);
    int kk = kk0;
    for (; kk + 8 <= kk1; kk += 8) {
        double a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            a[u] = Ab[(int64_t)(kk + u) * 64 + lane];
            b[u] = Xs[(kk + u) * 64 + xoff];
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
    for (; kk < kk1; kk++) {
        double a = Ab[(int64_t)kk * 64 + lane];
        double b = Xs[kk * 64 + xoff];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    return acc;
}

// acc += Apack[b][kk] * X rows for kk in [kk0, kk1) streaming the A fragments from L2
// (fallback for k-steps that do not fit the register prefetch, n > 16 * 3 * PFU).
template <typename XPtr>
__device__ inline v4d_ mfma_range(const double *__restrict__ Ab, XPtr Xs, int kk0, int kk1, int lane,
                                  v4d_ acc) {
    const double *ap = Ab + (int64_t)kk0 * 64 + lane;
    XPtr xp = Xs + kk0 * 64 + (lane >> 4) * 16 + (lane & 15);
    for (int k = kk0; k < kk1; k++) {
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[0], xp[0], acc, 0, 0, 0);
        ap += 64;
        xp += 64;
    }
    return acc;
}

}  // namespace qcqpmi
