// Symmetric eigen-solver for ONE matrix of up to 128 rows by ONE wavefront with ONE n2 x n2 array in LDS: shifted one-sided
// (Hestenes) Jacobi with the round-robin ordering of jacobi_small.h.  jacobi_small.h keeps the matrix and the eigenvectors (2 n2^2
// doubles, 264 KB at n2 = 128); this solver rotates the COLUMNS of G = A + c I until they are orthogonal and needs G alone (132 KB).
// A device function for the batch kernels (spectral_wide_kernel runs it; a device-side setup of batched ADMM at n = 128 could).  It
// takes the rotation and the ordering from spectral_solve.h -- two scalar functions that a host program can test -- and nothing else
// of the spectral suggest.
//
// Why the shift.  For symmetric positive definite G = U diag(mu) U', rotating columns from the right until they are orthogonal ends
// at G J = U diag(mu): the columns, normalised, are the eigenvectors.  c = 2 |A|_F puts every eigenvalue of G into [c / 2, 3 c / 2]
// (|lam_k(A)| <= |A|_F): G is never singular and its condition number is at most 3, so the number of sweeps does not depend on the
// spectrum of A.  |A|_F == 0 (fro2 == 0.0) is a case of its own: Q = I, no sweep (G would be 0 and the normalisation 0 / 0).
// Magnitude: the squares of the entries must neither all underflow nor overflow.  A matrix with a nonzero entry whose fro2 comes out
// as 0.0 takes that exit too, and one whose fro2 is not finite gets c = inf: `degenerate` reports both, and the callers turn it
// into status 2 (what comes back in G is NOT a set of eigenvectors).
// The eigenvalues are NOT read off the column norms (|g_k| - c carries the rounding of c, measured 1e-13 of max |lam| at n = 128 in
// the NumPy restatement): the caller forms Rayleigh quotients u_k' A u_k from its own copy of A.
//
// Layout.  G column-major: column k is the `str` doubles from G + k str, str >= n2.  n2 EVEN (an odd matrix is padded by its caller
// with a decoupled coordinate: a zero row and column; G[n2 - 1][n2 - 1] = c then, its dot product with every other column is exactly
// 0, it never rotates and stays at its index).  An odd stride (n2 + 1) spreads the columns of a round over the banks: lane = slot
// walks down its two columns, so a half-wave reads 32 different columns at one row; bank pair = (column + row) mod 32 for
// str = 1 mod 32.  The columns of a round-robin round are NOT consecutive, so two lanes of a half-wave can meet on a bank pair; how
// often has not been measured.
//
// In:  G = A (symmetric, padding in place).  fro2 = sum_ij a_ij^2: lane = column k and k + 64, each in ascending row by a*a added
//      to 0.0, the lane's two sums added, then wave_sum_tree.  c = 2 sqrt(fro2) is added to the diagonal.
// A sweep is n2 - 1 rounds; a round has n2 / 2 disjoint pairs (p, q) = round_robin_pair(n2, round, slot), p < q, lane = slot:
//      alpha = g_p . g_p, beta = g_q . g_q, gamma = g_p . g_q, each by fma in ascending row from 0.0;
//      hestenes_rotation(alpha, beta, gamma, tol): where it rotates, (g_p, g_q) <- (c g_p - s g_q, s g_p + c g_q) row by row.
//      Nothing crosses lanes inside a round; between rounds stands the barrier of a one-wave workgroup.
// The solver stops after the first sweep in which no pair was rotated (converged) or after max_sweeps sweeps.
// Out: column k of G = u_k = g_k / |g_k| (|g_k|^2 by fma in ascending row from 0.0), in NO particular order of the eigenvalues.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_util.h"
#include "spectral_solve.h"

namespace qcqpmi {

constexpr int JACOBI_WIDE_MAXN = 128;
constexpr int JACOBI_WIDE_BLOCK = 8;         // rows whose LDS reads are in flight together in a lane's pass over its two columns

// the odd column stride for an n2 x n2 matrix, and the doubles of LDS that the solver needs with it
__host__ __device__ inline int jacobi_wide_stride(int n2) { return n2 | 1; }
__host__ __device__ inline size_t jacobi_wide_doubles(int n2) { return (size_t)n2 * jacobi_wide_stride(n2); }

struct JacobiWideResult { int sweeps; bool converged; bool degenerate; double fro2; };

// Called by all 64 lanes of a one-wave workgroup; the caller's writes to G are ordered by the barrier at the top.
__device__ inline JacobiWideResult jacobi_wide(double *G, int n2, int str, int lane, int max_sweeps, double tol) {
    const int half = n2 / 2;
    JacobiWideResult res;
    res.sweeps = 0;
    res.converged = false;
    __syncthreads();
    double f[2] = {0.0, 0.0};
    bool nz = false;
    for (int h = 0; h < 2; h++) {
        const int k = lane + 64 * h;
        if (k < n2) for (int i = 0; i < n2; i++) { const double a = G[k * str + i]; f[h] += a * a; nz = nz || a != 0.0; }
    }
    res.fro2 = wave_sum_tree(f[0] + f[1]);
    res.degenerate = !(res.fro2 < __builtin_huge_val()) || (res.fro2 == 0.0 && __ballot(nz) != 0);
    if (res.fro2 == 0.0) {
        for (int h = 0; h < 2; h++) {
            const int k = lane + 64 * h;
            if (k < n2) G[k * str + k] = 1.0;
        }
        res.converged = true;
        __syncthreads();
        return res;
    }
    const double c = 2.0 * sqrt(res.fro2);
    for (int h = 0; h < 2; h++) {
        const int k = lane + 64 * h;
        if (k < n2) G[k * str + k] += c;
    }
    __syncthreads();
    while (res.sweeps < max_sweeps) {
        bool rotated = false;
        for (int round = 0; round < n2 - 1; round++) {
            if (lane < half) {
                int p, q;
                round_robin_pair(n2, round, lane, &p, &q);
                double *gp = G + p * str, *gq = G + q * str;
                // Both passes take JACOBI_WIDE_BLOCK rows at a time: the reads of a block are issued together and waited for once
                // (written row by row, every row waited for its own two reads, and with one wave per CU nothing else hides that
                // latency).  The arithmetic keeps its order: ascending row.
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                int i = 0;
                for (; i + JACOBI_WIDE_BLOCK <= n2; i += JACOBI_WIDE_BLOCK) {
                    double a[JACOBI_WIDE_BLOCK], b[JACOBI_WIDE_BLOCK];
#pragma unroll
                    for (int u = 0; u < JACOBI_WIDE_BLOCK; u++) { a[u] = gp[i + u]; b[u] = gq[i + u]; }
#pragma unroll
                    for (int u = 0; u < JACOBI_WIDE_BLOCK; u++) {
                        alpha = __builtin_fma(a[u], a[u], alpha);
                        beta = __builtin_fma(b[u], b[u], beta);
                        gamma = __builtin_fma(a[u], b[u], gamma);
                    }
                }
                for (; i < n2; i++) {
                    const double a = gp[i], b = gq[i];
                    alpha = __builtin_fma(a, a, alpha);
                    beta = __builtin_fma(b, b, beta);
                    gamma = __builtin_fma(a, b, gamma);
                }
                const JacobiRot r = hestenes_rotation(alpha, beta, gamma, tol);
                if (r.s != 0.0) {
                    rotated = true;
                    for (i = 0; i + JACOBI_WIDE_BLOCK <= n2; i += JACOBI_WIDE_BLOCK) {
                        double a[JACOBI_WIDE_BLOCK], b[JACOBI_WIDE_BLOCK];
#pragma unroll
                        for (int u = 0; u < JACOBI_WIDE_BLOCK; u++) { a[u] = gp[i + u]; b[u] = gq[i + u]; }
#pragma unroll
                        for (int u = 0; u < JACOBI_WIDE_BLOCK; u++) {
                            gp[i + u] = r.c * a[u] - r.s * b[u];
                            gq[i + u] = r.s * a[u] + r.c * b[u];
                        }
                    }
                    for (; i < n2; i++) {
                        const double a = gp[i], b = gq[i];
                        gp[i] = r.c * a - r.s * b;
                        gq[i] = r.s * a + r.c * b;
                    }
                }
            }
            __syncthreads();
        }
        res.sweeps++;
        if (__ballot(rotated) == 0) { res.converged = true; break; }
    }
    for (int h = 0; h < 2; h++) {
        const int k = lane + 64 * h;
        if (k < n2) {
            double nn = 0.0;
            for (int i = 0; i < n2; i++) { const double a = G[k * str + i]; nn = __builtin_fma(a, a, nn); }
            const double nrm = sqrt(nn);
            for (int i = 0; i < n2; i++) G[k * str + i] /= nrm;
        }
    }
    __syncthreads();
    return res;
}

}  // namespace qcqpmi
