// Wide spectral batch kernel (65 <= n <= 128): interface between its driver (capi_small.hip) and spectral_wide_kernel, which is built
// in the unit of the narrow kernel (spectral_small.hip: the two share the argument struct, the scalar pieces of spectral_solve.h and
// the ticket draw).  Host declarations only.
//
// The problem, its outputs and its status codes are those of spectral_small.h.  What differs is the eigen-solver and the lanes:
//   * A_b and Q_b do not both fit the LDS of a compute unit past n = 64 (2 n2^2 doubles: 264 KB at n = 128 against 160 KB).  The
//     kernel runs jacobi_wide (jacobi_wide.h): one-sided Jacobi on G = A_b + 2 |A_b|_F I, ONE n2 x (n2 + 1) array, which ends as Q_b
//     (column k = eigenvector k).  The eigenvalues are Rayleigh quotients against A_b re-read from global memory.
//   * a lane holds TWO indices, l and l + 64 (coordinates, eigen-indices, columns).  A wave sum over the indices adds the lane's two
//     slots first and then runs wave_sum_tree; maxima likewise.
// ONE WAVEFRONT PER PROBLEM, one wavefront per workgroup, problems drawn from a global counter.  Per problem, n2 = n rounded up to even,
// str = n2 + 1, G[k str + i] = entry (i, k):
//   stage     s_i, h_i; G = A_b = P0_b / (s_i s_j) with zero padding, entry (i, j) by the lane of j; P0_b[i][j] is compared with
//             P0_b[j][i] (the diagonal with itself: a NaN) and ticket[1] is set on a mismatch.  (P0 h)_i = sum_j P0_b[j][i] h_j by fma
//             in ascending j from 0.0; g_i; rho^2 = wave_sum_tree(slot 0 + slot 1 of beta_i^2 / (4 a_i)) - gamma.
//   Jacobi    jacobi_wide: G becomes Q.
//   spectrum  row i of A_b is formed again from global memory by the lanes of j (the same division, the same bits), left in LDS and
//             read by every lane (one operand for all lanes); lane = eigen-index k:  t = sum_j A_ij u_jk by fma in ascending j from
//             0.0, lam_k = sum_i u_ik t by fma in ascending i from 0.0.  gh_k = sum_i u_ik g_i by fma in ascending i from 0.0.
//             lam_min, max |lam|, d_k, rank_k and k_min as in spectral_small.h.
//   branch    as in spectral_small.h, through the same secular_w, spectral_hard_case and secular_root.
//   point     lane = i: y_i = sum_k u_ik w_k by fma in ascending k from 0.0 (+ tau q_min,i; q_min = column k_min with its entry of
//             largest magnitude positive, lowest index on ties); x_i; bound = f0(x) from P0_b as in spectral_small.h.
// status: 0; 1 if Jacobi stopped at max_sweeps; 2 if the bound, mu or a coordinate of x is not finite.  sweeps counts the last sweep,
// in which nothing was rotated, too (0 where |A_b|_F == 0).
// A problem's result depends on (P0_b, q0_b, r0_b, agg_b, relop, max_sweeps, tol) alone, bit for bit, as in spectral_small.h.
// LDS per wave: (n2 (n2 + 1) + 5 * 128) doubles: 137 216 bytes at n = 128 (one wave per CU of 160 KiB), 40 496 at n = 65 (four).
#pragma once
#include "spectral_small.h"

namespace qcqpmi {

constexpr int SPECTRAL_WIDE_MAXN = 128;      // two indices per lane

size_t spectral_wide_lds_bytes(int n);
// workgroups of the launch (persistent: at most what the device holds at once), or < 0: -hipError_t
int spectral_wide_workgroups(int n, int64_t B, int device);
int spectral_wide_launch(const SpectralSmallArgs &a, int wgs, hipStream_t st);

}  // namespace qcqpmi
