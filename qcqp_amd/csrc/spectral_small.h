// Small-problem spectral batch kernel: interface between its driver (capi_small.hip) and spectral_small.hip (own translation unit).
// Host declarations only: the kernel and the device headers it is built from (jacobi_small.h, spectral_solve.h) stay in that unit.
//
// suggest(SPECTRAL) (qcqp.py:41-70 + 391-393) for B problems of n <= 64 variables inside ONE persistent launch
// (qcqpmi_spectral_small_batch).  The reference sums all constraints of one relop into one and relaxes; for problems whose constraints
// all carry the SAME relop and aggregate to
//        c(x) = sum_i (a_i x_i^2 + beta_i x_i) + gamma  (relop)  0,      every a_i > 0,   rho^2 = sum_i beta_i^2 / (4 a_i) - gamma > 0
// (Boolean, x_i^2 == d_i, MAXCUT, boxes and discs written as (x - lo)(x - hi) <= 0 or == 0) that relaxation has ONE quadratic
// constraint, is exact, and its value is the value of  min f0(x) s.t. c(x) (relop) 0:  a trust-region problem on a sphere (==) or a
// ball (<=).  With s = sqrt(a) and y_i = s_i x_i + beta_i / (2 s_i):  c = |y|^2 - rho^2 and f0 = y'Ay + 2 g'y + const,
//        A_ij = P0_ij / (s_i s_j),      g_i = (q0_i / 2 - (P0 h)_i) / s_i,      h_i = beta_i / (2 a_i)        (x = y / s - h).
//
// ONE WAVEFRONT PER PROBLEM, one wavefront per workgroup; a wave draws its problems from a global counter (an ordinary atomic add)
// and never waits for another wave.  Per problem, n2 = n rounded up to even:
//   stage     A_b (n2 rows of 65 doubles, padding zero) in LDS, lane-strided over the entries; P0_b[i][j] is compared with P0_b[j][i]
//             (the diagonal with itself: a NaN) and ticket[1] is set on a mismatch.  lane = i: s_i, h_i;  (P0 h)_i = sum_j P0_b[j][i] h_j
//             by fma in ascending j from 0.0;  g_i;  rho^2 = wave_sum_tree(beta_i^2 / (4 a_i)) - gamma.
//   Jacobi    jacobi_small (jacobi_small.h): eigenvalues on the diagonal of the image, eigenvector k = row k of Q.
//   spectrum  lane = eigen-index k (Jacobi's order, NOT sorted): lam_k, gh_k = sum_i Q[k][i] g_i by fma in ascending i from 0.0;
//             lam_min and max |lam| by wave_max; d_k = lam_k - lam_min; rank_k = the number of j with lam_j < lam_k, or equal and j < k
//             (lam [B][n] is written ascending through it; k_min = the lane of rank 0).
//   branch    interior (0), <= only: lam_min > 0 and wave_sum_tree((gh_k / lam_k)^2) <= rho^2: mu = 0, w_k = -gh_k / lam_k.
//             Else sigma_lo = lam_min where the relop is <= and lam_min > 0, else 0.  Where sigma_lo == 0 the hard-case rule of
//             spectral_solve.h is asked, its four sums by wave_sum_tree: hard (2): sigma = 0, w_k = -gh_k / d_k (0 for the dropped
//             components), tau = sqrt(rho^2 - sum w_k^2), and tau q_min is added, q_min = row k_min of Q with its entry of largest
//             magnitude positive (lowest index on ties).  Otherwise boundary (1): sigma = secular_root from sigma_0 =
//             max(sigma_lo, wave_max(|gh_k| / rho - d_k)) and the right end sqrt(wave_sum_tree(gh_k^2)) / rho, psi and T by
//             wave_sum_tree of the per-lane terms of secular_eval; w_k = -gh_k / (d_k + sigma).  mu = sigma - lam_min.
//   point     lane = i: y_i = sum_k Q[k][i] w_k by fma in ascending k from 0.0 (+ tau q_min,i); x_i = (y_i - beta_i / (2 s_i)) / s_i;
//             bound = wave_sum_tree(x_i ((P0 x)_i + q0_i)) + r0, (P0 x)_i = sum_j P0_b[j][i] x_j by fma in ascending j from 0.0.
// status: 0; 1 if Jacobi stopped at max_sweeps; 2 if the bound, mu or a coordinate of x is not finite.
// A problem's result depends on (P0_b, q0_b, r0_b, agg_b, relop, max_sweeps, tol) alone -- every sum has one fixed order -- not on
// B, the problems beside it, the number of workgroups or the order in which the problems are dealt out: bit for bit.
// LDS per wave: (2 * 65 n2 + 96 + 5 * 64) doubles (A, Q, the rotations of a round, five vectors): 69 888 bytes at n = 64 (two waves
// per CU of 160 KiB), 36 608 at n = 32 (four).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qcqpmi {

constexpr int SPECTRAL_SMALL_MAXN = 64;      // lane = coordinate, lane = eigen-index

struct SpectralSmallArgs {
    int n;
    int64_t B;
    const double *P0s;           // [B][n][n] symmetric
    const double *q0s;           // [B][n]
    const double *r0s;           // [B]
    const double *agg;           // [a (n) | beta (n) | gamma] shared by the problems (agg_stride = 0), or per problem (agg_stride = 2 n + 1)
    int64_t agg_stride;
    int relop_eq;                // 1: c(x) == 0 (sphere); 0: c(x) <= 0 (ball)
    int max_sweeps;
    double tol;
    int *ticket;                 // [0] zeroed before the launch: next problem; [1] set when some P0_b is not symmetric
    double *x;                   // [B][n]
    double *bound;               // [B] f0(x), recomputed from P0_b, q0_b, r0_b
    double *mu;                  // [B]
    double *lam;                 // [B][n] eigenvalues of A_b, ascending
    int64_t *sweeps;             // [B] Jacobi sweeps
    int *branch;                 // [B] 0 interior, 1 boundary, 2 hard case
    int *status;                 // [B]
};

size_t spectral_small_lds_bytes(int n);
// workgroups of the launch (persistent: at most what the device holds at once), or < 0: -hipError_t
int spectral_small_workgroups(int n, int64_t B, int device);
int spectral_small_launch(const SpectralSmallArgs &a, int wgs, hipStream_t st);

}  // namespace qcqpmi
