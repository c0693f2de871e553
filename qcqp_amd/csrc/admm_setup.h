// Device-side setup of the batched ADMM: interface between its driver (capi_small.hip) and the kernels admm_setup_kernel (n <= 64) and
// admm_setup_wide_kernel (65 <= n <= 128) of admm_setup_kernel.h, which are built in the unit of the spectral kernels
// (spectral_small.hip: they run its two eigen-solvers, jacobi_small.h and jacobi_wide.h).  Host declarations only.
//
// improve(ADMM) needs two things per problem before its launch (qcqp_amd/batch.py: admm_rhos, admm_minvs): rho_b by the reference's
// rule from lambda_min(P0_b) (qcqp.py:261-278) and Minv_b = (2 (P0_b + rho_b m I))^-1.  With P0_b = sum_k lam_k u_k u_k' both fall
// out of ONE eigendecomposition:
//        rho_b = admm_setup_rho(min_k lam_k, m)  (admm_setup_rule.h),      Minv_b = sum_k w_k u_k u_k',   w_k = 1 / (2 (lam_k + rho_b m)).
//
// ONE WAVEFRONT PER PROBLEM, one wavefront per workgroup, problems drawn from a global counter by the branch-free draw of
// spectral_small_kernel; no wave waits for another.  Per problem, n2 = n rounded up to even:
//   stage     P0_b itself (no scaling) with zero padding into the solver's array -- narrow: As, n2 rows of JACOBI_STR doubles,
//             lane-strided over the entries; wide: G, column-major with stride jacobi_wide_stride(n2), entry (i, j) by the lane of j.
//             P0_b[i][j] is compared with P0_b[j][i] (the diagonal with itself: a NaN) and ticket[1] is set on a mismatch.
//   Jacobi    narrow: jacobi_small; lam_k = As[k][k], ROW k of Qs = u_k.  Wide: jacobi_wide; COLUMN k of G = u_k, and lam_k is the
//             Rayleigh quotient u_k' P0_b u_k: row i of P0_b from global memory into one of two row buffers (one operand for all
//             lanes), lane = eigen-index k (and k + 64):  t = sum_j P0_ij u_jk by fma in ascending j from 0.0, lam_k = sum_i u_ik t by
//             fma in ascending i from 0.0 -- the pass of spectral_wide_kernel, restated (a second copy: the first one divides every
//             entry by s_i s_j on its way and keeps the spectral kernel's instructions as they are).
//   minimum   lambda_min = the wave minimum (wave_max of the negated values; wide: the lane's two slots first) over the n REAL
//             eigen-indices.  The padding index n2 - 1 of an odd n (eigenvalue 0 / a unit column, at its index to the end) enters
//             neither the minimum nor the sums below.
//   rho       no rho given: admm_setup_rho(lambda_min, m).  rho given: rho_b = rho, and status 3 where lambda_min + m rho < 0 (Minv_b
//             is then not written).
//   inverse   w_k = admm_setup_weight(lam_k, rho_b, m) in LDS.  lane = column j (wide: j and j + 64), rows i four at a time:
//             Minv_b[i][j] = sum_k (u_ik u_jk) w_k over the real eigen-indices k in ascending SOLVER index, acc = fma(u_ik * u_jk, w_k,
//             acc) from 0.0.  The product of the two vector entries is formed first, so entries (i, j) and (j, i) are the same bits
//             (the ADMM kernels refuse an inverse that is not exactly symmetric).  The lane's operand comes from consecutive LDS
//             addresses, the row's operand is one address for all lanes, the stores of a row are coalesced; the output never lives
//             in LDS.
// status: 0; 1 if Jacobi stopped at max_sweeps; 2 if lambda_min, rho_b, a weight or an entry of Minv_b is not finite; 3 if the given
// rho is too small (it wins over 1).  sweeps as the solvers count them (the wide one counts its last sweep, without a rotation; 0
// where |P0_b|_F == 0).
// A problem's result depends on (P0_b, m, the rho argument, max_sweeps, tol) alone -- every sum has one fixed order -- not on B, the
// problems beside it, the number of workgroups or the order in which the problems are dealt out: bit for bit.
// LDS per wave (lam_k stays in its lane's registers).  Narrow: (2 * 65 n2 + 96 + 64) doubles (A, Q, the rotations of a round, w):
// 67 840 bytes at n = 64.  Wide: (n2 (n2 + 1) + 3 * 128) doubles (G, two row buffers, w): 135 168 bytes at n = 128, below the
// 137 216 of spectral_wide_kernel (one wave per CU either way).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qcqpmi {

constexpr int ADMM_SETUP_SMALL_MAXN = 64;    // lane = column, lane = eigen-index
constexpr int ADMM_SETUP_MAXN = 128;         // two indices per lane

struct AdmmSetupArgs {
    int n;
    int64_t B;
    const double *P0s;           // [B][n][n] symmetric
    double m;                    // the context's number of constraints: what the ADMM run multiplies rho by
    int has_rho;                 // 0: the reference's rule; 1: `rho` for every problem
    double rho;
    int max_sweeps;
    double tol;
    int *ticket;                 // [0] zeroed before the launch: next problem; [1] set when some P0_b is not symmetric
    double *rhos;                // [B]
    double *lambda_min;          // [B]
    double *Minvs;               // [B][n][n], exactly symmetric; problems of status 3 are left as they were
    int64_t *sweeps;             // [B] Jacobi sweeps
    int *status;                 // [B]
};

// n <= ADMM_SETUP_SMALL_MAXN: admm_setup_kernel; ADMM_SETUP_SMALL_MAXN < n <= ADMM_SETUP_MAXN: admm_setup_wide_kernel
size_t admm_setup_lds_bytes(int n);
// workgroups of the launch (persistent: at most what the device holds at once), or < 0: -hipError_t
int admm_setup_workgroups(int n, int64_t B, int device);
int admm_setup_launch(const AdmmSetupArgs &a, int wgs, hipStream_t st);

}  // namespace qcqpmi
