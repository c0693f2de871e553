// Small-problem SDR batch kernel: interface between its driver (capi_small.hip) and sdr_small.hip (own translation unit).
//
// suggest(SDR) (qcqp.py:72-97 + 394-396) for B problems of n <= 128 variables (n <= 64: sdr_small_kernel<false>; 65 <= n <= 128:
// sdr_small_kernel<true>, "the wide kernel", below) that share the constraints x_i^2 = d_i (the unit-diagonal
// family of sdr.unit_diagonal_family) and differ in their objective (P0_b, q0_b, r0_b) -- the batch of cd_small.h -- inside ONE
// persistent launch (qcqpmi_sdr_small_batch, qcqpmi_sdr_batch): the relaxation
//        minimise <C_b, X>  s.t.  X_ii = 1, X PSD,      N = n + 1,  s = sqrt(d),
//        C_b[:n,:n] = P0_b o s s^T,  C_b[:n,n] = C_b[n,:n] = q0_b o s / 2,  C_b[n,n] = r0_b          (sdr.lifted_cost)
// by the mixing method of sdr_solve.h (rank K = 64, unit rows, cyclic g_i = sum_{j != i} C_ij v_j, v_i <- -g_i / ||g_i||, a row with
// g_i = 0 is left as it is; the sweep objective tracked by the exact decrease of every update; stop at |delta_sweep| <= tol (1 + |f|)
// or max_sweeps; objective recomputed at the end), the multipliers y_i = -v_i . (C v)_i (sdr.dual_certificate) and S samples
//        x = s o (V_n u + V_n (xi - u (u . xi))),      u = v_n (the homogenising row),  V_n = the first n rows,
//        xi_k = keyed_normal(seed_b, first_index + sigma, k), k = 0..63
// of N(mu, Sigma) with mu = s o V_n u and Sigma = F F^T, F = diag(s) V_n (I - u u^T) -- the pair of qcqp.py:394-395; I - u u^T is a
// projector, so F F^T = diag(s) (V_n V_n^T - (V_n u)(V_n u)^T) diag(s) without any decomposition.
//
// The start.  seed_b = seed + b seed_stride.  Row i of V0 is the vector of keyed normals
//        z_k = keyed_normal(seed_b, 2^64 - 1 - i, k),  k = 0..63                                          (philox.h)
// divided by sqrt(sum_k z_k^2), the sum taken in the order of wave_sum_tree (dev_util.h: the binary tree over adjacent lanes -- pairs, quads, eights, ...).
// The rows count their restart index DOWN from 2^64 - 1 and the samples count theirs UP from first_index: the two ranges do not meet
// while first_index + S <= 2^64 - 65.  V0s [B][N][64], if given, is taken as it is instead (unit rows are the caller's business).
//
// A problem's result depends on (P0_b, q0_b, r0_b, d, seed_b, first_index) alone -- every sum has one fixed order -- not on B, the
// problems beside it, the number of workgroups or the order in which the problems are dealt out: bit for bit.
//
// The order of every sum (both kernels; tests/sdr_wide_cases.py restates it in NumPy).  N = n + 1, lane = component k in the sweeps.
//   g_i[k]      = sum_{j != i} C_ij V[j][k] as FOUR partial sums a_r over j = r (mod 4), each by fma in ascending j, over the full fours
//                 j < 4 floor(N / 4); the N mod 4 entries that are left (N = 129: one, N = 66: two) go to a_0 in ascending j; the term
//                 j == i is the fma of 0.0; g = (a0 + a1) + (a2 + a3).
//   wave sums   g . v_i, g . g, v_i . v_i: the products per lane, then wave_sum_tree.
//   a sweep     i = 0 .. N-1 in turn: gv = g . v_i, nrm = sqrt(g . g); where nrm > 0: v_i <- -g / nrm, dsweep += -2 (nrm + gv).
//               After the sweep f += dsweep; stop when |dsweep| <= tol (1 + |f|).
//   objective   (first and last pass, no update) t_i = gv + C_ii (v_i . v_i); f = t_0 + t_1 + ... in ascending i; y_i = -t_i.
//   samples     u = v_n.  t = wave_sum_tree(u_k xi_k); w_k = xi_k - u_k t.  For coordinate i: mu_i = sum_k V[i][k] u_k and
//               t_i = sum_k V[i][k] w_k, both by fma in ascending k from 0.0; x_i = s_i (mu_i + t_i).
// The wide kernel (65 <= n <= 128) differs in two places and in no sum:
//   C_b packed  the lower triangle with the diagonal, row after row: C_ij at tri(max(i, j)) + min(i, j), tri(i) = i (i + 1) / 2 --
//               N (N + 1) / 2 doubles instead of N^2.  Every address is wave-uniform, so the reads stay broadcasts.  The image is built
//               row by row (lane = column j <= i) with the products of the full one, C_ij = P0_b[i][j] (s_i s_j) for j <= i < n; every
//               P0_b[i][j] is compared with P0_b[j][i] (the diagonal with itself: a NaN), ticket[1] is set on a mismatch.
//   samples     two coordinates per lane, the slots of the other wide kernels (cd_small.h): lane l forms x_l and, where l + 64 < n,
//               x_{l+64} -- mu and t per coordinate as above, from the same u and the same w in LDS.  xi_k still comes from lane k.
// LDS per wave: (65 N + N^2 + 64) doubles for n <= 64, (65 N + N (N + 1) / 2 + 64) doubles past it: 52 520 bytes at n = 65 (three
// workgroups per CU by LDS), 88 976 at n = 96 (one), 134 672 at n = 128 (one).  One layout serves the whole wide range.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qcqpmi {

constexpr int SDR_SMALL_MAXN = 64;       // lane = coordinate in the sampling product; N = n + 1 <= 65
constexpr int SDR_WIDE_MAXN = 128;       // the wide kernel: two coordinates per lane in the sampling product, C_b packed
constexpr int SDR_SMALL_K = 64;          // rank of the factor: lane = component in the mixing sweeps
constexpr int SDR_SMALL_VSTR = 65;       // row stride of V in LDS (doubles): V[i][k] with lane = i is conflict-free

struct SdrSmallArgs {
    int n;                       // variables; N = n + 1
    int64_t B, S;
    const double *s;             // sqrt(d): [n] shared by the problems (s_stride = 0), or [B][n] (s_stride = n): problem b reads s + b s_stride
    int64_t s_stride;
    const double *P0s;           // [B][n][n] symmetric
    const double *q0s;           // [B][n]
    const double *r0s;           // [B]
    const double *V0s;           // [B][N][64] start, or nullptr: the keyed start above
    int max_sweeps;
    double tol;
    uint64_t seed, seed_stride, first_index;
    int *ticket;                 // [0] zeroed before the launch: next problem; [1] set when some P0_b is not symmetric
    double *V;                   // [B][N][64]
    double *primal;              // [B] <C_b, V V^T>, recomputed at the end
    double *y;                   // [B][N]
    int64_t *sweeps;             // [B] sweeps done
    double *X;                   // [B][S][n] samples (not written when S == 0)
};

size_t sdr_small_lds_bytes(int n);          // n <= SDR_SMALL_MAXN: the full C_b; past it the packed one (the kernel is chosen by n alike)
// workgroups of the launch (persistent: at most what the device holds at once), or < 0: -hipError_t
int sdr_small_workgroups(int n, int64_t B, int device);
int sdr_small_launch(const SdrSmallArgs &a, int wgs, hipStream_t st);

}  // namespace qcqpmi
