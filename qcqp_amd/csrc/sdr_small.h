// Small-problem SDR batch kernel: interface between its driver (capi_small.hip) and sdr_small.hip (own translation unit).
//
// suggest(SDR) (qcqp.py:72-97 + 394-396) for B problems of n <= 64 variables that share the constraints x_i^2 = d_i (the unit-diagonal
// family of sdr.unit_diagonal_family) and differ in their objective (P0_b, q0_b, r0_b) -- the batch of cd_small.h -- inside ONE
// persistent launch (qcqpmi_sdr_small_batch): the relaxation
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
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qcqpmi {

constexpr int SDR_SMALL_MAXN = 64;       // lane = coordinate in the sampling product; N = n + 1 <= 65
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

size_t sdr_small_lds_bytes(int n);
// workgroups of the launch (persistent: at most what the device holds at once), or < 0: -hipError_t
int sdr_small_workgroups(int n, int64_t B, int device);
int sdr_small_launch(const SdrSmallArgs &a, int wgs, hipStream_t st);

}  // namespace qcqpmi
