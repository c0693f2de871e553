// Symmetric eigen-solver for ONE small matrix (n2 <= 64) by ONE wavefront, the matrix and the eigenvectors in LDS: cyclic two-sided
// Jacobi with a fixed round-robin ordering.  A device function for the batch kernels (spectral_small.hip runs it; a device-side setup
// of batched ADMM could).  It takes the rotation and the ordering from spectral_solve.h -- two scalar functions that a host program
// can test -- and nothing else of the spectral suggest.
//
// Layout.  As and Qs: n2 rows of JACOBI_STR = 65 doubles, n2 EVEN (an odd matrix is padded by its caller with a decoupled coordinate:
// a zero row and column; a rotation with a_pq == 0 is the identity, so the padding never mixes and stays at its index).  On return
// the diagonal of As holds the eigenvalues in NO particular order and ROW k of Qs is the eigenvector of As[k][k]:
//        A = sum_k As[k][k] Qs[k][:]' Qs[k][:].
// A row stride of 65 doubles puts the 32 lanes of a half-wave on 32 different bank pairs whether they walk along a row (lane =
// column: consecutive doubles) or down a column (lane = row: 130 dwords apart, 2 lane mod 64): no read or write below conflicts.
//
// A sweep is n2 - 1 rounds; a round has n2 / 2 disjoint pairs (p, q) = round_robin_pair(n2, round, slot):
//   1. lane = slot: the rotation of (a_pp, a_qq, a_pq), read from the UPPER triangle (p < q), left in LDS with its pair;
//   2. lane = column j, slot after slot: rows p and q of A and of Q:  (row_p, row_q) <- (c row_p - s row_q, s row_p + c row_q);
//   3. lane = row i, slot after slot: columns p and q of A the same way;
//   4. lane = slot: a_pp = app - t apq, a_qq = aqq + t apq, a_pq = a_qp = 0 exactly.
// Slots whose rotation is the identity (a_pq == 0 or negligible, below) are skipped in 2 to 4.  Between the steps stands the barrier of
// a one-wave workgroup.
// Before every sweep: off2 = sum_{i != j} a_ij^2 (lane = column j, ascending i, then wave_sum_tree); the solver stops at
// off2 <= tol^2 |A|_F^2 (|A|_F^2 summed the same way before the first sweep) or after max_sweeps sweeps.
//
// A NEGLIGIBLE a_pq is not rotated: a_pq^2 <= JACOBI_NEGLIGIBLE2 tol^2 |A|_F^2, that is |a_pq| <= 2^-60 tol |A|_F.  Were all n2^2 <= 2^12
// entries that small, off(A) would be 2^-54 tol |A|_F: the stop test cannot see it and no eigenvalue moves by it.  Why it has to be
// said: inside an eigenspace of a repeated eigenvalue the off-diagonal entries fall quadratically (1e-20, 1e-40, ... 1e-300) while
// a_pp == a_qq exactly, so theta == 0 and the rotation is by 45 degrees however small a_pq is -- until it underflows.  The eigenvectors
// inside that eigenspace then depended on WHERE the underflow came, that is on the scale of A (seen: the same matrix times 2^-100 came
// back with other eigenvectors, four rotations driven by entries of 1e-278 to 1e-314).  With the rule a power-of-two scaling of A is
// exact as long as 2^-120 tol^2 |A|_F^2 is a normal number.
//
// Magnitude.  The stop test needs |A|_F^2 as a positive finite number: the squares of the entries must neither all underflow nor
// overflow.  A matrix with a nonzero entry whose |A|_F^2 comes out as 0.0 would pass `off2 <= stop2` as 0 <= 0 before any sweep, one
// whose |A|_F^2 is not finite as anything <= inf: `degenerate` reports both, and the callers turn it into status 2 (the diagonal
// and Qs = I that come back are NOT a decomposition).  The all-zero matrix is not degenerate: 0 sweeps, converged, Q = I.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_util.h"
#include "spectral_solve.h"

namespace qcqpmi {

constexpr int JACOBI_MAXN = 64;
constexpr int JACOBI_STR = 65;                                    // row stride of As and Qs (doubles)
constexpr int JACOBI_ROT_DOUBLES = 3 * (JACOBI_MAXN / 2);         // scratch: c, s per slot and the slot's pair (two ints in a double's place)
constexpr double JACOBI_NEGLIGIBLE2 = 0x1p-120;                   // a_pq^2 <= this times tol^2 |A|_F^2: not rotated (see above)

// doubles of LDS that the solver needs for an n2 x n2 matrix: As, Qs and the rotations of a round
__host__ __device__ inline size_t jacobi_small_doubles(int n2) { return (size_t)2 * n2 * JACOBI_STR + JACOBI_ROT_DOUBLES; }

struct JacobiResult { int sweeps; bool converged; bool degenerate; double fro2; };

// As: the matrix (symmetric, n2 even, padding in place); Qs: set to the identity here; rot: JACOBI_ROT_DOUBLES doubles.
// Called by all 64 lanes of a one-wave workgroup.
__device__ inline JacobiResult jacobi_small(double *As, double *Qs, double *rot, int n2, int lane, int max_sweeps, double tol) {
    const int half = n2 / 2;
    const bool on = lane < n2;
    double *rc = rot, *rs = rot + JACOBI_MAXN / 2;
    int *rpq = (int *)(rot + JACOBI_MAXN);
    for (int i = 0; i < n2; i++) Qs[i * JACOBI_STR + lane] = lane == i ? 1.0 : 0.0;
    double f = 0.0;
    bool nz = false;
    if (on) for (int i = 0; i < n2; i++) { const double a = As[i * JACOBI_STR + lane]; f += a * a; nz = nz || a != 0.0; }
    JacobiResult res;
    res.fro2 = wave_sum_tree(f);
    res.degenerate = !(res.fro2 < __builtin_huge_val()) || (res.fro2 == 0.0 && __ballot(nz) != 0);
    res.sweeps = 0;
    res.converged = false;
    const double stop2 = tol * tol * res.fro2;
    const double negl2 = JACOBI_NEGLIGIBLE2 * stop2;
    for (;;) {
        double o = 0.0;
        if (on) for (int i = 0; i < n2; i++) { const double a = As[i * JACOBI_STR + lane]; if (i != lane) o += a * a; }
        const double off2 = wave_sum_tree(o);
        if (off2 <= stop2) { res.converged = true; break; }
        if (res.sweeps >= max_sweeps || !(off2 == off2)) break;
        for (int round = 0; round < n2 - 1; round++) {
            int p = 0, q = 0;
            double app = 0.0, aqq = 0.0, apq = 0.0;
            JacobiRot r = {1.0, 0.0, 0.0};
            if (lane < half) {
                round_robin_pair(n2, round, lane, &p, &q);
                app = As[p * JACOBI_STR + p]; aqq = As[q * JACOBI_STR + q]; apq = As[p * JACOBI_STR + q];
                if (!(apq * apq <= negl2)) r = jacobi_rotation(app, aqq, apq);
                rc[lane] = r.c; rs[lane] = r.s; rpq[2 * lane] = p; rpq[2 * lane + 1] = q;
            }
            __syncthreads();
            for (int k = 0; k < half; k++) {
                const double s = rs[k];
                if (s == 0.0) continue;
                const double c = rc[k];
                const int pk = rpq[2 * k] * JACOBI_STR + lane, qk = rpq[2 * k + 1] * JACOBI_STR + lane;
                if (on) {
                    const double ap = As[pk], aq = As[qk], vp = Qs[pk], vq = Qs[qk];
                    As[pk] = c * ap - s * aq; As[qk] = s * ap + c * aq;
                    Qs[pk] = c * vp - s * vq; Qs[qk] = s * vp + c * vq;
                }
            }
            __syncthreads();
            for (int k = 0; k < half; k++) {
                const double s = rs[k];
                if (s == 0.0) continue;
                const double c = rc[k];
                const int pk = lane * JACOBI_STR + rpq[2 * k], qk = lane * JACOBI_STR + rpq[2 * k + 1];
                if (on) {
                    const double ap = As[pk], aq = As[qk];
                    As[pk] = c * ap - s * aq; As[qk] = s * ap + c * aq;
                }
            }
            __syncthreads();
            if (lane < half && r.s != 0.0) {
                As[p * JACOBI_STR + p] = app - r.t * apq;
                As[q * JACOBI_STR + q] = aqq + r.t * apq;
                As[p * JACOBI_STR + q] = 0.0;
                As[q * JACOBI_STR + p] = 0.0;
            }
            __syncthreads();
        }
        res.sweeps++;
    }
    return res;
}

}  // namespace qcqpmi
