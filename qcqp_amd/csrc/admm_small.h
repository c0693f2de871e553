// Small-problem ADMM batch kernel: interface between its driver (capi_small.hip) and admm_small.hip (own translation unit).
//
// improve_admm (qcqp.py:254-285: phase 1, `better`, phase 2 with its bestx bookkeeping, `better`) for B problems of n <= 64 variables
// with separable constraints (up to four per coordinate: the lists of qcqpmi_cd_small_batch_run) that differ in their objective
// (P0_b, q0_b, r0_b) -- and, with cons, in the coefficients of their constraints --, R restarts each, inside ONE persistent launch
// (qcqpmi_admm_small_batch_run).  The loop, its exits and its iteration counts are those of orc_admm_phase1 /
// orc_admm_phase2 (oracle/qcqp_oracle.c); the projection is admm_small_solve<1> (admm.h), the operand and dual expressions are those of
// admm_unit_step_kernel.  Restart (b, r) starts from the keyed normals (seed + b seed_stride, first_index + r) or from X0 and depends
// on nothing but (problem b, rho_b, Minv_b, its start): not on B, the neighbours, the workgroups or the order in which the work is
// dealt out.
//
// 64 < n <= 128 (qcqpmi_admm_batch_run): the wide kernels admm_small_kernel<MAXC, pc, 2> -- one wavefront per (problem,
// restart) as before, two coordinates per lane, the same LDS image (up to 144 392 bytes), the same parity statement.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "small_batch.h"      // the LDS image, the ticket frame

namespace qcqpmi {

constexpr int ADMM_SMALL_MAXN = 64;      // lane = coordinate: one wavefront holds a point
constexpr int ADMM_WIDE_MAXN = 128;      // the wide kernels (admm_small_kernel<MAXC, pc, 2>): lane l holds coordinates l and l + 64
// their largest workgroup; the launch takes 256 or 512 threads, whichever puts more waves on a CU (admm_small_workgroups)
constexpr int ADMM_WIDE_THREADS = 512;

struct AdmmSmallArgs {
    DevProblem P;                // n, m and the per-coordinate constraint lists (cptr / cp / cq / cr / crel / cidx); its objective is not read
    int64_t B, R;
    int64_t RC, chunks;          // a ticket = (problem, RC consecutive restarts); chunks = tickets per problem
    const double *P0s;           // [B][n][n] symmetric (read from global memory: the objective of the two or three points that no solve produced)
    const double *q0s;           // [B][n]
    const double *r0s;           // [B]
    const double *rhos;          // [B]
    const double *Minvs;         // [B][n][n] (2 (P0_b + rho_b m I))^-1, symmetric (staged in LDS)
    const double *X0;            // [B][R][n] start points (generate == 0), else unused
    const double *cons;          // per-problem constraint coefficients [B][m][3] = (p, q, r) in CONSTRAINT order, or nullptr: P's
    int generate, phase1;
    int64_t num_iters;
    double tol, viol_lim;
    uint64_t seed, seed_stride, first_index;
    int *ticket;                 // [0] zeroed before the launch: next ticket; [1] set when some P0_b or Minv_b is not symmetric
    // per restart [B R]
    int64_t *iters1, *iters2;
    double *f0, *maxviol;
    double *X;                   // [B][R][n] final points
};

// workgroups of the launch (small_workgroup_cap; pc_entries: as small_image_bytes takes it), or < 0: -hipError_t; *threads: the size of a workgroup
// -- 256 for n <= ADMM_SMALL_MAXN; for the wide kernels 256 or ADMM_WIDE_THREADS, whichever the occupancy query gives more resident
// waves (a tie goes to the larger one)
int admm_small_workgroups(int64_t n, int maxc, int64_t pc_entries, int64_t tickets, int device, int *threads);
int admm_small_launch(const AdmmSmallArgs &a, int maxc, int wgs, int threads, hipStream_t st);      // a.cons != nullptr: the <MAXC, pc> kernels
const char *admm_small_name(int maxc, bool pc, bool wide);

}  // namespace qcqpmi
