// Small-problem batch kernel: interface between its driver (capi_small.hip) and cd_small.hip (own translation unit).
//
// improve_coord_descent (qcqp.py:181-192) for B problems of n <= 64 variables that share ONE set of separable constraint lists
// and differ in their objective (P0_b, q0_b, r0_b) -- a frame of MIMO detection problems: thousands of Boolean least squares
// instances of n = 8..64 -- R restarts each, inside ONE persistent launch (qcqpmi_cd_small_batch_run).  Restart (b, r) is the
// restart r that qcqpmi_pop_randn(R, seed + b seed_stride, first_index) + qcqpmi_cd_run(seed + b seed_stride, first_index) produce on
// a context that holds the constraints and objective b: the keyed draws go by the GLOBAL restart index first_index + r, so a
// result depends on nothing but (objective b, seed of b, global index) -- not on B, the neighbours, the workgroups or the order
// in which the work is dealt out.
//
// Per-problem constraint coefficients (qcqpmi_cd_small_batch_run_pc): the context fixes the STRUCTURE of the lists
// (cptr, crel, maxc -- which coordinate a constraint touches, its relop) and problem b brings (p, q, r) of every constraint in
// cons [B][m][3]; the ticket's workgroup stages them in LDS beside P0_b.  Restart (b, r) is then bit for bit the restart of the shared
// call with B = 1 on a context created from problem b's own functions.
//
// 64 < n <= 128 (qcqpmi_cd_batch_run): the wide kernels cd_small_kernel<MAXC, pc, 2> -- one wavefront per (problem,
// restart) as before, two coordinates per lane, the same LDS image (up to 144 392 bytes), the same parity statement.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "small_batch.h"      // the LDS image, the ticket frame, small_gather_launch

namespace qcqpmi {

constexpr int CD_SMALL_MAXN = 64;        // lane = coordinate: one wavefront holds a point
constexpr int CD_WIDE_MAXN = 128;        // the wide kernels (cd_small_kernel<MAXC, pc, 2>): lane l holds coordinates l and l + 64
// their largest workgroup: from n = 101 the LDS image lets ONE workgroup on a CU, so its size decides how many waves the CU holds (eight;
// with __launch_bounds__(768) the kernels for one constraint per coordinate, at 168 VGPRs, spill 8 bytes per lane: DESIGN.md 4.12).
// The launch takes 256 or 512 threads, whichever puts more waves on a CU (cd_small_workgroups).
constexpr int CD_WIDE_THREADS = 512;

struct CdSmallArgs {
    DevProblem P;                // n and the shared per-coordinate constraint lists (cptr / cp / cq / cr / crel); its objective is not read
    int64_t B, R;
    int64_t RC, chunks;          // a ticket = (problem, RC consecutive restarts); chunks = tickets per problem
    const double *P0s;           // [B][n][n] symmetric
    const double *q0s;           // [B][n]
    const double *r0s;           // [B]
    const double *X0;            // [B][R][n] start points (generate == 0), else unused
    int generate, phase1;
    int64_t num_iters;
    double viol_tol, tol;
    uint64_t seed, seed_stride, first_index;
    int *ticket;                 // [0] zeroed before the launch: next ticket; [1] set when some P0_b is not symmetric
    // per restart [B R]
    int64_t *sweeps1, *sweeps2, *visits2, *accepted2;
    uint8_t *ran2;
    int *status1, *status2;
    double *f0, *maxviol;
    double *X;                   // [B][R][n] final points
    const double *cons;          // per-problem constraint coefficients [B][m][3] = (p, q, r) in CONSTRAINT order, or nullptr: P's
};

// workgroups of the launch (small_workgroup_cap; pc_entries: as small_image_bytes takes it), or < 0: -hipError_t; *threads: the size of a workgroup
// -- 256 for n <= CD_SMALL_MAXN; for the wide kernels 256 or CD_WIDE_THREADS, whichever the occupancy query gives more resident waves
// (a tie goes to the larger one)
int cd_small_workgroups(int64_t n, int maxc, int64_t pc_entries, int64_t tickets, int device, int *threads);
int cd_small_launch(const CdSmallArgs &a, int maxc, int wgs, int threads, hipStream_t st);      // a.cons != nullptr: the <MAXC, pc> kernels
const char *cd_small_name(int maxc, bool pc, bool wide);

}  // namespace qcqpmi
