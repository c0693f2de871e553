// Small-problem improve CHAIN kernel: interface between its driver (capi_small.hip) and chain_small.hip (own translation unit).
//
// improve([method_0, ..., method_{S-1}]) (qcqp.py:420-432: the methods one after the other, each from the point the previous one left)
// for the batch of qcqpmi_cd_small_batch_run / qcqpmi_admm_small_batch_run -- B problems of n <= 64 variables over the context's
// separable constraint lists, R restarts each -- inside ONE persistent launch (qcqpmi_chain_small_batch_run).  A stage
// is COORD_DESCENT (sm_restart, sm_restart.h) or ADMM (as_restart, as_restart.h) with arguments of its own; stage 0 starts from the
// keyed normals (seed + b seed_stride, first_index + r) or from X0, stage s > 0 from the point stage s - 1 wrote, whatever that stage
// reported about it; every stage keys its draws with the same (seed + b seed_stride, first_index + r).  Restart (b, r) of stage s is bit
// for bit what the single calls give when they are made one after the other with X of one as X0 of the next: the same device
// functions on the same inputs.  A result depends on nothing but (problem b, rho_b, Minv_b, seed of b, global index, the stages).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "small_batch.h"      // the LDS image, the chain frame

namespace qcqpmi {

constexpr int CHAIN_SMALL_MAXN = 64;     // lane = coordinate: one wavefront holds a point
constexpr int CHAIN_MAX_STAGES = 4;
constexpr int CHAIN_CD = 0, CHAIN_ADMM = 1;      // ChainStage::method (qcqpmi_chain_stage::method)

struct ChainStage {
    int method, phase1;
    int64_t num_iters;
    double tol, viol_tol, viol_lim;      // CD reads tol and viol_tol, ADMM tol and viol_lim
    // this stage's records, per restart [B R]; a CD stage writes the first seven, an ADMM stage iters1 / iters2, both f0 / maxviol
    int64_t *sweeps1, *sweeps2, *visits2, *accepted2;
    uint8_t *ran2;
    int *status1, *status2;
    int64_t *iters1, *iters2;
    double *f0, *maxviol;
};

struct ChainSmallArgs {
    DevProblem P;                // n, m and the per-coordinate constraint lists; its objective is not read
    int64_t B, R;
    int64_t RC, chunks;          // a ticket = (problem, RC consecutive restarts); chunks = tickets per problem
    const double *P0s;           // [B][n][n] symmetric: the image of a CD stage; an ADMM stage reads it from global memory
    const double *q0s;           // [B][n]
    const double *r0s;           // [B]
    const double *rhos;          // [B]        (ADMM stages)
    const double *Minvs;         // [B][n][n]  (ADMM stages: their image)
    const double *X0;            // [B][R][n] start points of stage 0 (generate == 0), else unused
    const double *cons;          // per-problem constraint coefficients [B][m][3], or nullptr: P's
    int generate, nstages;
    uint64_t seed, seed_stride, first_index;
    int *ticket;                 // [0] zeroed before the launch: next ticket; [1] set when a staged or scanned matrix is not symmetric
    double *X;                   // [B][R][n]: every stage writes its points here and the next one starts from them (in place)
    ChainStage st[CHAIN_MAX_STAGES];
};

// workgroups of the launch (small_workgroup_cap; pc_entries: as small_image_bytes takes it), or < 0: -hipError_t; workgroups of 256 threads
int chain_small_workgroups(int64_t n, int maxc, int64_t pc_entries, int64_t tickets, int device);
int chain_small_launch(const ChainSmallArgs &a, int maxc, int wgs, hipStream_t st);      // a.cons != nullptr: the <MAXC, pc> kernels
const char *chain_small_name(int maxc, bool pc);

}  // namespace qcqpmi
