// The two small kernels of coordinate descent on the resident population that belong to no kernel family of their own:
//
//   cd_phase1_sep     coordinate descent phase 1, separable constraints (qcqp.py:101-148); the visit is cd_phase1_sep.h's
//   gate_kernel       the gate of improve_coord_descent between the phases (qcqp.py:189)
//
// Not a translation unit: capi_cd.hip includes this file, and only it (the launches live there, next to those of the phase-2
// families cd_phase2.h, cd_phase2_rs.h, cd_phase2_q.h and of cd_general.h).
#pragma once
#include "kernels.h"
#include "cd_phase1_sep.h"

namespace qcqpmi {

// -------------------------------------------------------------------- coordinate descent phase 1

// Separable constraints: a coordinate's local violation and its update depend on x_i alone
// (objective is identically zero in phase 1, qcqp.py:114), so a sweep is element-wise; the
// sweep loop, the per-restart max-violation reduction and the termination tests stay in-kernel.
// 1024 threads = 64 coordinate slots x 16 restarts: 4 waves per SIMD hide the latency of the
// long scalar dependency chains (sqrt / divide / Philox) of the bisection.
constexpr int P1_THREADS = 1024, P1_SLOTS = P1_THREADS / 16;
template <int MAXC>
__global__ __launch_bounds__(P1_THREADS) void cd_phase1_sep_kernel(CdArgs a) {
    __shared__ double vred[P1_THREADS];
    __shared__ int ured[P1_THREADS];
    __shared__ double viol_last[16];
    __shared__ int fin[16];
    __shared__ int nlive;
    const DevProblem &P = a.P;
    const int tid = threadIdx.x;
    const int r = tid & 15, slot = tid >> 4;
    const int64_t tile = blockIdx.x;
    double *Xs = a.X + tile * P.n16 * 16;
    const int64_t gr = tile * 16 + r;
    const bool live = gr < a.R;
    if (tid < 16) { viol_last[tid] = QM_INF; fin[tid] = (tile * 16 + tid < a.R) ? 0 : 1; }
    int64_t my_visits = 0, my_acc = 0;
    int my_status = 0;
    int64_t sweeps_done = 0;
    __syncthreads();
    for (int64_t t = 0; t < a.num_iters; t++) {
        // loop-top test of the reference (qcqp.py:111) is folded into fin[]
        if (tid == 0) { int c = 0; for (int k = 0; k < 16; k++) c += fin[k] ? 0 : 1; nlive = c; }
        __syncthreads();
        if (nlive == 0) break;
        const bool run = live && !fin[r];
        double vmax = -QM_INF;
        int upd = 0;
        if (run) {
            if (slot == 0) sweeps_done++;
            for (int64_t i = slot; i < P.n; i += P1_SLOTS) {
                double xi = Xs[i * 16 + r];
                P1Visit V;
                p1_sep_visit<MAXC>(P, i, xi, a.tol, a.viol_tol, a.seed, a.first_index + (uint64_t)gr, t, V);
                if (V.status) my_status = V.status;
                if (!V.visited) continue;
                my_visits++;
                if (V.moved) { Xs[i * 16 + r] = xi; upd = 1; my_acc++; }
                vmax = V.vafter > vmax ? V.vafter : vmax;
            }
        }
        vred[tid] = vmax; ured[tid] = upd;
        __syncthreads();
        if (tid < 16 && !fin[tid]) {
            double v = -QM_INF;
            int u = 0;
            for (int g = 0; g < P1_SLOTS; g++) { double w = vred[g * 16 + tid]; v = w > v ? w : v; u |= ured[g * 16 + tid]; }
            viol_last[tid] = v;
            // done when feasible enough (qcqp.py:111); a sweep without any update is a fixed
            // point of the (deterministic-in-feasibility) map, so later sweeps cannot change x.
            if (v < a.viol_tol || !u) fin[tid] = 1;
        }
        __syncthreads();
    }
    // per-restart outputs
    vred[tid] = (double)my_visits; ured[tid] = (int)my_acc;
    __shared__ int sred[P1_THREADS];
    sred[tid] = my_status;
    __syncthreads();
    if (tid < 16 && tile * 16 + tid < a.R) {
        int64_t vis = 0, acc = 0;
        int st = 0;
        for (int g = 0; g < P1_SLOTS; g++) { vis += (int64_t)vred[g * 16 + tid]; acc += ured[g * 16 + tid]; if (sred[g * 16 + tid]) st = sred[g * 16 + tid]; }
        int64_t g = tile * 16 + tid;
        a.visits[g] = vis; a.accepted[g] = acc; a.status[g] = st;
        a.flag[g] = (viol_last[tid] < a.viol_tol) ? 1 : 0;
    }
    if (slot == 0 && live) a.sweeps[gr] = sweeps_done;
}

// gate of improve_coord_descent (qcqp.py:189): phase 2 runs only for restarts whose max violation
// is below viol_tol (and whose phase 1 did not hit a case where the reference raises)
__global__ void gate_kernel(const double *__restrict__ maxviol, const int *__restrict__ status1,
                            uint8_t *__restrict__ flag, int64_t R, int64_t Rpad, double viol_tol) {
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= Rpad) return;
    flag[r] = (r < R && status1[r] == 0 && maxviol[r] < viol_tol) ? 1 : 0;
}

}  // namespace qcqpmi
