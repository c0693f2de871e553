// The scalar half of coordinate descent phase 2 (qcqp.py:152-178) that every phase-2 kernel shares: the one-variable
// feasible sets of separable constraints as LDS tables (they depend only on the constraint coefficients and on the
// restart's slack, both fixed during phase 2, qcqp.py:157,167), the quotient and broadcast helpers of the per-coordinate
// step, and the per-restart state of the sequential part with its commit rule.
#pragma once
#include "kernels.h"
#include "onevar.h"

namespace qcqpmi {

template <int MAXC>
struct SetTable {
    int *n;        // [slots] number of intervals
    int *slow;     // [slots] 1 if an end point is infinite (generic path needed)
    double *lo;    // [(MAXC+1)][slots]
    double *hi;    // [(MAXC+1)][slots]
    int slots;
};

template <int MAXC>
__device__ inline void store_set(const SetTable<MAXC> &T, int slot, const FeasSet<MAXC> &C) {
    bool inf = false;
#pragma unroll
    for (int j = 0; j <= MAXC; j++) {
        T.lo[j * T.slots + slot] = C.lo[j];
        T.hi[j * T.slots + slot] = C.hi[j];
        if (j < C.n && (__builtin_isinf(C.lo[j]) || __builtin_isinf(C.hi[j]))) inf = true;
    }
    T.n[slot] = C.n;
    T.slow[slot] = inf ? 1 : 0;
}

template <int MAXC>
__device__ inline void compute_set(const DevProblem &P, int list, double slack, FeasSet<MAXC> &C) {
    const int e0 = P.cptr[list], mf = P.cptr[list + 1] - e0;
    double cp[MAXC], cq[MAXC], cr[MAXC];
    int crel[MAXC];
#pragma unroll
    for (int k = 0; k < MAXC; k++) {
        bool ok = k < mf;
        cp[k] = ok ? P.cp[e0 + k] : 0.0; cq[k] = ok ? P.cq[e0 + k] : 0.0;
        cr[k] = ok ? P.cr[e0 + k] : 0.0; crel[k] = ok ? P.crel[e0 + k] : RELOP_LE;
    }
    if (mf == 1) feasible_set_single<MAXC>(cp[0], cq[0], cr[0], crel[0], slack, C);
    else feasible_set<MAXC>(cp, cq, cr, crel, mf, slack, C);
}

// near-IEEE quotient num/den from a precomputed reciprocal: one Newton correction in fma
// arithmetic (within 1 ulp of the correctly rounded quotient the reference computes).
__device__ inline double div_by_rcp(double num, double den, double rcp) {
    double q = num * rcp;
    double r = __builtin_fma(-q, den, num);
    return __builtin_fma(r, rcp, q);
}

// wave-uniform broadcast of a double held by lane `src` (static lane index)
__device__ inline double readlane_d(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

// feasible set of one (coordinate, restart) as the fast path consumes it (<= 2 intervals)
struct StepTab {
    double l0, h0, l1, h1, mid, thr;
    int n, slow;
};

// per-restart state of the sequential part
struct ChainState {
    double fcur;
    int64_t upd_counter, visits, accepted, sweeps;
    bool conv;
    int status;
};

template <int MAXC>
__device__ inline void chain_commit(ChainState &S, int got, double xn, double xi, double t2,
                                    double t1, double t0, double tol, int64_t n, bool &moved,
                                    double &delta) {
    moved = false;
    delta = 0.0;
    if (S.conv) return;
    S.visits++;
    if (got < 0) { S.status = got; S.conv = true; return; }
    if (got && fabs(xn - xi) > tol) {
        delta = xn - xi;
        moved = true;
        S.fcur = t0 + xn * (t2 * xn + t1);
        S.upd_counter = 0;
        S.accepted++;
    } else {
        S.upd_counter++;
        if (S.upd_counter == n) S.conv = true;
    }
}

}  // namespace qcqpmi
