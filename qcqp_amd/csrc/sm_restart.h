// sm_restart -- ONE restart of improve_coord_descent by ONE wavefront on the LDS image of a small problem: the restart body of
// cd_small_kernel (cd_small.hip, whose header describes the layout) and of the CD stages of chain_small_kernel (chain_small.hip).
// Self-contained; everything here has internal linkage: a translation unit that includes it gets instances of its own.
#pragma once
#include "cd_small.h"      // CdSmallArgs

#include "onevar.h"
#include "cd_phase1_sep.h"
#include "cd_chain.h"      // compute_set, ChainState, chain_commit, readlane_d
#include "dev_util.h"

namespace qcqpmi {
namespace {

// max violation of coordinate i's own constraints at xi (the expression of eval_kernel; -inf without a constraint)
__device__ inline double sm_coord_viol(const DevProblem &P, int i, double xi) {
    double v = -QM_INF;
    for (int e = P.cptr[i]; e < P.cptr[i + 1]; e++) {
        const double w = viol_of((P.cp[e] * xi + P.cq[e]) * xi + P.cr[e], P.crel[e]);
        v = w > v ? w : v;
    }
    return v;
}

// W = coordinates per lane (cd_small.h): lane l holds coordinate l in slot 0 and, in the wide kernels (W = 2), coordinate l + 64 in
// slot 1.  The value of coordinate i, broadcast: slot i >> 6 (wave-uniform) at lane i & 63.
template <int W>
__device__ inline double sm_bcast(const double (&v)[W], int i) {
    if constexpr (W == 1) return readlane_d(v[0], i);
    else return readlane_d((i >> 6) ? v[1] : v[0], i & 63);
}

// h (coordinate j) = sum_{k != j} P0[k][j] x_k in ascending k; returns f0(x) = sum_j (row_j + q_j) x_j + r0 in ascending j, row_j the
// same sum with the diagonal term.  x is zero in the slots whose coordinate is >= n.
template <int W>
__device__ inline double sm_refresh(const double *Ps, const double *qs, double r0, int n, int lane, const double (&x)[W], double (&h)[W]) {
    // slot 0 is written out and slot 1 added under if constexpr (no loop over the slots): the W = 1 kernels stay the code they were
    const int lc = lane < n ? lane : 0;
    const int lc1 = lane + 64 < n ? lane + 64 : 0;
    double row = 0.0, row1 = 0.0;
    h[0] = 0.0;
    if constexpr (W == 2) h[W - 1] = 0.0;
    for (int k = 0; k < n; k++) {
        const double xk = sm_bcast<W>(x, k);
        const double prod = Ps[k * n + lc] * xk;
        row += prod;
        h[0] = (k == lane) ? h[0] : h[0] + prod;
        if constexpr (W == 2) {
            const double prod1 = Ps[k * n + lc1] * xk;
            row1 += prod1;
            h[W - 1] = (k == lane + 64) ? h[W - 1] : h[W - 1] + prod1;
        }
    }
    double term[W];
    term[0] = (row + qs[lc]) * x[0];
    if constexpr (W == 2) term[W - 1] = (row1 + qs[lc1]) * x[W - 1];
    double acc = 0.0;
    for (int k = 0; k < n; k++) acc += sm_bcast<W>(term, k);
    return acc + r0;
}

// max violation of the point: a wave maximum of the own constraints of every coordinate the lanes hold
template <int W>
__device__ inline double sm_point_viol(const DevProblem &P, int n, int lane, const double (&x)[W]) {
    double v = -QM_INF;
#pragma unroll
    for (int s = 0; s < W; s++) {
        const int j = lane + 64 * s;
        if (j < n) {
            const double w = sm_coord_viol(P, j, x[s]);
            v = (s == 0 || w > v) ? w : v;
        }
    }
    return wave_max(v);
}

// a.P: the constraint lists the restart reads -- the context's, or the view of problem b's staged coefficients (cd_small_kernel).
// PC only names the caller: every kernel keeps an instance of its own, inlined as the single-caller function it was.  It is NOT marked
// always_inline (the mark costs a VGPR in two wide kernels): that no kernel calls it rests on the inliner; tools/asm_digest.py shows it.
template <int MAXC, bool PC, int W>
__device__ inline void sm_restart(const CdSmallArgs &a, const double *Ps, const double *qs, int64_t b, int64_t r, int lane) {
    const DevProblem &P = a.P;
    const int n = (int)P.n;
    const uint64_t seed = a.seed + (uint64_t)b * a.seed_stride;
    const uint64_t gr = a.first_index + (uint64_t)r;
    const int64_t o = b * a.R + r;
    const double r0 = a.r0s[b];
    bool on[W];
    int jc[W];
    double x[W];
    on[0] = lane < n;
    jc[0] = on[0] ? lane : 0;
    x[0] = 0.0;
    if (on[0]) x[0] = a.generate ? keyed_normal(seed, gr, (uint64_t)lane) : a.X0[o * n + lane];
    if constexpr (W == 2) {      // the keyed draws go by the coordinate, not the lane
        on[W - 1] = lane + 64 < n;
        jc[W - 1] = on[W - 1] ? lane + 64 : 0;
        x[W - 1] = 0.0;
        if (on[W - 1]) x[W - 1] = a.generate ? keyed_normal(seed, gr, (uint64_t)(lane + 64)) : a.X0[o * n + lane + 64];
    }

    // ---- phase 1 (qcqp.py:101-149): the loop of cd_phase1_sep_kernel for one restart; a lane visits the coordinates it holds
    int64_t sweeps1 = 0;
    int st1 = 0;
    if (a.phase1) {
        int my_status[W];
#pragma unroll
        for (int s = 0; s < W; s++) my_status[s] = 0;
        bool fin = false;
        for (int64_t t = 0; t < a.num_iters && !fin; t++) {
            sweeps1++;
            double vmax = -QM_INF;
            bool upd = false;
#pragma nounroll
            for (int s = 0; s < W; s++) {      // one copy of the visit's code: the slot is picked with selects
                const bool live = (W == 1 || s == 0) ? on[0] : on[W - 1];
                if (live) {
                    double xi = (W == 1 || s == 0) ? x[0] : x[W - 1];
                    P1Visit V;
                    p1_sep_visit<MAXC>(P, lane + 64 * s, xi, a.tol, a.viol_tol, seed, gr, t, V);
                    if (V.status) { if (W == 1 || s == 0) my_status[0] = V.status; else my_status[W - 1] = V.status; }
                    if (V.visited) {
                        if (V.moved) { if (W == 1 || s == 0) x[0] = xi; else x[W - 1] = xi; upd = true; }
                        vmax = (s == 0 || !(V.vafter <= vmax)) ? V.vafter : vmax;
                    }
                }
            }
            const double v = wave_max(vmax);
            const bool u = __builtin_amdgcn_ballot_w64(upd) != 0ull;
            // done when feasible enough (qcqp.py:111); a sweep without an update is a fixed point
            fin = v < a.viol_tol || !u;
        }
        // the highest coordinate's, like the serial kernel: a coordinate of slot 1 lies above every coordinate of slot 0
#pragma unroll
        for (int s = W - 1; s >= 0; s--) {
            const unsigned long long bad = __builtin_amdgcn_ballot_w64(my_status[s] != 0);
            if (bad && st1 == 0) st1 = __builtin_amdgcn_readlane(my_status[s], 63 - __builtin_clzll(bad));
        }
    }

    // ---- gate (qcqp.py:189); the max violation is also the slack phase 2 fixes (qcqp.py:157)
    const double slack = sm_point_viol<W>(P, n, lane, x);
    const bool ran2 = st1 == 0 && slack < a.viol_tol;

    // ---- phase 2 (qcqp.py:152-178)
    ChainState S;
    S.fcur = 0.0; S.upd_counter = 0; S.visits = 0; S.accepted = 0; S.sweeps = 0; S.conv = !ran2; S.status = 0;
    if (ran2) {
        // the feasible sets at the fixed slack: in registers, one per slot -- except in the wide kernels with up to four constraints
        // per coordinate, where two FeasSet<4> do not fit beside the visit: those recompute coordinate i's set at its visit (the same
        // inputs through the same code: the same bits)
        constexpr bool KEEP = W == 1 || MAXC <= 1;
        FeasSet<MAXC> Cm[KEEP ? W : 1];
        double dg[W], ql[W];
        if constexpr (KEEP) {
            Cm[0].n = 0;
#pragma unroll
            for (int j = 0; j <= MAXC; j++) { Cm[0].lo[j] = 0.0; Cm[0].hi[j] = 0.0; }
            if (on[0]) compute_set<MAXC>(P, lane, slack, Cm[0]);
        }
        dg[0] = Ps[jc[0] * n + jc[0]]; ql[0] = qs[jc[0]];
        if constexpr (W == 2) {
            if constexpr (KEEP) {
                Cm[W - 1].n = 0;
#pragma unroll
                for (int j = 0; j <= MAXC; j++) { Cm[W - 1].lo[j] = 0.0; Cm[W - 1].hi[j] = 0.0; }
                if (on[W - 1]) compute_set<MAXC>(P, lane + 64, slack, Cm[W - 1]);
            }
            dg[W - 1] = Ps[jc[W - 1] * n + jc[W - 1]]; ql[W - 1] = qs[jc[W - 1]];
        }
        for (int64_t t = 0; t < a.num_iters && !S.conv; t++) {
            S.sweeps++;
            double h[W];
            S.fcur = sm_refresh<W>(Ps, qs, r0, n, lane, x, h);
            for (int i = 0; i < n; i++) {
                const double xi = sm_bcast<W>(x, i), t2 = sm_bcast<W>(dg, i);
                const double t1 = 2.0 * sm_bcast<W>(h, i) + sm_bcast<W>(ql, i);
                const double t0 = S.fcur - xi * (t2 * xi + t1);
                FeasSet<MAXC> C;
                if constexpr (!KEEP) {
                    compute_set<MAXC>(P, i, slack, C);
                } else if constexpr (W == 1) {
                    C.n = __builtin_amdgcn_readlane(Cm[0].n, i);
#pragma unroll
                    for (int j = 0; j <= MAXC; j++) { C.lo[j] = readlane_d(Cm[0].lo[j], i); C.hi[j] = readlane_d(Cm[0].hi[j], i); }
                } else {
                    const bool hi = (i >> 6) != 0;
                    C.n = __builtin_amdgcn_readlane(hi ? Cm[W - 1].n : Cm[0].n, i & 63);
#pragma unroll
                    for (int j = 0; j <= MAXC; j++) {
                        C.lo[j] = readlane_d(hi ? Cm[W - 1].lo[j] : Cm[0].lo[j], i & 63);
                        C.hi[j] = readlane_d(hi ? Cm[W - 1].hi[j] : Cm[0].hi[j], i & 63);
                    }
                }
                DrawKey dk{seed, gr, (uint32_t)i, (uint32_t)t | 0x80000000u, 0u};
                double xn = xi;
                const int got = onevar_minimise<MAXC>(t2, t1, t0, C, dk, &xn);
                bool moved;
                double delta;
                chain_commit<MAXC>(S, got, xn, xi, t2, t1, t0, a.tol, n, moved, delta);
                if (moved) {      // rank-one update along column i (= row i of the symmetric image)
#pragma unroll
                    for (int s = 0; s < W; s++) {
                        const double pij = Ps[i * n + jc[s]];
                        h[s] = (lane + 64 * s == i) ? h[s] : h[s] + pij * delta;
                        x[s] = (lane + 64 * s == i) ? xn : x[s];
                    }
                }
                if (S.conv) break;
            }
        }
    }

    // ---- results: objective and max violation of the final point; a restart on which the reference raises never wins
    double hh[W];
    double f = sm_refresh<W>(Ps, qs, r0, n, lane, x, hh);
    double mv = sm_point_viol<W>(P, n, lane, x);
    if (st1 != 0 || S.status != 0) { f = QM_INF; mv = QM_INF; }
    if (lane == 0) {
        a.sweeps1[o] = sweeps1; a.sweeps2[o] = S.sweeps; a.visits2[o] = S.visits; a.accepted2[o] = S.accepted;
        a.ran2[o] = ran2 ? 1 : 0;
        a.status1[o] = st1; a.status2[o] = S.status;
        a.f0[o] = f; a.maxviol[o] = mv;
    }
    if (on[0]) a.X[o * n + lane] = x[0];
    if constexpr (W == 2) {
        if (on[W - 1]) a.X[o * n + lane + 64] = x[W - 1];
    }
}

}  // namespace
}  // namespace qcqpmi
