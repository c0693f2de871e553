// as_restart / as_restart_w2 -- ONE restart of improve_admm by ONE wavefront on the LDS image of a small problem: the restart bodies of
// admm_small_kernel (admm_small.hip, whose header describes the layout) and of the ADMM stages of chain_small_kernel (chain_small.hip).
// Self-contained; everything here has internal linkage: a translation unit that includes it gets instances of its own.
#pragma once
#include "admm_small.h"    // AdmmSmallArgs

#include "admm_solve.h"    // admm_small_solve<1>, AdmmArgs
#include "cd_chain.h"      // readlane_d
#include "dev_util.h"
#include "philox.h"

namespace qcqpmi {
namespace {

// the constraints on a lane's coordinate, in entry order
template <int MAXC>
struct AsList {
    int cnt;
    double p[MAXC], q[MAXC], r[MAXC];
    int rel[MAXC];
};

// One entry of a projection pass of the WIDE kernels (as_project2): constraint (p, q, rk, relop) on a coordinate at z with dual uo --
// the statements of as_project's loop body, which keeps its text so that the kernels for n <= 64 keep their code.
// Returns the new dual; op = the operand 2 xhat - vhat - z; viol takes the entry's violation of z.
__device__ __attribute__((always_inline)) inline double as_entry(double p, double q, double rk, int relop, double uo, double z, bool first, double &op,
                                                                 double &viol) {
    double L[1], Qh[1], V[1], Zq[1], X[1];
    L[0] = p; Qh[0] = q;
    Zq[0] = z;
    uo = first ? 0.0 : uo;
    V[0] = Zq[0] + uo;
    double fz = 0.0, fv = 0.0;
    fz += L[0] * (Zq[0] * Zq[0]) + Qh[0] * Zq[0];
    fv += L[0] * (V[0] * V[0]) + Qh[0] * V[0];
    fz += rk; fv += rk;
    const double w = (relop == RELOP_EQ) ? fabs(fz) : (fz > 0.0 ? fz : 0.0);
    viol = w > viol ? w : viol;
    // the bracket of one row (admm_brackets, capi_admm.hip)
    double br[2];
    br[0] = L[0] > 0.0 ? -1.0 / L[0] : -QM_INF;
    br[1] = L[0] < 0.0 ? -1.0 / L[0] : QM_INF;
    AdmmArgs sa;
    sa.slo = &br[0]; sa.ehi = &br[1]; sa.sec_tol = 1e-6; sa.no_shortcut = 0;      // what admm_small_solve reads (utilities.py:149)
    admm_small_solve<1>(sa, 0, L, Qh, V, rk, relop, fv, X);
    op = 2.0 * X[0] - V[0] - Zq[0];
    return V[0] - X[0];
}

// One projection pass at z (the body of admm_unit_step_kernel with s_h = +1): the duals move, the sum of the operands is returned,
// viol = max violation of z over the coordinate's constraints (0 without one, like the zeroed mvbits of the serial kernels).
// ONE copy of the solve's code for the up to MAXC entries: the loop is not unrolled and the entry is picked with selects (with four
// inlined copies per call site the <4> kernels took 223 VGPRs: two waves per SIMD).
template <int MAXC>
__device__ inline double as_project(const AsList<MAXC> &K, double z, bool first, double (&u)[MAXC], double &viol) {
    double acc = 0.0;
    viol = 0.0;
#pragma nounroll
    for (int c = 0; c < K.cnt; c++) {
        double L[1], Qh[1], V[1], Zq[1], X[1];
        double rk = K.r[0], uo = u[0];
        int relop = K.rel[0];
        L[0] = K.p[0]; Qh[0] = K.q[0];
#pragma unroll
        for (int s = 1; s < MAXC; s++) {
            const bool pick = c == s;
            L[0] = pick ? K.p[s] : L[0]; Qh[0] = pick ? K.q[s] : Qh[0]; rk = pick ? K.r[s] : rk; relop = pick ? K.rel[s] : relop;
            uo = pick ? u[s] : uo;
        }
        Zq[0] = z;
        uo = first ? 0.0 : uo;
        V[0] = Zq[0] + uo;
        double fz = 0.0, fv = 0.0;
        fz += L[0] * (Zq[0] * Zq[0]) + Qh[0] * Zq[0];
        fv += L[0] * (V[0] * V[0]) + Qh[0] * V[0];
        fz += rk; fv += rk;
        const double w = (relop == RELOP_EQ) ? fabs(fz) : (fz > 0.0 ? fz : 0.0);
        viol = w > viol ? w : viol;
        // the bracket of one row (admm_brackets, capi_admm.hip)
        double br[2];
        br[0] = L[0] > 0.0 ? -1.0 / L[0] : -QM_INF;
        br[1] = L[0] < 0.0 ? -1.0 / L[0] : QM_INF;
        AdmmArgs sa;
        sa.slo = &br[0]; sa.ehi = &br[1]; sa.sec_tol = 1e-6; sa.no_shortcut = 0;      // what admm_small_solve reads (utilities.py:149)
        admm_small_solve<1>(sa, 0, L, Qh, V, rk, relop, fv, X);
        const double un = V[0] - X[0];
#pragma unroll
        for (int s = 0; s < MAXC; s++) u[s] = (c == s) ? un : u[s];
        acc += 2.0 * X[0] - V[0] - Zq[0];
    }
    return acc;
}

// The pass of a lane of the wide kernels: the entries of slot 0 (coordinate lane, at z0), then those of slot 1 (coordinate lane + 64, at
// z1), each slot in ascending entry order with a sum of its own.  STILL one copy of the solve: the slot is one more select in front of
// the same non-unrolled loop.  viol = max violation over both coordinates.
template <int MAXC>
__device__ inline void as_project2(const AsList<MAXC> &K0, const AsList<MAXC> &K1, double z0, double z1, bool first, double (&u0)[MAXC],
                                   double (&u1)[MAXC], double &viol, double &acc0, double &acc1) {
    acc0 = 0.0; acc1 = 0.0;
    viol = 0.0;
    const int total = K0.cnt + K1.cnt;
#pragma nounroll
    for (int t = 0; t < total; t++) {
        const bool hi = t >= K0.cnt;
        const int c = hi ? t - K0.cnt : t;
        double pk = hi ? K1.p[0] : K0.p[0], qk = hi ? K1.q[0] : K0.q[0], rk = hi ? K1.r[0] : K0.r[0], uo = hi ? u1[0] : u0[0];
        int relop = hi ? K1.rel[0] : K0.rel[0];
#pragma unroll
        for (int s = 1; s < MAXC; s++) {
            const bool p0 = !hi && c == s, p1 = hi && c == s;
            pk = p0 ? K0.p[s] : (p1 ? K1.p[s] : pk); qk = p0 ? K0.q[s] : (p1 ? K1.q[s] : qk); rk = p0 ? K0.r[s] : (p1 ? K1.r[s] : rk);
            relop = p0 ? K0.rel[s] : (p1 ? K1.rel[s] : relop);
            uo = p0 ? u0[s] : (p1 ? u1[s] : uo);
        }
        double op;
        const double un = as_entry(pk, qk, rk, relop, uo, hi ? z1 : z0, first, op, viol);
#pragma unroll
        for (int s = 0; s < MAXC; s++) { u0[s] = (!hi && c == s) ? un : u0[s]; u1[s] = (hi && c == s) ? un : u1[s]; }
        acc0 = hi ? acc0 : acc0 + op;
        acc1 = hi ? acc1 + op : acc1;
    }
}

// max violation of the lane's coordinate at z without a projection (the start)
template <int MAXC>
__device__ inline double as_viol(const AsList<MAXC> &K, double z) {
    double viol = 0.0;
#pragma unroll
    for (int c = 0; c < MAXC; c++) {
        if (c < K.cnt) {
            double fz = 0.0;
            fz += K.p[c] * (z * z) + K.q[c] * z;
            fz += K.r[c];
            const double w = (K.rel[c] == RELOP_EQ) ? fabs(fz) : (fz > 0.0 ? fz : 0.0);
            viol = w > viol ? w : viol;
        }
    }
    return viol;
}

// f0(x) = sum_j (row_j + q_j) x_j + r0, row_j = sum_k P0[k][j] x_k, both in ascending index order (the sums of sm_refresh, cd_small.hip);
// P0 from global memory (symmetric: column j as word k n + j), x zero in the lanes >= n
__device__ inline double as_f0(const double *__restrict__ Pg, const double *qs, double r0, int n, int lane, double x) {
    const int lc = lane < n ? lane : 0;
    double row = 0.0;
    for (int k = 0; k < n; k++) row += Pg[k * n + lc] * readlane_d(x, k);
    const double term = (row + qs[lc]) * x;
    double acc = 0.0;
    for (int k = 0; k < n; k++) acc += readlane_d(term, k);
    return acc + r0;
}

// the same for a point held two coordinates per lane (x0: coordinates 0..63, x1: 64..n-1, zero in the lanes past n): row_j in
// ascending k and the sum over j in ascending j ACROSS both slots -- slot 0's 64 terms, then slot 1's
__device__ inline double as_f0_w2(const double *__restrict__ Pg, const double *qs, double r0, int n, int lane, double x0, double x1) {
    const int l0 = lane < n ? lane : 0, l1 = lane + 64 < n ? lane + 64 : 0;
    const int n0 = n < 64 ? n : 64;
    double row0 = 0.0, row1 = 0.0;
    for (int k = 0; k < n0; k++) { const double xk = readlane_d(x0, k); row0 += Pg[k * n + l0] * xk; row1 += Pg[k * n + l1] * xk; }
    for (int k = 64; k < n; k++) { const double xk = readlane_d(x1, k - 64); row0 += Pg[k * n + l0] * xk; row1 += Pg[k * n + l1] * xk; }
    const double term0 = (row0 + qs[l0]) * x0, term1 = (row1 + qs[l1]) * x1;
    double acc = 0.0;
    for (int k = 0; k < n0; k++) acc += readlane_d(term0, k);
    for (int k = 64; k < n; k++) acc += readlane_d(term1, k - 64);
    return acc + r0;
}

// does QCQPForm.better return its FIRST argument?  (utilities.py:135-146; admm_book_kernel)
__device__ inline bool as_better_first(double f1, double v1, double f2, double v2) {
    const long long b1 = (long long)(v1 / 1e-4), b2 = (long long)(v2 / 1e-4);
    return b1 < b2 || (b1 == b2 && f1 < f2);
}

// NOT marked always_inline, like sm_restart (cd_small.hip): that no kernel calls it rests on the inliner; tools/asm_digest.py shows it.
template <int MAXC>
__device__ inline void as_restart(const AdmmSmallArgs &a, const double *Ms, const double *qs, int64_t b, int64_t r, int lane) {
    const DevProblem &P = a.P;
    const int n = (int)P.n;
    const bool on = lane < n;
    const int lc = on ? lane : 0;
    const uint64_t seed = a.seed + (uint64_t)b * a.seed_stride;
    const uint64_t gr = a.first_index + (uint64_t)r;
    const int64_t o = b * a.R + r;
    const double r0 = a.r0s[b], rho = a.rhos[b], mm = (double)P.m, rho_m = rho * mm;
    const double *Pg = a.P0s + b * n * n;
    const double ql = qs[lc];

    AsList<MAXC> K;
    K.cnt = 0;
#pragma unroll
    for (int c = 0; c < MAXC; c++) { K.p[c] = 0.0; K.q[c] = 0.0; K.r[c] = 0.0; K.rel[c] = RELOP_LE; }
    if (on) {
        const int e0 = P.cptr[lane], e1 = P.cptr[lane + 1];
        K.cnt = e1 - e0 < MAXC ? e1 - e0 : MAXC;
#pragma unroll
        for (int c = 0; c < MAXC; c++)
            if (c < K.cnt) { K.p[c] = P.cp[e0 + c]; K.q[c] = P.cq[e0 + c]; K.r[c] = P.cr[e0 + c]; K.rel[c] = P.crel[e0 + c]; }
    }
    double u[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; c++) u[c] = 0.0;

    double x0 = 0.0;
    if (on) x0 = a.generate ? keyed_normal(seed, gr, (uint64_t)lane) : a.X0[o * n + lane];
    const double mv0 = wave_max(as_viol<MAXC>(K, x0));
    const double f_x0 = as_f0(Pg, qs, r0, n, lane, x0);

    // ---- phase 1 (qcqp.py:195-212; orc_admm_phase1), x1 = better(x0, z1) (qcqp.py:281), phase 2 (qcqp.py:215-251; orc_admm_phase2).
    // The two phases are ONE loop nest, so that the projection is inlined once: a phase is its z-update, the projections they share
    // and its exits.
    double x1 = x0, f1 = f_x0, mv1 = mv0;
    double best = x0, bf = f_x0, bmv = mv0;
    int64_t it1 = 0, it2 = 0;
    bool took = false;
    for (int ph = a.phase1 ? 1 : 2; ph <= 2; ph++) {
        double z = x1, last = x1, mvz = mv1, acc = 0.0;       // (phase 1 starts from x1 = x0)
        bool have_last = false;
        for (int64_t t = 0; t < a.num_iters; t++) {
            double f0z = 0.0;
            if (ph == 1) {
                if (mvz < a.tol) break;                        // qcqp.py:203
                double sm = acc;
                sm += mm * z;
                z = on ? sm / mm : 0.0;                        // qcqp.py:205
                it1++;
            } else {
                it2++;
                double sm = acc;
                sm += mm * z;
                const double rhs = on ? 2.0 * rho * sm - ql : 0.0;      // qcqp.py:231
                double zn = 0.0;
                for (int k = 0; k < n; k++) zn += Ms[k * n + lc] * readlane_d(rhs, k);
                z = on ? zn : 0.0;
                // f0(z) from the solve's own right-hand side (admm_take_z_kernel)
                f0z = wave_sum_tree(((0.5 * rhs - rho_m * z) + ql) * z) + r0;
            }
            double vl;
            acc = as_project<MAXC>(K, z, t == 0, u, vl);
            mvz = wave_max(vl);
            if (ph == 2) {
                if (have_last) {
                    const double d = last - z;
                    if (sqrt(wave_sum_tree(d * d)) < a.tol) break;      // qcqp.py:241-242 (before bestx)
                }
                last = z; have_last = true;
                if (mvz > a.viol_lim) break;                             // qcqp.py:248
                if (as_better_first(f0z, mvz, bf, bmv)) { best = z; bf = f0z; bmv = mvz; took = true; }
            }
        }
        if (ph == 1) {
            if (it1 > 0) {                                     // (no iteration: z1 is x0 itself and `better` keeps its second argument)
                const double f_z = as_f0(Pg, qs, r0, n, lane, z);
                if (!as_better_first(f_x0, mv0, f_z, mvz)) { x1 = z; f1 = f_z; mv1 = mvz; }
            }
            best = x1; bf = f1; bmv = mv1;                     // bestx = x1 (qcqp.py:218)
        }
    }
    // ---- x2 = better(x1, bestx) (qcqp.py:284); what is compared and reported is f0 of the best point through P0 itself
    if (took) {
        bf = as_f0(Pg, qs, r0, n, lane, best);
        if (as_better_first(f1, mv1, bf, bmv)) { best = x1; bf = f1; bmv = mv1; }
    }
    if (lane == 0) { a.iters1[o] = it1; a.iters2[o] = it2; a.f0[o] = bf; a.maxviol[o] = bmv; }
    if (on) a.X[o * n + lane] = best;
}

// The restart of the wide kernels (64 < n <= 128): lane l holds coordinate l in slot 0 and coordinate l + 64 in slot 1 (live where
// l + 64 < n; slot 0 is always live).  The body is as_restart's statement for statement with slot 1 (names ending in b: its z, S, last,
// best, x1, duals and list) beside slot 0.  A function of its own and not a parameter of as_restart: with the slot-1 statements under
// `if constexpr` in ONE function the <MAXC[,pc]> kernels came out with other registers and another schedule (same counts; DESIGN.md
// 4.14), and they are to stay the code they were.  The cross-lane work takes both slots in ONE fixed order that depends on n alone:
//   solve        z_j = sum_k Minv[k][j] rhs_k for k = 0 .. n-1 ascending, rhs_k from slot k >> 6 at lane k & 63, one accumulator per slot;
//   sums         the lane adds its two slots (slot 0 + slot 1; a dead slot holds 0), then wave_sum_tree over the lanes;
//   maximum      the larger of the lane's two slots, then wave_max;
//   f0 by P0_b   as_f0_w2: ascending k, ascending j across the slots.
template <int MAXC>
__device__ inline void as_restart_w2(const AdmmSmallArgs &a, const double *Ms, const double *qs, int64_t b, int64_t r, int lane) {
    const DevProblem &P = a.P;
    const int n = (int)P.n;
    const bool on = lane < n, onb = lane + 64 < n;
    const int lc = on ? lane : 0, lb = onb ? lane + 64 : 0;
    const uint64_t seed = a.seed + (uint64_t)b * a.seed_stride;
    const uint64_t gr = a.first_index + (uint64_t)r;
    const int64_t o = b * a.R + r;
    const double r0 = a.r0s[b], rho = a.rhos[b], mm = (double)P.m, rho_m = rho * mm;
    const double *Pg = a.P0s + b * n * n;
    const double ql = qs[lc], qb = qs[lb];

    AsList<MAXC> K, Kb;
    K.cnt = 0; Kb.cnt = 0;
    double u[MAXC], ub[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; c++) {
        K.p[c] = 0.0; K.q[c] = 0.0; K.r[c] = 0.0; K.rel[c] = RELOP_LE; u[c] = 0.0;
        Kb.p[c] = 0.0; Kb.q[c] = 0.0; Kb.r[c] = 0.0; Kb.rel[c] = RELOP_LE; ub[c] = 0.0;
    }
    if (on) {
        const int e0 = P.cptr[lc], e1 = P.cptr[lc + 1];
        K.cnt = e1 - e0 < MAXC ? e1 - e0 : MAXC;
#pragma unroll
        for (int c = 0; c < MAXC; c++)
            if (c < K.cnt) { K.p[c] = P.cp[e0 + c]; K.q[c] = P.cq[e0 + c]; K.r[c] = P.cr[e0 + c]; K.rel[c] = P.crel[e0 + c]; }
    }
    if (onb) {
        const int e0 = P.cptr[lb], e1 = P.cptr[lb + 1];
        Kb.cnt = e1 - e0 < MAXC ? e1 - e0 : MAXC;
#pragma unroll
        for (int c = 0; c < MAXC; c++)
            if (c < Kb.cnt) { Kb.p[c] = P.cp[e0 + c]; Kb.q[c] = P.cq[e0 + c]; Kb.r[c] = P.cr[e0 + c]; Kb.rel[c] = P.crel[e0 + c]; }
    }

    double x0 = 0.0, x0b = 0.0;      // keyed by the COORDINATE, not the lane
    if (on) x0 = a.generate ? keyed_normal(seed, gr, (uint64_t)lc) : a.X0[o * n + lc];
    if (onb) x0b = a.generate ? keyed_normal(seed, gr, (uint64_t)lb) : a.X0[o * n + lb];
    const double va = as_viol<MAXC>(K, x0), vb = as_viol<MAXC>(Kb, x0b);
    const double mv0 = wave_max(vb > va ? vb : va);
    const double f_x0 = as_f0_w2(Pg, qs, r0, n, lane, x0, x0b);

    double x1 = x0, x1b = x0b, f1 = f_x0, mv1 = mv0;
    double best = x0, bestb = x0b, bf = f_x0, bmv = mv0;
    int64_t it1 = 0, it2 = 0;
    bool took = false;
    for (int ph = a.phase1 ? 1 : 2; ph <= 2; ph++) {
        double z = x1, zb = x1b, last = x1, lastb = x1b, mvz = mv1, acc = 0.0, accb = 0.0;
        bool have_last = false;
        for (int64_t t = 0; t < a.num_iters; t++) {
            double f0z = 0.0;
            double sm = acc, smb = accb;
            sm += mm * z; smb += mm * zb;
            if (ph == 1) {
                if (mvz < a.tol) break;
                z = on ? sm / mm : 0.0;
                zb = onb ? smb / mm : 0.0;
                it1++;
            } else {
                it2++;
                const double rhs = on ? 2.0 * rho * sm - ql : 0.0, rhsb = onb ? 2.0 * rho * smb - qb : 0.0;
                double zn = 0.0, znb = 0.0;
                const int n0 = n < 64 ? n : 64;
                for (int k = 0; k < n0; k++) { const double rk = readlane_d(rhs, k); zn += Ms[k * n + lc] * rk; znb += Ms[k * n + lb] * rk; }
                for (int k = 64; k < n; k++) { const double rk = readlane_d(rhsb, k - 64); zn += Ms[k * n + lc] * rk; znb += Ms[k * n + lb] * rk; }
                z = on ? zn : 0.0;
                zb = onb ? znb : 0.0;
                f0z = wave_sum_tree(((0.5 * rhs - rho_m * z) + ql) * z + ((0.5 * rhsb - rho_m * zb) + qb) * zb) + r0;
            }
            double vl;
            as_project2<MAXC>(K, Kb, z, zb, t == 0, u, ub, vl, acc, accb);
            mvz = wave_max(vl);
            if (ph == 2) {
                if (have_last) {
                    const double d = last - z, db = lastb - zb;
                    if (sqrt(wave_sum_tree(d * d + db * db)) < a.tol) break;
                }
                last = z; lastb = zb; have_last = true;
                if (mvz > a.viol_lim) break;
                if (as_better_first(f0z, mvz, bf, bmv)) { best = z; bestb = zb; bf = f0z; bmv = mvz; took = true; }
            }
        }
        if (ph == 1) {
            if (it1 > 0) {
                const double f_z = as_f0_w2(Pg, qs, r0, n, lane, z, zb);
                if (!as_better_first(f_x0, mv0, f_z, mvz)) { x1 = z; x1b = zb; f1 = f_z; mv1 = mvz; }
            }
            best = x1; bestb = x1b; bf = f1; bmv = mv1;
        }
    }
    if (took) {
        bf = as_f0_w2(Pg, qs, r0, n, lane, best, bestb);
        if (as_better_first(f1, mv1, bf, bmv)) { best = x1; bestb = x1b; bf = f1; bmv = mv1; }
    }
    if (lane == 0) { a.iters1[o] = it1; a.iters2[o] = it2; a.f0[o] = bf; a.maxviol[o] = bmv; }
    if (on) a.X[o * n + lc] = best;
    if (onb) a.X[o * n + lb] = bestb;
}

}  // namespace
}  // namespace qcqpmi
