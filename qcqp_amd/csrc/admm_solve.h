// The projection of consensus ADMM on a reduced basis (utilities.py:149-196) and the arguments it reads: the part of admm.h that
// admm_small_kernel (admm_small.hip) shares with the population kernels.  admm.h defines kernels that are not templates, so only
// one translation unit may include it; this header holds nothing but inline device functions and a plain structure.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "onevar.h"

namespace qcqpmi {

struct AdmmArgs {
    int64_t n, m, R;
    int64_t rows_k;       // hat rows per constraint (n or rp)
    int64_t Mh16;         // m * rows_k padded to a multiple of 16
    const double *lam;    // [m][rows_k] eigenvalues (numpy eigh order / basis order)
    const double *qhat;   // [m][rows_k] B_k^T q_k
    const double *rk;     // [m]
    const int *relop;     // [m]
    const double *slo;    // [m] bracket start  max_{lam>0} -1/lam  (or -inf)
    const double *ehi;    // [m] bracket end    min_{lam<0} -1/lam  (or +inf)
    double *ZQ;           // in: B_k^T z ; out: the operand of the consensus product
    double *UH;           // in/out: dual in the basis
    const uint8_t *act;   // [R] restart still iterating
    unsigned long long *mvbits;  // [R] max violation of z over the constraints, as ordered bits
    int first_iter;       // 1: xs = x0, us = 0: the duals are zero and UH is not read
    int viol_only;        // 1: only the violations of z are wanted (no update)
    int lowrank;          // 1: reduced basis (operand 2 xhat - vhat - zq, dual vhat - xhat)
    int project_only;     // 1: unit operator onecons_qcqp: out = xhat (no dual, no update)
    double sec_tol;       // 1e-6 (utilities.py:149)
    int zq_planes;        // ZQ arrives as this many split-K partial planes (small kernel only; summed in a fixed order)
    int64_t zq_plane;     // doubles between two planes
    int no_shortcut;      // 1: every step of the bisection evaluates the secular function (cross-check of the one-row shortcut)
};

// num / den through the hardware reciprocal + two Newton steps (relative error ~1e-16; the exact IEEE division
// expands to ~30 instructions and the secular function costs 16 of them per lane and bisection step).  The
// multiplier is only located to 1e-6 (utilities.py:149), so last-bit differences of phi are immaterial.
__device__ inline double admm_div(double num, double den) {
    double r = __builtin_amdgcn_rcp(den);
    r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
    return num * r;
}

// The projection itself (utilities.py:165-196) on the RP coordinates of a reduced basis for one (constraint, restart) pair: v -> x.
// Shared by admm_secular_small_kernel and admm_unit_step_kernel: same expressions, same bits.
template <int RP>
__device__ __attribute__((always_inline)) inline void admm_small_solve(const AdmmArgs &a, int64_t k, const double (&L)[RP], const double (&Qh)[RP],
                                                                       const double (&V)[RP], double rk, int relop, double fv, double (&X)[RP]) {
    if (relop == RELOP_LE && fv <= 0.0) {
#pragma unroll
        for (int e = 0; e < RP; e++) X[e] = V[e];
    } else {
        auto phi = [&](double nu) {
            double p = 0.0;
#pragma unroll
            for (int e = 0; e < RP; e++) {
                const double num = -(nu * Qh[e] - 2.0 * V[e]);
                const double xh = (L[e] != 0.0) ? admm_div(num, 2.0 * (1.0 + nu * L[e])) : num * 0.5;
                X[e] = xh;
                p += L[e] * (xh * xh) + Qh[e] * xh;
            }
            return p + rk;
        };
        // One row (RP == 1: a constraint on ONE coordinate): the secular function is scalar,
        //   phi(nu) = L x^2 + q x + r,  x = (2 v - nu q) / (2 (1 + nu L)),  phi' = -(2 L x + q)^2 / (2 (1 + nu L)) <= 0 on the bracket,
        // so its root nu* is known in closed form (x* = the root of the constraint's own quadratic on v's side, nu* = 2 (v - x*) /
        // (2 L x* + q)) and every comparison the reference's loops make (utilities.py:176-194: the doubling of the bracket, the
        // bisection to 1e-6) is decided by the SIDE of nu* the trial value lies on -- the same outcome, without evaluating phi --
        // unless the trial is so close to nu* that rounding could decide (then phi is evaluated like before).  ~25-60 evaluations with
        // a division each become ~1 per solve: this kernel was 38 % of an ADMM iteration on Boolean least squares at n = 1024.
        bool fast = false;
        double nus = 0.0, dphi = 0.0, scale = 0.0;
        if (RP == 1 && !a.no_shortcut) {
            const double l = L[0], qh = Qh[0], v = V[0];
            const double w = qh + 2.0 * l * v;                 // sign of (1 + nu L) (2 L x + q): picks the root on the bracket's branch
            double xs = 0.0;
            bool ok = false;
            if (l != 0.0) {
                const double disc = qh * qh - 4.0 * l * rk;
                if (disc > 0.0 && w != 0.0) {
                    const double sq = sqrt(disc);
                    xs = (w > 0.0) ? (-qh + sq) / (2.0 * l) : (-qh - sq) / (2.0 * l);
                    ok = true;
                }
            } else if (qh != 0.0) { xs = -rk / qh; ok = true; }
            if (ok) {
                const double den = 2.0 * l * xs + qh;
                nus = 2.0 * (v - xs) / den;
                const double onel = 1.0 + nus * l;
                dphi = -(den * den) / (2.0 * onel);
                scale = fabs(l) * xs * xs + fabs(qh * xs) + fabs(rk);
                fast = den != 0.0 && onel > 0.0 && nus - nus == 0.0 && dphi - dphi == 0.0;
            }
        }
        // The sign of phi at a trial value: by the SIDE of nu* unless the trial is too close to tell (then phi is evaluated).  Written
        // straight-line -- `up` / `dn` are plain compares, phi sits behind ONE wave-uniform test (no lane of the wave near nu*: the common
        // case has nothing to skip over), the bracket moves by selects: with an early return per case a step was ten exec-mask regions
        // and 40 instructions, and the ~25 steps of a solve were what admm_unit_step_kernel spent its time ISSUING (a wave64 vector
        // instruction occupies its SIMD for 4 cycles whatever it does; round 6, profiles/r06_admm_unit_bases.md).  Same decisions, same
        // bits: |d| > c1 and |phi'(nu*) d| > c2  <=>  |d| > zone up to the rounding of c2 / |phi'| -- a trial THAT close to the zone's
        // edge has the sign of its side either way (the zone is 1e6 roundings wide).
        const double zone = fast ? fmax(1e-8 * (1.0 + fabs(nus)), 1e-10 * scale / fabs(dphi)) : QM_INF;
        bool pnan = false;                                     // phi was evaluated and is not a number (ends the doubling loops like the reference's comparisons do)
        auto psign = [&](double nu, bool &up, bool &dn) {
            const double d = nu - nus;
            const bool near = !(fabs(d) > zone);               // (also for a not-a-number trial)
            up = d < 0.0; dn = !up;
            if (__builtin_amdgcn_ballot_w64(near) != 0ull) {
                if (near) { const double p = phi(nu); up = p > 0.0; dn = p < 0.0; pnan = p != p; }
            }
        };
        double s = a.slo[k], e_ = a.ehi[k];
        int guard = 0;
        bool up, dn;
        if (s == -QM_INF) { s = -1.0; for (;;) { psign(s, up, dn); if (up || pnan || guard++ >= 2000) break; s *= 2.0; } }          // while phi(s) <= 0
        if (e_ == QM_INF) { e_ = 1.0; for (;;) { psign(e_, up, dn); if (dn || pnan || guard++ >= 4000) break; e_ *= 2.0; } }        // while phi(e) >= 0
        int steps = 0;
        while (e_ - s > a.sec_tol && steps++ < 100000) {
            const double mid = (s + e_) / 2.0;
            psign(mid, up, dn);
            // phi > 0: s = mid; phi < 0: e = mid; otherwise (zero, or not a number) both, which ends the loop (utilities.py:189-194)
            s = (up || !dn) ? mid : s;
            e_ = (dn || !up) ? mid : e_;
        }
        (void)phi((s + e_) / 2.0);
    }
}

}  // namespace qcqpmi
