// The bisection on the achievable slack of a phase-1 visit (qcqp.py:122-131) for the band class with r < -1e-3 (the Boolean family:
// one constraint p x^2 + r == 0 per coordinate), NV visits fused -- the loop of cd_phase1_sep.h::p1_band_visit_n, in a header that
// is also plain C++ (no HIP include; build the host side with -ffp-contract=off like the device side), so that a host program can
// drive it: tests/host/p1_bisect_selftest.cpp.
//
// State per element, as the visit sets it up: ss = -tol, es = viol - viol_tol (or -tol for padding), sp = 0, it = itp = 0,
// pending = false.  A step takes the midpoint s = (ss + es) / 2 and asks whether the slack s is achievable; for this class that is
// s > 0 unless s is within rounding (`guard`) of 0, where the discriminants are formed as the reference forms them.  Achievable:
// es = sp = s, itp = the step's index, pending; not achievable: ss = s.  Elements do not interact: fusing only shares the trip count.
//
// Phase A (QCQPMI_P1_FASTBISECT, default on): a visit starts far outside the band, so its first steps -- about log2(es / tol) of
// them, 17 for the slowest element of a wave at the headline -- all have s > guard and succeed.  During them ss stays, sp equals es,
// itp equals it - 1 and pending is it > 0: the loop carries es and a step count, nothing else.  An element leaves phase A at the first
// step whose condition fails, in exactly the state the general loop would have given it (same expressions, same order), and the
// general loop finishes every element: typically one or two steps, the test inside the guard among them.
// p1_band_bisect is what cd_life_prep_kernel runs (p1_band_visit_n<NV, true>); the build inside the lifecycle kernels and
// cd_queue.hip keep the general loop as p1_band_visit_n always had it, so that their code stays what it was, instruction for instruction.
#pragma once
#include <stdint.h>

#ifndef QCQPMI_P1_FASTBISECT
#define QCQPMI_P1_FASTBISECT 1
#endif

#if defined(__HIPCC__)
#define P1B_FN __host__ __device__ inline
#else
#define P1B_FN inline
#endif

namespace qcqpmi {

template <int NV>
P1B_FN void p1_band_bisect_general(double p, double r, double tol, double guard, double (&ss)[NV], double (&es)[NV], double (&sp)[NV],
                                   uint32_t (&it)[NV], uint32_t (&itp)[NV], bool (&pending)[NV]) {
    for (;;) {
        bool any = false;
#pragma unroll
        for (int k = 0; k < NV; k++) any = any || (es[k] - ss[k] > tol);
        if (!any) break;
#pragma unroll
        for (int k = 0; k < NV; k++) {
            const bool act = es[k] - ss[k] > tol;
            const double s = (ss[k] + es[k]) / 2.0;
            const uint32_t itb = it[k];
            it[k] += act ? 1u : 0u;
            bool nonempty = s > 0.0;
            if (__builtin_expect(act && !(__builtin_fabs(s) > guard), 0)) {       // within rounding of the threshold: the reference's discriminants
                const double D1 = 0.0 - 4.0 * p * (r - s);
                const double D2 = 0.0 - 4.0 * (-p) * (-r - s);
                nonempty = D1 > 0.0 && (D2 < 0.0 || D2 < D1);
            }
            const bool up = act && nonempty, dn = act && !nonempty;
            ss[k] = dn ? s : ss[k];
            es[k] = up ? s : es[k];
            sp[k] = up ? s : sp[k];
            itp[k] = up ? itb : itp[k];
            pending[k] = pending[k] || up;
        }
    }
}

// the steps every element takes while its midpoint stays above the guard (see the head of the file)
template <int NV>
P1B_FN void p1_band_bisect_phase_a(double tol, double guard, const double (&ss)[NV], double (&es)[NV], double (&sp)[NV], uint32_t (&it)[NV],
                                   uint32_t (&itp)[NV], bool (&pending)[NV]) {
    uint32_t na[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) na[k] = 0;
    for (;;) {
        bool any = false;
        bool go[NV];
        double s[NV];
#pragma unroll
        for (int k = 0; k < NV; k++) {
            s[k] = (ss[k] + es[k]) / 2.0;
            go[k] = es[k] - ss[k] > tol && s[k] > guard;
            any = any || go[k];
        }
        if (!any) break;
#pragma unroll
        for (int k = 0; k < NV; k++) {
            es[k] = go[k] ? s[k] : es[k];
            na[k] += go[k] ? 1u : 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < NV; k++)
        if (na[k]) { sp[k] = es[k]; itp[k] = it[k] + na[k] - 1u; it[k] += na[k]; pending[k] = true; }
}

template <int NV>
P1B_FN void p1_band_bisect(double p, double r, double tol, double (&ss)[NV], double (&es)[NV], double (&sp)[NV], uint32_t (&it)[NV],
                           uint32_t (&itp)[NV], bool (&pending)[NV]) {
    const double guard = 1e-9 * (1.0 - r);
#if QCQPMI_P1_FASTBISECT
    p1_band_bisect_phase_a<NV>(tol, guard, ss, es, sp, it, itp, pending);
#endif
    p1_band_bisect_general<NV>(p, r, tol, guard, ss, es, sp, it, itp, pending);
}

}  // namespace qcqpmi
