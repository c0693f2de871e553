// One case of a unit operator, for every instantiation of the one-variable solver the coordinate-descent kernels run:
//   feasible_set<1|2|4> + onevar_minimise            (cd_phase2*.h, cd_life.hip MULTI, cd_small.hip)
//   feasible_set_single<1|2|4> + onevar_minimise     (cd_chain.h::compute_set, p1_sep_visit_core)
//   p1_sep_visit_core<1|4>, p1_band_visit, p1_band_visit_n<2, false|true>     (phase 1, cd_phase1_sep.h)
// The variant is a template argument: each instantiation is the straight-line code of that variant alone.  capi_units.hip runs one
// lane per case (qcqpmi_onevar_variant_batch, qcqpmi_p1_visit_batch); tests/host/onevar_selftest.cpp runs the same functions on
// the host, where <hip/hip_runtime.h> is a stub of empty qualifiers.  Layouts are those of qcqpmi_onevar_qcqp_batch.
#pragma once
#include <stdint.h>
#include "onevar.h"
#include "cd_phase1_sep.h"

namespace qcqpmi {

enum { UV_SWEEP4 = 0, UV_SWEEP2 = 1, UV_SWEEP1 = 2, UV_SINGLE4 = 3, UV_SINGLE2 = 4, UV_SINGLE1 = 5, UV_ONEVAR_VARIANTS = 6 };
enum { PV_CORE1 = 0, PV_CORE4 = 1, PV_BAND = 2, PV_BAND_N2 = 3, PV_BAND_N2_FASTA = 4, PV_VISIT_VARIANTS = 5 };
constexpr int UV_SLOTS = 4;       // constraint slots per case and, plus one, pieces per case in the layouts

constexpr int uv_maxc(int variant) {
    return (variant == UV_SWEEP4 || variant == UV_SINGLE4) ? 4 : (variant == UV_SWEEP2 || variant == UV_SINGLE2) ? 2 : 1;
}
constexpr bool uv_single(int variant) { return variant >= UV_SINGLE4; }
constexpr int pv_maxc(int variant) { return variant == PV_CORE4 ? 4 : 1; }

// the contract of a variant, checked by the host before anything is launched
inline bool uv_case_ok(int variant, int nf) { return nf >= 0 && nf <= uv_maxc(variant) && (!uv_single(variant) || nf == 1); }
inline bool pv_band_class(const double *con) { return con[1] == 0.0 && (int)con[3] == RELOP_EQ && con[0] > 1e-4; }
inline bool pv_case_ok(int variant, const double *cons /* 4 x (p, q, r, relop) */, int nf) {
    if (nf < 1 || nf > pv_maxc(variant)) return false;
    if (variant >= PV_BAND && !pv_band_class(cons)) return false;
    if (variant >= PV_BAND_N2 && !(cons[2] < -1e-3)) return false;
    return true;
}

template <int VARIANT>
__device__ inline void uv_onevar_case(int64_t i, const double *__restrict__ f0, const double *__restrict__ fs, const int *__restrict__ nf,
                                      const double *__restrict__ s, uint64_t seed, double *__restrict__ x, int *__restrict__ status,
                                      double *__restrict__ Cout, int *__restrict__ nC) {
    constexpr int MAXC = uv_maxc(VARIANT);
    double cp[MAXC], cq[MAXC], cr[MAXC];
    int crel[MAXC];
#pragma unroll
    for (int k = 0; k < MAXC; k++) {
        cp[k] = fs[(i * UV_SLOTS + k) * 4]; cq[k] = fs[(i * UV_SLOTS + k) * 4 + 1]; cr[k] = fs[(i * UV_SLOTS + k) * 4 + 2];
        crel[k] = (int)fs[(i * UV_SLOTS + k) * 4 + 3];
    }
    FeasSet<MAXC> C;
    if constexpr (uv_single(VARIANT)) feasible_set_single<MAXC>(cp[0], cq[0], cr[0], crel[0], s[i], C);
    else feasible_set<MAXC>(cp, cq, cr, crel, nf[i], s[i], C);
    DrawKey dk{seed, (uint64_t)i, 0u, 0u, 0u};
    double xn = QM_NAN;
    const int got = onevar_minimise<MAXC>(f0[3 * i], f0[3 * i + 1], f0[3 * i + 2], C, dk, &xn);
    x[i] = xn;
    status[i] = got;
    if (nC) nC[i] = C.n;
    if (Cout)
#pragma unroll
        for (int j = 0; j <= UV_SLOTS; j++) {      // pieces the variant cannot hold are NaN
            Cout[(i * (UV_SLOTS + 1) + j) * 2] = j <= MAXC ? C.lo[j <= MAXC ? j : 0] : QM_NAN;
            Cout[(i * (UV_SLOTS + 1) + j) * 2 + 1] = j <= MAXC ? C.hi[j <= MAXC ? j : 0] : QM_NAN;
        }
}

// true where case j is a band case with the (p, r) of case i: the two can share a fused visit
__device__ inline bool pv_same_band(const double *__restrict__ cons, const int *__restrict__ nf, int64_t i, int64_t j) {
    const double *a = cons + i * UV_SLOTS * 4, *b = cons + j * UV_SLOTS * 4;
    return nf[j] == 1 && b[0] == a[0] && b[1] == 0.0 && b[2] == a[2] && (int)b[3] == RELOP_EQ;
}

// restart = case, coordinate 0.  The fused variants visit case i together with its neighbour i ^ 1 where that one shares (p, r),
// else with a padding element (on = false); an even case is element 0 of its pair, an odd one element 1.
template <int VARIANT>
__device__ inline void pv_visit_case(int64_t i, int64_t count, const double *__restrict__ cons, const int *__restrict__ nf,
                                     const double *__restrict__ xi, double tol, double viol_tol, uint64_t seed, int64_t sweep,
                                     double *__restrict__ x_out, int *__restrict__ moved, double *__restrict__ vafter,
                                     int *__restrict__ status) {
    constexpr int MAXC = pv_maxc(VARIANT);
    double cp[MAXC], cq[MAXC], cr[MAXC];
    int crel[MAXC];
#pragma unroll
    for (int k = 0; k < MAXC; k++) {
        cp[k] = cons[(i * UV_SLOTS + k) * 4]; cq[k] = cons[(i * UV_SLOTS + k) * 4 + 1]; cr[k] = cons[(i * UV_SLOTS + k) * 4 + 2];
        crel[k] = (int)cons[(i * UV_SLOTS + k) * 4 + 3];
    }
    double x = xi[i];
    P1Visit V;
    if constexpr (VARIANT == PV_CORE1 || VARIANT == PV_CORE4) {
        p1_sep_visit_core<MAXC>(nf[i], cp, cq, cr, crel, 0, x, tol, viol_tol, seed, (uint64_t)i, sweep, V);
    } else if constexpr (VARIANT == PV_BAND) {
        p1_band_visit(cp[0], cq[0], cr[0], 0, x, tol, viol_tol, seed, (uint64_t)i, sweep, V);
    } else {
        // the fused visit shares the restart between its elements: the neighbour is visited with this case's key, and only
        // this case's element is kept
        const int64_t j = i ^ 1;
        const bool pair = j < count && pv_same_band(cons, nf, i, j);
        const int me = (int)(i & 1);
        const int64_t ii[2] = {0, 0};
        const double xo = pair ? xi[j] : 0.0;
        double xx[2] = {me ? xo : x, me ? x : xo};
        const bool on[2] = {me ? pair : true, me ? true : pair};
        P1Visit VV[2];
        p1_band_visit_n<2, VARIANT == PV_BAND_N2_FASTA>(cp[0], cq[0], cr[0], ii, xx, on, tol, viol_tol, seed, (uint64_t)i, sweep, VV);
        x = me ? xx[1] : xx[0];
        V = me ? VV[1] : VV[0];
    }
    x_out[i] = x;
    moved[i] = V.moved ? 1 : 0;
    vafter[i] = V.vafter;
    status[i] = V.status;
}

}  // namespace qcqpmi
