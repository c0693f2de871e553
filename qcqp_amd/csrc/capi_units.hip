// Unit operators of the C ABI: the reference's module-level helpers
// get_feasible_intervals (utilities.py:198-232) and onevar_qcqp (utilities.py:241-288) evaluated ON THE
// DEVICE for a batch of independent cases, by exactly the device functions the coordinate-descent
// kernels inline (onevar.h).  They exist so that the golden vectors captured from the reference for
// these two functions (tests/golden/g3_intervals, g4_onevar_qcqp) are checked against the GPU code
// itself and not only through whole trajectories.
#include "capi_ctx.h"
#include "onevar.h"
#include "unit_variants.h"   // one case of every instantiation the kernels run: sweep / single at 1, 2, 4 slots, the phase-1 visits
#include "cd_general.h"      // gen_onevar_t2t1, gen_onevar_t0: the two device functions only, no kernel of it is instantiated here

using namespace qcqpmi;

namespace {

__global__ void unit_intervals_kernel(int64_t count, const double *__restrict__ pqrs, const int *__restrict__ relop,
                                      double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const Seg2 iv = feasible_intervals(pqrs[4 * i], pqrs[4 * i + 1], pqrs[4 * i + 2], relop[i], pqrs[4 * i + 3]);
    out[5 * i] = (double)iv.n;
    out[5 * i + 1] = iv.lo0; out[5 * i + 2] = iv.hi0; out[5 * i + 3] = iv.lo1; out[5 * i + 4] = iv.hi1;
}

constexpr int UNIT_MAXC = 4;

__global__ void unit_onevar_kernel(int64_t count, const double *__restrict__ f0, const double *__restrict__ fs,
                                   const int *__restrict__ nf, const double *__restrict__ s, uint64_t seed,
                                   double *__restrict__ x, int *__restrict__ status, double *__restrict__ Cout,
                                   int *__restrict__ nC) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double cp[UNIT_MAXC], cq[UNIT_MAXC], cr[UNIT_MAXC];
    int crel[UNIT_MAXC];
    const int mf = nf[i];
#pragma unroll
    for (int k = 0; k < UNIT_MAXC; k++) {
        cp[k] = fs[(i * UNIT_MAXC + k) * 4]; cq[k] = fs[(i * UNIT_MAXC + k) * 4 + 1]; cr[k] = fs[(i * UNIT_MAXC + k) * 4 + 2];
        crel[k] = (int)fs[(i * UNIT_MAXC + k) * 4 + 3];
    }
    FeasSet<UNIT_MAXC> C;
    feasible_set<UNIT_MAXC>(cp, cq, cr, crel, mf, s[i], C);
    DrawKey dk{seed, (uint64_t)i, 0u, 0u, 0u};
    double xn = QM_NAN;
    const int got = onevar_minimise<UNIT_MAXC>(f0[3 * i], f0[3 * i + 1], f0[3 * i + 2], C, dk, &xn);
    x[i] = xn;
    status[i] = got;
    if (nC) nC[i] = C.n;
    if (Cout)
#pragma unroll
        for (int j = 0; j <= UNIT_MAXC; j++) { Cout[(i * (UNIT_MAXC + 1) + j) * 2] = C.lo[j]; Cout[(i * (UNIT_MAXC + 1) + j) * 2 + 1] = C.hi[j]; }
}

// onevar_qcqp by the instantiation VARIANT of the set builder + minimiser, and one phase-1 coordinate visit by the restatement
// VARIANT (unit_variants.h): one kernel per variant, chosen by the host, so that each is the straight-line code of that variant
template <int VARIANT>
__global__ void unit_onevar_variant_kernel(int64_t count, const double *__restrict__ f0, const double *__restrict__ fs,
                                           const int *__restrict__ nf, const double *__restrict__ s, uint64_t seed,
                                           double *__restrict__ x, int *__restrict__ status, double *__restrict__ Cout,
                                           int *__restrict__ nC) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uv_onevar_case<VARIANT>(i, f0, fs, nf, s, seed, x, status, Cout, nC);
}

template <int VARIANT>
__global__ void unit_p1_visit_kernel(int64_t count, const double *__restrict__ cons, const int *__restrict__ nf,
                                     const double *__restrict__ xi, double tol, double viol_tol, uint64_t seed, int64_t sweep,
                                     double *__restrict__ x_out, int *__restrict__ moved, double *__restrict__ vafter,
                                     int *__restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    pv_visit_case<VARIANT>(i, count, cons, nf, xi, tol, viol_tol, seed, sweep, x_out, moved, vafter, status);
}

// get_onevar_func (utilities.py:99-105) for every function of the problem at the coordinate coord[r] of restart r of the
// resident population, in the reference's summation order: the device functions of cd_general.h (the coordinate-descent
// kernel for coupled constraints inlines the same two) for the objective and for dense constraints; for constraints that
// touch one coordinate (the lists the separable kernels read) the one-entry matrix is written out.
__global__ void unit_onevar_coeffs_kernel(DevProblem P, const double *__restrict__ gP, const double *__restrict__ Xall, int64_t R,
                                          const int64_t *__restrict__ coord, double *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m1 = P.m + 1;
    if (t >= R * m1) return;
    const int64_t gr = t / m1;
    const int k = (int)(t % m1);
    const int r = (int)(gr & 15);
    const double *X = Xall + (gr >> 4) * P.n16 * 16;
    const int64_t i = coord[gr];
    double t2 = 0.0, t1 = 0.0, t0 = 0.0;
    if (k == 0 || !P.sep) {
        gen_onevar_t2t1(P, gP, X, r, i, k, &t2, &t1);
        t0 = gen_onevar_t0(P, gP, X, r, i, k);
    } else {
        // constraint k touches ONE coordinate c: P = p e_c e_c', q = q e_c
        for (int64_t c = 0; c < P.n; c++)
            for (int e = P.cptr[c]; e < P.cptr[c + 1]; e++)
                if (P.cidx[e] == k) {
                    if (c == i) { t2 = P.cp[e]; t1 = 2.0 * 0.0 + P.cq[e]; t0 = P.cr[e]; }
                    else { const double xc = X[c * 16 + r]; t2 = 0.0; t1 = 0.0; t0 = (P.cp[e] * xc + P.cq[e]) * xc + P.cr[e]; }
                }
    }
    out[3 * t] = t2; out[3 * t + 1] = t1; out[3 * t + 2] = t0;
}

// a scoped device buffer of one unit call: cnt elements, filled from src when there is one (the null stream: these calls have no context)
template <typename T>
hipError_t unit_up(DevBuf<T> &b, const T *src, size_t cnt) {
    hipError_t e = b.reserve(nullptr, cnt, false);
    if (e == hipSuccess && src) e = hipMemcpy(b.p, src, cnt * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

#define UNITCHK(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(nullptr, QCQPMI_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

}  // namespace

extern "C" {

int qcqpmi_onevar_coeffs(qcqpmi_ctx *c, const int64_t *coord, double *out) {
    int rc = check_ready(c, true);
    if (rc) return rc;
    if (!coord || !out) return fail(c, QCQPMI_EINVAL, "onevar_coeffs: coord / out missing");
    if (!c->sep && !c->d_gP)
        return fail(c, QCQPMI_EUNSUPPORTED, "onevar_coeffs needs the row-major constraint matrices (uploaded functions, m n^2 <= 2e9 entries)");
    for (int64_t r = 0; r < c->R; r++)
        if (coord[r] < 0 || coord[r] >= c->n) return fail(c, QCQPMI_EINVAL, "onevar_coeffs: coordinate %lld of restart %lld", (long long)coord[r], (long long)r);
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<int64_t> dcoord;
    DevBuf<double> dout;
    const size_t cnt = (size_t)c->R * (size_t)(c->m + 1) * 3;
    UNITCHK(unit_up(dcoord, coord, (size_t)c->R));
    UNITCHK(unit_up(dout, (const double *)nullptr, cnt));
    HIPCHK(c, spin_sync(c->stream));
    const int64_t tot = c->R * (c->m + 1);
    hipLaunchKernelGGL(unit_onevar_coeffs_kernel, dim3((unsigned)((tot + 127) / 128)), dim3(128), 0, c->stream, c->dp,
                       (const double *)c->d_gP, (const double *)c->X, c->R, (const int64_t *)dcoord.p, dout.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, spin_sync(c->stream));
    HIPCHK(c, hipMemcpy(out, dout.p, cnt * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int qcqpmi_feasible_intervals_batch(int device, int64_t count, const double *pqrs, const int *relop, double *out) {
    if (count <= 0 || !pqrs || !relop || !out) return fail(nullptr, QCQPMI_EINVAL, "feasible_intervals_batch: bad arguments");
    if (qcqpmi_device_count() <= 0) return fail(nullptr, QCQPMI_EHIP, "no HIP device visible (there is no CPU fallback)");
    UNITCHK(hipSetDevice(device));
    DevBuf<double> dp, dout;
    DevBuf<int> dr;
    UNITCHK(unit_up(dp, pqrs, (size_t)count * 4));
    UNITCHK(unit_up(dr, relop, (size_t)count));
    UNITCHK(unit_up(dout, (const double *)nullptr, (size_t)count * 5));
    hipLaunchKernelGGL(unit_intervals_kernel, dim3((unsigned)((count + 127) / 128)), dim3(128), 0, 0, count, dp.p, dr.p, dout.p);
    UNITCHK(hipGetLastError());
    UNITCHK(hipMemcpy(out, dout.p, (size_t)count * 5 * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int qcqpmi_onevar_qcqp_batch(int device, int64_t count, const double *f0, const double *fs, const int *nf, const double *s,
                             uint64_t seed, double *x, int *status, double *C_out, int *nC_out) {
    if (count <= 0 || !f0 || !fs || !nf || !s || !x || !status) return fail(nullptr, QCQPMI_EINVAL, "onevar_qcqp_batch: bad arguments");
    for (int64_t i = 0; i < count; i++)
        if (nf[i] < 0 || nf[i] > UNIT_MAXC) return fail(nullptr, QCQPMI_EUNSUPPORTED, "onevar_qcqp_batch: at most %d constraints per case", UNIT_MAXC);
    if (qcqpmi_device_count() <= 0) return fail(nullptr, QCQPMI_EHIP, "no HIP device visible (there is no CPU fallback)");
    UNITCHK(hipSetDevice(device));
    DevBuf<double> df0, dfs, ds, dx, dC;
    DevBuf<int> dnf, dst, dnC;
    UNITCHK(unit_up(df0, f0, (size_t)count * 3));
    UNITCHK(unit_up(dfs, fs, (size_t)count * UNIT_MAXC * 4));
    UNITCHK(unit_up(dnf, nf, (size_t)count));
    UNITCHK(unit_up(ds, s, (size_t)count));
    UNITCHK(unit_up(dx, (const double *)nullptr, (size_t)count));
    UNITCHK(unit_up(dst, (const int *)nullptr, (size_t)count));
    UNITCHK(unit_up(dC, (const double *)nullptr, (size_t)count * (UNIT_MAXC + 1) * 2));
    UNITCHK(unit_up(dnC, (const int *)nullptr, (size_t)count));
    hipLaunchKernelGGL(unit_onevar_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, 0, count, df0.p, dfs.p, dnf.p, ds.p, seed, dx.p,
                       dst.p, dC.p, dnC.p);
    UNITCHK(hipGetLastError());
    UNITCHK(hipMemcpy(x, dx.p, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
    UNITCHK(hipMemcpy(status, dst.p, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    if (C_out) UNITCHK(hipMemcpy(C_out, dC.p, (size_t)count * (UNIT_MAXC + 1) * 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (nC_out) UNITCHK(hipMemcpy(nC_out, dnC.p, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int qcqpmi_onevar_variant_batch(int device, int variant, int64_t count, const double *f0, const double *fs, const int *nf,
                                const double *s, uint64_t seed, double *x, int *status, double *C_out, int *nC_out) {
    if (count <= 0 || !f0 || !fs || !nf || !s || !x || !status) return fail(nullptr, QCQPMI_EINVAL, "onevar_variant_batch: bad arguments");
    if (variant < 0 || variant >= UV_ONEVAR_VARIANTS) return fail(nullptr, QCQPMI_EINVAL, "onevar_variant_batch: unknown variant %d", variant);
    for (int64_t i = 0; i < count; i++)
        if (!uv_case_ok(variant, nf[i]))
            return fail(nullptr, QCQPMI_EUNSUPPORTED, "onevar_variant_batch: case %lld has %d constraints, variant %d takes %s%d",
                        (long long)i, nf[i], variant, uv_single(variant) ? "exactly 1 of its " : "at most ", uv_maxc(variant));
    if (qcqpmi_device_count() <= 0) return fail(nullptr, QCQPMI_EHIP, "no HIP device visible (there is no CPU fallback)");
    UNITCHK(hipSetDevice(device));
    DevBuf<double> df0, dfs, ds, dx, dC;
    DevBuf<int> dnf, dst, dnC;
    UNITCHK(unit_up(df0, f0, (size_t)count * 3));
    UNITCHK(unit_up(dfs, fs, (size_t)count * UV_SLOTS * 4));
    UNITCHK(unit_up(dnf, nf, (size_t)count));
    UNITCHK(unit_up(ds, s, (size_t)count));
    UNITCHK(unit_up(dx, (const double *)nullptr, (size_t)count));
    UNITCHK(unit_up(dst, (const int *)nullptr, (size_t)count));
    UNITCHK(unit_up(dC, (const double *)nullptr, (size_t)count * (UV_SLOTS + 1) * 2));
    UNITCHK(unit_up(dnC, (const int *)nullptr, (size_t)count));
    const dim3 grid((unsigned)((count + 63) / 64)), block(64);
#define UV_LAUNCH(V)                                                                                                            \
    case V:                                                                                                                     \
        hipLaunchKernelGGL(unit_onevar_variant_kernel<V>, grid, block, 0, 0, count, df0.p, dfs.p, dnf.p, ds.p, seed, dx.p, dst.p, dC.p, \
                           dnC.p);                                                                                              \
        break;
    switch (variant) {
        UV_LAUNCH(UV_SWEEP4) UV_LAUNCH(UV_SWEEP2) UV_LAUNCH(UV_SWEEP1) UV_LAUNCH(UV_SINGLE4) UV_LAUNCH(UV_SINGLE2) UV_LAUNCH(UV_SINGLE1)
    }
#undef UV_LAUNCH
    UNITCHK(hipGetLastError());
    UNITCHK(hipMemcpy(x, dx.p, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
    UNITCHK(hipMemcpy(status, dst.p, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    if (C_out) UNITCHK(hipMemcpy(C_out, dC.p, (size_t)count * (UV_SLOTS + 1) * 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (nC_out) UNITCHK(hipMemcpy(nC_out, dnC.p, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int qcqpmi_p1_visit_batch(int device, int variant, int64_t count, const double *cons, const int *nf, const double *xi, double tol,
                          double viol_tol, uint64_t seed, int64_t sweep, double *x_out, int *moved, double *vafter, int *status) {
    if (count <= 0 || !cons || !nf || !xi || !x_out || !moved || !vafter || !status)
        return fail(nullptr, QCQPMI_EINVAL, "p1_visit_batch: bad arguments");
    if (variant < 0 || variant >= PV_VISIT_VARIANTS) return fail(nullptr, QCQPMI_EINVAL, "p1_visit_batch: unknown variant %d", variant);
    for (int64_t i = 0; i < count; i++)
        if (!pv_case_ok(variant, cons + i * UV_SLOTS * 4, nf[i]))
            return fail(nullptr, QCQPMI_EUNSUPPORTED, "p1_visit_batch: case %lld (%d constraints) is outside the contract of variant %d",
                        (long long)i, nf[i], variant);
    if (qcqpmi_device_count() <= 0) return fail(nullptr, QCQPMI_EHIP, "no HIP device visible (there is no CPU fallback)");
    UNITCHK(hipSetDevice(device));
    DevBuf<double> dcons, dxi, dx, dva;
    DevBuf<int> dnf, dmv, dst;
    UNITCHK(unit_up(dcons, cons, (size_t)count * UV_SLOTS * 4));
    UNITCHK(unit_up(dnf, nf, (size_t)count));
    UNITCHK(unit_up(dxi, xi, (size_t)count));
    UNITCHK(unit_up(dx, (const double *)nullptr, (size_t)count));
    UNITCHK(unit_up(dva, (const double *)nullptr, (size_t)count));
    UNITCHK(unit_up(dmv, (const int *)nullptr, (size_t)count));
    UNITCHK(unit_up(dst, (const int *)nullptr, (size_t)count));
    const dim3 grid((unsigned)((count + 63) / 64)), block(64);
#define PV_LAUNCH(V)                                                                                                             \
    case V:                                                                                                                      \
        hipLaunchKernelGGL(unit_p1_visit_kernel<V>, grid, block, 0, 0, count, dcons.p, dnf.p, dxi.p, tol, viol_tol, seed, sweep, dx.p, \
                           dmv.p, dva.p, dst.p);                                                                                 \
        break;
    switch (variant) {
        PV_LAUNCH(PV_CORE1) PV_LAUNCH(PV_CORE4) PV_LAUNCH(PV_BAND) PV_LAUNCH(PV_BAND_N2) PV_LAUNCH(PV_BAND_N2_FASTA)
    }
#undef PV_LAUNCH
    UNITCHK(hipGetLastError());
    UNITCHK(hipMemcpy(x_out, dx.p, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
    UNITCHK(hipMemcpy(moved, dmv.p, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    UNITCHK(hipMemcpy(vafter, dva.p, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
    UNITCHK(hipMemcpy(status, dst.p, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
