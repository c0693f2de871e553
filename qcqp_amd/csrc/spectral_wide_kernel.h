// spectral_wide_kernel -- suggest(SPECTRAL) for problems of 65 to 128 variables (any n <= 128 is computed correctly; the driver sends
// n <= 64 to the narrow kernel).  spectral_wide.h has the stages and the order of every sum.  Included by spectral_small.hip, the one
// unit that holds the spectral kernels and their launchers (the kernel sits in an unnamed namespace: a header for that unit alone).
//
// Layout.  ONE WAVEFRONT PER PROBLEM, one wavefront per workgroup.  LDS: G (n2 columns of n2 + 1 doubles: A_b, then Q_b) and five
// vectors of 128 (g, h then s, lam, w, x; w and x serve as the two row buffers of the Rayleigh quotients before they are needed).
// A lane holds the indices l and l + 64 (slot 0 and slot 1).
#pragma once

#include "dev_util.h"
#include "jacobi_wide.h"
#include "spectral_solve.h"
#include "spectral_wide.h"

namespace qcqpmi {
namespace {

constexpr int SPW_VECS = 5, SPW_VEC = 128;

__device__ inline double spw_sum(double v0, double v1) { return wave_sum_tree(v0 + v1); }
__device__ inline double spw_max(double v0, double v1) { return wave_max(v0 > v1 ? v0 : v1); }

__device__ inline void spw_problem(const SpectralSmallArgs &a, double *lds, int64_t b, int lane) {
    const int n = a.n, n2 = (n + 1) & ~1, str = jacobi_wide_stride(n2);
    double *G = lds, *gs = G + jacobi_wide_doubles(n2), *hs = gs + SPW_VEC, *lams = hs + SPW_VEC, *ws = lams + SPW_VEC, *xs = ws + SPW_VEC;
    const double *Pg = a.P0s + b * n * n, *qg = a.q0s + b * n, *ag = a.agg + b * a.agg_stride;
    const double inf = __builtin_huge_val();
    int idx[2], il[2];
    bool on[2];
    double ai[2], bi[2], si[2], qi[2];
    for (int h = 0; h < 2; h++) {
        idx[h] = lane + 64 * h;
        on[h] = idx[h] < n;
        il[h] = on[h] ? idx[h] : 0;
    }
    __syncthreads();             // the wave is done with the LDS image of its previous problem

    // ---- stage: s, h, then G = A_b = P0_b / (s_i s_j) with zero padding
    const double gamma = ag[2 * n];
    for (int h = 0; h < 2; h++) {
        ai[h] = ag[il[h]]; bi[h] = ag[n + il[h]]; qi[h] = qg[il[h]];
        si[h] = sqrt(ai[h]);
        gs[idx[h]] = on[h] ? si[h] : 1.0;    // (s for the staging; g below)
        hs[idx[h]] = on[h] ? bi[h] / (2.0 * ai[h]) : 0.0;
    }
    __syncthreads();
    bool asym = false;
    for (int i = 0; i < n2; i++) {
        for (int h = 0; h < 2; h++) {
            const int j = idx[h];
            if (j >= n2) continue;
            double v = 0.0;
            if (i < n && j < n) {
                const double p = Pg[i * n + j];
                asym = asym || (j >= i && !(p == Pg[j * n + i]));
                v = p / (gs[i] * gs[j]);
            }
            G[j * str + i] = v;
        }
    }
    if (asym) a.ticket[1] = 1;
    double ph[2] = {0.0, 0.0};
    for (int h = 0; h < 2; h++)
        if (on[h]) for (int j = 0; j < n; j++) ph[h] = __builtin_fma(Pg[j * n + idx[h]], hs[j], ph[h]);
    const double rho2 = spw_sum(on[0] ? bi[0] * bi[0] / (4.0 * ai[0]) : 0.0, on[1] ? bi[1] * bi[1] / (4.0 * ai[1]) : 0.0) - gamma;
    const double rho = sqrt(rho2);
    __syncthreads();             // every lane has read s and h
    for (int h = 0; h < 2; h++) {
        gs[idx[h]] = on[h] ? (0.5 * qi[h] - ph[h]) / si[h] : 0.0;
        hs[idx[h]] = on[h] ? si[h] : 1.0;    // (s again, for the Rayleigh quotients)
    }

    // ---- eigendecomposition: G becomes Q, column k = eigenvector k
    const JacobiWideResult jr = jacobi_wide(G, n2, str, lane, a.max_sweeps, a.tol);

    // ---- spectrum: lane = eigen-index
    double lamk[2] = {0.0, 0.0}, gh[2] = {0.0, 0.0};
    for (int i = 0; i < n; i++) {
        double *arow = (i & 1) ? xs : ws;
        for (int h = 0; h < 2; h++)
            if (on[h]) arow[idx[h]] = Pg[i * n + idx[h]] / (hs[i] * si[h]);
        __syncthreads();         // (one barrier per row: the buffer written next was read before the barrier of the row before)
        for (int h = 0; h < 2; h++) {
            if (!on[h]) continue;
            const double *u = G + idx[h] * str;
            double t = 0.0;
            for (int j = 0; j < n; j++) t = __builtin_fma(arow[j], u[j], t);
            lamk[h] = __builtin_fma(u[i], t, lamk[h]);
        }
    }
    for (int h = 0; h < 2; h++) {
        if (on[h]) for (int i = 0; i < n; i++) gh[h] = __builtin_fma(G[idx[h] * str + i], gs[i], gh[h]);
        lams[idx[h]] = on[h] ? lamk[h] : 0.0;
    }
    __syncthreads();
    int rank[2] = {0, 0};
    for (int j = 0; j < n; j++) {
        const double lj = lams[j];
        for (int h = 0; h < 2; h++) rank[h] += (lj < lamk[h] || (lj == lamk[h] && j < idx[h])) ? 1 : 0;
    }
    const double lam_min = -spw_max(on[0] ? -lamk[0] : -inf, on[1] ? -lamk[1] : -inf);
    const double lam_abs = spw_max(on[0] ? fabs(lamk[0]) : 0.0, on[1] ? fabs(lamk[1]) : 0.0);
    const unsigned long long first0 = __ballot(on[0] && rank[0] == 0), first1 = __ballot(on[1] && rank[1] == 0);
    int kmin = first0 ? __builtin_ctzll(first0) : 64 + __builtin_ctzll(first1 | (1ull << 63));
    kmin = kmin < n ? kmin : 0;      // (some lane always has rank 0; this keeps the read of column k_min inside G whatever happens)
    const double d[2] = {lamk[0] - lam_min, lamk[1] - lam_min};
    const double g2 = spw_sum(gh[0] * gh[0], gh[1] * gh[1]);

    // ---- branch
    int branch = 1;
    double w[2] = {0.0, 0.0}, sigma = 0.0, tau = 0.0, mu = 0.0;
    bool interior = false;
    if (!a.relop_eq && lam_min > 0.0) {
        for (int h = 0; h < 2; h++) w[h] = on[h] ? secular_w(gh[h], lamk[h]) : 0.0;
        interior = spw_sum(w[0] * w[0], w[1] * w[1]) <= rho2;
    }
    if (interior) {
        branch = 0;
        w[0] = -w[0]; w[1] = -w[1];
    } else {
        const double sigma_lo = (!a.relop_eq && lam_min > 0.0) ? lam_min : 0.0;
        int hard = 0;
        double wr[2] = {0.0, 0.0}, w0[2] = {0.0, 0.0}, gl[2] = {0.0, 0.0}, psi_reg = 0.0, psi0 = 0.0;
        if (sigma_lo == 0.0) {
            for (int h = 0; h < 2; h++) {
                const bool inL = d[h] <= SPECTRAL_HARD_THR * lam_abs;
                w0[h] = on[h] ? secular_w(gh[h], d[h]) : 0.0;
                wr[h] = inL ? 0.0 : w0[h];
                gl[h] = inL ? gh[h] * gh[h] : 0.0;
            }
            const double gL2 = spw_sum(gl[0], gl[1]);
            psi_reg = spw_sum(wr[0] * wr[0], wr[1] * wr[1]);
            psi0 = spw_sum(w0[0] * w0[0], w0[1] * w0[1]);
            hard = spectral_hard_case(gL2, g2, psi_reg, psi0, rho2);
        }
        if (hard) {
            branch = 2;
            for (int h = 0; h < 2; h++) w[h] = hard == 1 ? -wr[h] : -w0[h];
            tau = sqrt(rho2 - (hard == 1 ? psi_reg : psi0));
        } else {
            const double lo = spw_max(on[0] ? fabs(gh[0]) / rho - d[0] : -inf, on[1] ? fabs(gh[1]) / rho - d[1] : -inf);
            const SecularRoot sr = secular_root(
                [&](double sg, double *psi, double *T) {
                    double p[2], q[2];
                    for (int h = 0; h < 2; h++) {
                        const double den = on[h] ? d[h] + sg : 1.0;
                        const double t = on[h] ? secular_w(gh[h], den) : 0.0;
                        p[h] = t * t;
                        q[h] = t == 0.0 ? 0.0 : t * t / den;
                    }
                    *psi = spw_sum(p[0], p[1]);
                    *T = spw_sum(q[0], q[1]);
                },
                rho, lo > sigma_lo ? lo : sigma_lo, sqrt(g2) / rho);
            sigma = sr.sigma;
            for (int h = 0; h < 2; h++) w[h] = on[h] ? -secular_w(gh[h], d[h] + sigma) : 0.0;
        }
        mu = sigma - lam_min;
    }
    ws[idx[0]] = w[0]; ws[idx[1]] = w[1];
    __syncthreads();

    // ---- the point: lane = coordinate
    double x[2], v[2] = {0.0, 0.0};
    for (int h = 0; h < 2; h++) {
        double y = 0.0;
        if (on[h]) for (int k = 0; k < n; k++) y = __builtin_fma(G[k * str + idx[h]], ws[k], y);
        x[h] = y;
        if (branch == 2 && on[h]) v[h] = G[kmin * str + idx[h]];
    }
    if (branch == 2) {
        const double vmax = spw_max(fabs(v[0]), fabs(v[1]));
        const unsigned long long at0 = __ballot(on[0] && fabs(v[0]) == vmax), at1 = __ballot(on[1] && fabs(v[1]) == vmax);
        const double lead = at0 ? __shfl(v[0], __builtin_ctzll(at0), 64) : __shfl(v[1], __builtin_ctzll(at1 | (1ull << 63)), 64);
        const double st = lead < 0.0 ? -tau : tau;
        x[0] += st * v[0]; x[1] += st * v[1];
    }
    for (int h = 0; h < 2; h++) {
        x[h] = (x[h] - bi[h] / (2.0 * si[h])) / si[h];
        xs[idx[h]] = on[h] ? x[h] : 0.0;
    }
    __syncthreads();
    double fx[2] = {0.0, 0.0};
    for (int h = 0; h < 2; h++) {
        double px = 0.0;
        if (on[h]) for (int j = 0; j < n; j++) px = __builtin_fma(Pg[j * n + idx[h]], xs[j], px);
        fx[h] = on[h] ? x[h] * (px + qi[h]) : 0.0;
    }
    const double f = spw_sum(fx[0], fx[1]) + a.r0s[b];
    const bool bad = __ballot((on[0] && !(fabs(x[0]) < inf)) || (on[1] && !(fabs(x[1]) < inf))) != 0 || !(fabs(f) < inf) || !(fabs(mu) < inf);

    for (int h = 0; h < 2; h++)
        if (on[h]) {
            a.x[b * n + idx[h]] = x[h];
            a.lam[b * n + rank[h]] = lamk[h];
        }
    if (lane == 0) {
        a.bound[b] = f;
        a.mu[b] = mu;
        a.sweeps[b] = jr.sweeps;
        a.branch[b] = branch;
        a.status[b] = (bad || jr.degenerate) ? 2 : (jr.converged ? 0 : 1);
    }
}

__global__ __launch_bounds__(64) void spectral_wide_kernel(SpectralSmallArgs a) {
    extern __shared__ __attribute__((aligned(16))) double spw_lds[];
    const int lane = threadIdx.x;
    for (;;) {
        // the branch-free ticket draw of spectral_small_kernel, for its reason
        int tk = __hip_atomic_fetch_add(a.ticket, lane == 0 ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tk = __builtin_amdgcn_readfirstlane(tk);
        if (tk >= a.B) break;
        spw_problem(a, spw_lds, tk, lane);
    }
}

}  // namespace
}  // namespace qcqpmi
