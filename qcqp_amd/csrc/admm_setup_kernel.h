// admm_setup_kernel (n <= 64) and admm_setup_wide_kernel (65 <= n <= 128; any n <= 128 is computed correctly, the launcher sends
// n <= 64 to the narrow kernel) -- rho_b by the reference's rule and Minv_b = (2 (P0_b + rho_b m I))^-1 for a batch of small problems
// from ONE eigendecomposition each, inside one persistent launch.  admm_setup.h has the stages and the order of every sum.  Included
// by spectral_small.hip, the one unit that holds the two eigen-solvers (the kernels sit in an unnamed namespace: a header for that
// unit alone).
//
// Layout.  ONE WAVEFRONT PER PROBLEM, one wavefront per workgroup.  Narrow LDS: As and Qs (n2 rows of 65 doubles each), the rotations
// of a Jacobi round and w (64).  Wide LDS: G (n2 columns of n2 + 1 doubles: P0_b, then its eigenvectors), two row buffers for the
// Rayleigh quotients and w (128 each); a lane holds the indices l and l + 64 (slot 0 and slot 1).  lam_k stays in its lane's registers.
#pragma once

#include "admm_setup.h"
#include "admm_setup_rule.h"
#include "dev_util.h"
#include "jacobi_small.h"
#include "jacobi_wide.h"

namespace qcqpmi {
namespace {

constexpr int AS_VECS = 1, AS_VEC = 64;          // narrow: w
constexpr int ASW_VECS = 3, ASW_VEC = 128;       // wide: two row buffers, w
constexpr int AS_ROWS = 4;                       // rows of Minv_b that a lane accumulates together: one read of its own operand serves four

__device__ inline double as_wave_min(double v) { return -wave_max(-v); }
__device__ inline double as_wave_min2(double v0, double v1) { return as_wave_min(v0 < v1 ? v0 : v1); }
__device__ inline bool as_finite(double v) { return fabs(v) < __builtin_huge_val(); }

// rho_b and the verdict on a given rho, the same for both widths; returns whether Minv_b is to be formed
__device__ inline bool as_rho(const AdmmSetupArgs &a, double lmin, double *rho) {
    *rho = a.has_rho ? a.rho : admm_setup_rho(lmin, a.m);
    return !(a.has_rho && admm_setup_rho_too_small(lmin, a.m, a.rho));
}

__device__ inline void as_problem(const AdmmSetupArgs &a, double *lds, int64_t b, int lane) {
    const int n = a.n, n2 = (n + 1) & ~1;
    double *As = lds, *Qs = As + n2 * JACOBI_STR, *rot = Qs + n2 * JACOBI_STR;
    double *ws = rot + JACOBI_ROT_DOUBLES;
    const bool on = lane < n;
    const int il = on ? lane : 0;
    const double *Pg = a.P0s + b * n * n;
    double *Mg = a.Minvs + b * n * n;
    const double inf = __builtin_huge_val();
    __syncthreads();             // the wave is done with the LDS image of its previous problem

    // ---- stage: A_b = P0_b with zero padding
    bool asym = false;
    for (int e = lane; e < n2 * n2; e += 64) {
        const int i = e / n2, j = e - i * n2;
        double v = 0.0;
        if (i < n && j < n) {
            v = Pg[i * n + j];
            asym = asym || (j >= i && !(v == Pg[j * n + i]));
        }
        As[i * JACOBI_STR + j] = v;
    }
    if (asym) a.ticket[1] = 1;
    __syncthreads();

    // ---- eigendecomposition
    const JacobiResult jr = jacobi_small(As, Qs, rot, n2, lane, a.max_sweeps, a.tol);

    // ---- lambda_min, rho, the weights: lane = eigen-index
    const double lamk = on ? As[lane * JACOBI_STR + lane] : 0.0;
    const double lmin = as_wave_min(on ? lamk : inf);
    double rho;
    const bool form = as_rho(a, lmin, &rho);
    const double w = on ? admm_setup_weight(lamk, rho, a.m) : 0.0;
    ws[lane] = w;
    bool bad = !as_finite(lmin) || !as_finite(rho) || __ballot(on && !as_finite(w)) != 0;
    __syncthreads();             // w for every lane; Qs as the last round (or the identity of a diagonal P0_b) left it

    // ---- Minv_b: lane = column j, rows i in blocks
    if (form) {
        bool nf = false;
        for (int i0 = 0; i0 < n; i0 += AS_ROWS) {
            int ir[AS_ROWS];
            double acc[AS_ROWS];
#pragma unroll
            for (int u = 0; u < AS_ROWS; u++) { ir[u] = i0 + u < n ? i0 + u : n - 1; acc[u] = 0.0; }
            for (int k = 0; k < n; k++) {
                const double *q = Qs + k * JACOBI_STR;
                const double uj = q[il], wk = ws[k];
#pragma unroll
                for (int u = 0; u < AS_ROWS; u++) acc[u] = __builtin_fma(q[ir[u]] * uj, wk, acc[u]);
            }
#pragma unroll
            for (int u = 0; u < AS_ROWS; u++)
                if (on && i0 + u < n) {
                    Mg[(i0 + u) * n + lane] = acc[u];
                    nf = nf || !as_finite(acc[u]);
                }
        }
        bad = bad || __ballot(nf) != 0;
    }
    if (lane == 0) {
        a.rhos[b] = rho;
        a.lambda_min[b] = lmin;
        a.sweeps[b] = jr.sweeps;
        a.status[b] = !form ? 3 : ((bad || jr.degenerate) ? 2 : (jr.converged ? 0 : 1));
    }
}

__global__ __launch_bounds__(64) void admm_setup_kernel(AdmmSetupArgs a) {
    extern __shared__ __attribute__((aligned(16))) double as_lds[];
    const int lane = threadIdx.x;
    for (;;) {
        // the branch-free ticket draw of spectral_small_kernel, for its reason
        int tk = __hip_atomic_fetch_add(a.ticket, lane == 0 ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tk = __builtin_amdgcn_readfirstlane(tk);
        if (tk >= a.B) break;
        as_problem(a, as_lds, tk, lane);
    }
}

__device__ inline void asw_problem(const AdmmSetupArgs &a, double *lds, int64_t b, int lane) {
    const int n = a.n, n2 = (n + 1) & ~1, str = jacobi_wide_stride(n2);
    double *G = lds, *row0 = G + jacobi_wide_doubles(n2), *row1 = row0 + ASW_VEC, *ws = row1 + ASW_VEC;
    const double *Pg = a.P0s + b * n * n;
    double *Mg = a.Minvs + b * n * n;
    const double inf = __builtin_huge_val();
    int idx[2], il[2];
    bool on[2];
    for (int h = 0; h < 2; h++) {
        idx[h] = lane + 64 * h;
        on[h] = idx[h] < n;
        il[h] = on[h] ? idx[h] : 0;
    }
    __syncthreads();             // the wave is done with the LDS image of its previous problem

    // ---- stage: G = P0_b with zero padding, entry (i, j) by the lane of j
    bool asym = false;
    for (int i = 0; i < n2; i++) {
        for (int h = 0; h < 2; h++) {
            const int j = idx[h];
            if (j >= n2) continue;
            double v = 0.0;
            if (i < n && j < n) {
                v = Pg[i * n + j];
                asym = asym || (j >= i && !(v == Pg[j * n + i]));
            }
            G[j * str + i] = v;
        }
    }
    if (asym) a.ticket[1] = 1;

    // ---- eigendecomposition: G becomes Q, column k = eigenvector k
    const JacobiWideResult jr = jacobi_wide(G, n2, str, lane, a.max_sweeps, a.tol);

    // ---- Rayleigh quotients: lane = eigen-index
    double lamk[2] = {0.0, 0.0};
    for (int i = 0; i < n; i++) {
        double *arow = (i & 1) ? row1 : row0;
        for (int h = 0; h < 2; h++)
            if (on[h]) arow[idx[h]] = Pg[i * n + idx[h]];
        __syncthreads();         // (one barrier per row: the buffer written next was read before the barrier of the row before)
        for (int h = 0; h < 2; h++) {
            if (!on[h]) continue;
            const double *u = G + idx[h] * str;
            double t = 0.0;
            for (int j = 0; j < n; j++) t = __builtin_fma(arow[j], u[j], t);
            lamk[h] = __builtin_fma(u[i], t, lamk[h]);
        }
    }

    // ---- lambda_min, rho, the weights
    const double lmin = as_wave_min2(on[0] ? lamk[0] : inf, on[1] ? lamk[1] : inf);
    double rho;
    const bool form = as_rho(a, lmin, &rho);
    double w[2];
    for (int h = 0; h < 2; h++) {
        w[h] = on[h] ? admm_setup_weight(lamk[h], rho, a.m) : 0.0;
        ws[idx[h]] = w[h];
    }
    bool bad = !as_finite(lmin) || !as_finite(rho) || __ballot((on[0] && !as_finite(w[0])) || (on[1] && !as_finite(w[1]))) != 0;
    __syncthreads();

    // ---- Minv_b: lane = columns j and j + 64, rows i in blocks
    if (form) {
        bool nf = false;
        for (int i0 = 0; i0 < n; i0 += AS_ROWS) {
            int ir[AS_ROWS];
            double acc[AS_ROWS][2];
#pragma unroll
            for (int u = 0; u < AS_ROWS; u++) { ir[u] = i0 + u < n ? i0 + u : n - 1; acc[u][0] = acc[u][1] = 0.0; }
            for (int k = 0; k < n; k++) {
                const double *q = G + k * str;
                const double uj0 = q[il[0]], uj1 = q[il[1]], wk = ws[k];
#pragma unroll
                for (int u = 0; u < AS_ROWS; u++) {
                    const double ui = q[ir[u]];
                    acc[u][0] = __builtin_fma(ui * uj0, wk, acc[u][0]);
                    acc[u][1] = __builtin_fma(ui * uj1, wk, acc[u][1]);
                }
            }
#pragma unroll
            for (int u = 0; u < AS_ROWS; u++)
                for (int h = 0; h < 2; h++)
                    if (on[h] && i0 + u < n) {
                        Mg[(i0 + u) * n + idx[h]] = acc[u][h];
                        nf = nf || !as_finite(acc[u][h]);
                    }
        }
        bad = bad || __ballot(nf) != 0;
    }
    if (lane == 0) {
        a.rhos[b] = rho;
        a.lambda_min[b] = lmin;
        a.sweeps[b] = jr.sweeps;
        a.status[b] = !form ? 3 : ((bad || jr.degenerate) ? 2 : (jr.converged ? 0 : 1));
    }
}

__global__ __launch_bounds__(64) void admm_setup_wide_kernel(AdmmSetupArgs a) {
    extern __shared__ __attribute__((aligned(16))) double asw_lds[];
    const int lane = threadIdx.x;
    for (;;) {
        // the branch-free ticket draw of spectral_small_kernel, for its reason
        int tk = __hip_atomic_fetch_add(a.ticket, lane == 0 ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tk = __builtin_amdgcn_readfirstlane(tk);
        if (tk >= a.B) break;
        asw_problem(a, asw_lds, tk, lane);
    }
}

}  // namespace
}  // namespace qcqpmi
