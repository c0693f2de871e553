// spectral_small_kernel -- suggest(SPECTRAL) for a batch of SMALL problems (n <= 64) whose constraints aggregate to one sphere or one
// ball: the symmetric eigendecomposition (cyclic Jacobi, jacobi_small.h) and the secular equation (spectral_solve.h) of every problem
// inside one persistent launch.  spectral_small.h has the mathematics, the stages and the order of every sum.
//
// Layout.  ONE WAVEFRONT PER PROBLEM, one wavefront per workgroup: a wave draws a problem from a global counter, keeps A_b and Q_b
// (n2 rows of 65 doubles each) in its LDS with the rotations of a Jacobi round and five vectors of 64 (g, h, lam, w, x) behind them,
// and never waits for another wave: the barriers are those of a one-wave workgroup and order the wave's own LDS traffic where lanes
// read what other lanes wrote.  The row stride of 65 makes every access conflict-free, lane = column or lane = row (jacobi_small.h).
#include "spectral_small.h"

#include "dev_util.h"
#include "jacobi_small.h"
#include "small_batch.h"     // the launchers: small_wave_workgroups, small_launch
#include "spectral_solve.h"

namespace qcqpmi {
namespace {

constexpr int SP_VECS = 5;       // g, h, lam, w, x: 64 doubles each

__device__ inline double sp_wave_min(double v) { return -wave_max(-v); }

__device__ inline void sp_problem(const SpectralSmallArgs &a, double *lds, int64_t b, int lane) {
    const int n = a.n, n2 = (n + 1) & ~1;
    double *As = lds, *Qs = As + n2 * JACOBI_STR, *rot = Qs + n2 * JACOBI_STR;
    double *gs = rot + JACOBI_ROT_DOUBLES, *hs = gs + 64, *lams = hs + 64, *ws = lams + 64, *xs = ws + 64;
    const bool on = lane < n;
    const int il = on ? lane : 0;
    const double *Pg = a.P0s + b * n * n, *qg = a.q0s + b * n, *ag = a.agg + b * a.agg_stride;
    const double inf = __builtin_huge_val();
    __syncthreads();             // the wave is done with the LDS image of its previous problem

    // ---- stage: s, h, then A_b = P0_b / (s_i s_j) with zero padding
    const double ai = ag[il], bi = ag[n + il], gamma = ag[2 * n];
    const double si = sqrt(ai), hi = bi / (2.0 * ai), qi = qg[il];
    gs[lane] = on ? si : 1.0;    // (s for the staging; g below)
    hs[lane] = on ? hi : 0.0;
    __syncthreads();
    bool asym = false;
    for (int e = lane; e < n2 * n2; e += 64) {
        const int i = e / n2, j = e - i * n2;
        double v = 0.0;
        if (i < n && j < n) {
            const double p = Pg[i * n + j];
            asym = asym || (j >= i && !(p == Pg[j * n + i]));
            v = p / (gs[i] * gs[j]);
        }
        As[i * JACOBI_STR + j] = v;
    }
    if (asym) a.ticket[1] = 1;
    double ph = 0.0;
    if (on) for (int j = 0; j < n; j++) ph = __builtin_fma(Pg[j * n + lane], hs[j], ph);
    const double rho2 = wave_sum_tree(on ? bi * bi / (4.0 * ai) : 0.0) - gamma;
    const double rho = sqrt(rho2);
    __syncthreads();             // every lane has read s
    gs[lane] = on ? (0.5 * qi - ph) / si : 0.0;
    __syncthreads();

    // ---- eigendecomposition
    const JacobiResult jr = jacobi_small(As, Qs, rot, n2, lane, a.max_sweeps, a.tol);

    // ---- spectrum: lane = eigen-index
    const double lamk = on ? As[lane * JACOBI_STR + lane] : 0.0;
    double gh = 0.0;
    if (on) for (int i = 0; i < n; i++) gh = __builtin_fma(Qs[lane * JACOBI_STR + i], gs[i], gh);
    lams[lane] = lamk;
    __syncthreads();
    int rank = 0;
    for (int j = 0; j < n; j++) { const double lj = lams[j]; rank += (lj < lamk || (lj == lamk && j < lane)) ? 1 : 0; }
    const double lam_min = sp_wave_min(on ? lamk : inf), lam_abs = wave_max(on ? fabs(lamk) : 0.0);
    const int kmin = __builtin_ctzll(__ballot(on && rank == 0) | (1ull << 63));
    const double d = lamk - lam_min;
    const double g2 = wave_sum_tree(gh * gh);

    // ---- branch
    int branch = 1;
    double w = 0.0, sigma = 0.0, tau = 0.0, mu = 0.0;
    bool interior = false;
    if (!a.relop_eq && lam_min > 0.0) {
        w = on ? secular_w(gh, lamk) : 0.0;
        interior = wave_sum_tree(w * w) <= rho2;
    }
    if (interior) {
        branch = 0;
        w = -w;
    } else {
        const double sigma_lo = (!a.relop_eq && lam_min > 0.0) ? lam_min : 0.0;
        int hard = 0;
        double wr = 0.0, w0 = 0.0, psi_reg = 0.0, psi0 = 0.0;
        if (sigma_lo == 0.0) {
            const bool inL = d <= SPECTRAL_HARD_THR * lam_abs;
            w0 = on ? secular_w(gh, d) : 0.0;
            wr = inL ? 0.0 : w0;
            const double gL2 = wave_sum_tree(inL ? gh * gh : 0.0);
            psi_reg = wave_sum_tree(wr * wr);
            psi0 = wave_sum_tree(w0 * w0);
            hard = spectral_hard_case(gL2, g2, psi_reg, psi0, rho2);
        }
        if (hard) {
            branch = 2;
            w = hard == 1 ? -wr : -w0;
            tau = sqrt(rho2 - (hard == 1 ? psi_reg : psi0));
        } else {
            const double lo = wave_max(on ? fabs(gh) / rho - d : -inf);
            const SecularRoot sr = secular_root(
                [&](double sg, double *psi, double *T) {
                    const double den = on ? d + sg : 1.0;
                    const double t = on ? secular_w(gh, den) : 0.0;
                    *psi = wave_sum_tree(t * t);
                    *T = wave_sum_tree(t == 0.0 ? 0.0 : t * t / den);
                },
                rho, lo > sigma_lo ? lo : sigma_lo, sqrt(g2) / rho);
            sigma = sr.sigma;
            w = on ? -secular_w(gh, d + sigma) : 0.0;
        }
        mu = sigma - lam_min;
    }
    ws[lane] = w;
    __syncthreads();

    // ---- the point: lane = coordinate
    double y = 0.0;
    if (on) for (int k = 0; k < n; k++) y = __builtin_fma(Qs[k * JACOBI_STR + lane], ws[k], y);
    if (branch == 2) {
        const double v = on ? Qs[kmin * JACOBI_STR + lane] : 0.0;
        const double vmax = wave_max(fabs(v));
        const int at = __builtin_ctzll(__ballot(on && fabs(v) == vmax) | (1ull << 63));
        const double lead = __shfl(v, at, 64);
        y += (lead < 0.0 ? -tau : tau) * v;
    }
    const double x = (y - bi / (2.0 * si)) / si;
    xs[lane] = on ? x : 0.0;
    __syncthreads();
    double px = 0.0;
    if (on) for (int j = 0; j < n; j++) px = __builtin_fma(Pg[j * n + lane], xs[j], px);
    const double f = wave_sum_tree(on ? x * (px + qi) : 0.0) + a.r0s[b];
    const bool bad = __ballot(on && !(fabs(x) < inf)) != 0 || !(fabs(f) < inf) || !(fabs(mu) < inf);

    if (on) {
        a.x[b * n + lane] = x;
        a.lam[b * n + rank] = lamk;
    }
    if (lane == 0) {
        a.bound[b] = f;
        a.mu[b] = mu;
        a.sweeps[b] = jr.sweeps;
        a.branch[b] = branch;
        a.status[b] = (bad || jr.degenerate) ? 2 : (jr.converged ? 0 : 1);
    }
}

__global__ __launch_bounds__(64) void spectral_small_kernel(SpectralSmallArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sp_lds[];
    const int lane = threadIdx.x;
    for (;;) {
        // The draw has NO branch on the lane: every lane adds (lane 0 one, the others nothing) and the wave takes lane 0's answer.
        // Written as `if (lane == 0) tk = add(1)`, that branch was threaded together with the `if (lane == 0)` that ends
        // sp_problem: lanes 1..63 then came back to the loop head without lane 0, read their own 0 as the ticket and solved
        // problem 0 for ever (seen in the unit's assembly: a loop around the whole body that only lane 0 leaves).
        int tk = __hip_atomic_fetch_add(a.ticket, lane == 0 ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tk = __builtin_amdgcn_readfirstlane(tk);
        if (tk >= a.B) break;
        sp_problem(a, sp_lds, tk, lane);
    }
}

}  // namespace

size_t spectral_small_lds_bytes(int n) {
    const int n2 = (n + 1) & ~1;
    return (jacobi_small_doubles(n2) + SP_VECS * 64) * sizeof(double);
}

int spectral_small_workgroups(int n, int64_t B, int device) {
    return small_wave_workgroups((const void *)spectral_small_kernel, spectral_small_lds_bytes(n), B, device);
}

int spectral_small_launch(const SpectralSmallArgs &a, int wgs, hipStream_t st) {
    return small_launch(spectral_small_kernel, spectral_small_lds_bytes(a.n), a, wgs, 64, true, st);
}

}  // namespace qcqpmi

// ---- the wide kernel (65 <= n <= 128, spectral_wide.h): same unit, the kernel in a file of its own
#include "spectral_wide_kernel.h"

namespace qcqpmi {

size_t spectral_wide_lds_bytes(int n) {
    const int n2 = (n + 1) & ~1;
    return (jacobi_wide_doubles(n2) + SPW_VECS * SPW_VEC) * sizeof(double);
}

int spectral_wide_workgroups(int n, int64_t B, int device) {
    return small_wave_workgroups((const void *)spectral_wide_kernel, spectral_wide_lds_bytes(n), B, device);
}

int spectral_wide_launch(const SpectralSmallArgs &a, int wgs, hipStream_t st) {
    return small_launch(spectral_wide_kernel, spectral_wide_lds_bytes(a.n), a, wgs, 64, true, st);
}

}  // namespace qcqpmi

// ---- the device-side setup of batched ADMM (admm_setup.h): same unit -- it runs the two eigen-solvers --, the kernels in a file of their own
#include "admm_setup_kernel.h"

namespace qcqpmi {

size_t admm_setup_lds_bytes(int n) {
    const int n2 = (n + 1) & ~1;
    return (n > ADMM_SETUP_SMALL_MAXN ? jacobi_wide_doubles(n2) + ASW_VECS * ASW_VEC : jacobi_small_doubles(n2) + AS_VECS * AS_VEC) * sizeof(double);
}

typedef void (*AdmmSetupKernel)(AdmmSetupArgs);

static AdmmSetupKernel admm_setup_function(int n) { return n > ADMM_SETUP_SMALL_MAXN ? admm_setup_wide_kernel : admm_setup_kernel; }

int admm_setup_workgroups(int n, int64_t B, int device) {
    return small_wave_workgroups((const void *)admm_setup_function(n), admm_setup_lds_bytes(n), B, device);
}

int admm_setup_launch(const AdmmSetupArgs &a, int wgs, hipStream_t st) {
    return small_launch(admm_setup_function(a.n), admm_setup_lds_bytes(a.n), a, wgs, 64, true, st);
}

}  // namespace qcqpmi
